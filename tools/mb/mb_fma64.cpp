// Microbenchmark (GPU box, analysis only): the chip's fp64 vector FMA rate, the ceiling of the fixed-order product
// kernel of shyft_amd/csrc/kernels/ok.hip. Every lane runs 16 independent v_fma_f64 chains whose multiplier is a
// scalar operand, as that kernel's inner loop does; nothing touches memory inside the loop. Prints one JSON line.
// build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -o tools/mb/mb_fma64 tools/mb/mb_fma64.cpp
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

constexpr int CHAINS = 16, UNROLL = 8;

__global__ __launch_bounds__(256) void fma64_kernel(const double* __restrict__ mul, int iters, double* __restrict__ out) {
    double acc[CHAINS];
    const double x = 1.0 + 1e-9 * double(threadIdx.x);
#pragma unroll
    for (int i = 0; i < CHAINS; ++i) acc[i] = double(i);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const double m = mul[u];  // wave-uniform: a scalar load, the SGPR operand of the FMA
#pragma unroll
            for (int i = 0; i < CHAINS; ++i) acc[i] = __builtin_fma(m, x, acc[i]);
        }
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < CHAINS; ++i) s += acc[i];
    out[size_t(blockIdx.x) * blockDim.x + threadIdx.x] = s;
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 4096, reps = argc > 2 ? atoi(argv[2]) : 5;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int blocks = prop.multiProcessorCount * 8;  // 8 waves per SIMD
    double host_mul[UNROLL];
    for (int u = 0; u < UNROLL; ++u) host_mul[u] = 1e-7 * (u + 1);
    double *d_mul = nullptr, *d_out = nullptr;
    CK(hipMalloc(&d_mul, sizeof host_mul));
    CK(hipMalloc(&d_out, size_t(blocks) * 256 * sizeof(double)));
    CK(hipMemcpy(d_mul, host_mul, sizeof host_mul, hipMemcpyHostToDevice));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    float best = 1e30f;
    for (int r = 0; r < reps + 1; ++r) {  // the first pass warms up
        CK(hipEventRecord(a));
        hipLaunchKernelGGL(fma64_kernel, dim3(blocks), dim3(256), 0, 0, d_mul, iters, d_out);
        CK(hipGetLastError());
        CK(hipEventRecord(b));
        CK(hipEventSynchronize(b));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, a, b));
        if (r > 0) best = std::min(best, ms);
    }
    const double fmas = double(blocks) * 256.0 * double(iters) * UNROLL * CHAINS;
    printf("{\"bench\": \"mb_fma64\", \"device\": \"%s\", \"cus\": %d, \"fma\": %.0f, \"ms\": %.4f, \"fma_per_s\": %.4e}\n",
           prop.name, prop.multiProcessorCount, fmas, best, fmas / (best * 1e-3));
    CK(hipFree(d_mul));
    CK(hipFree(d_out));
    return 0;
}
