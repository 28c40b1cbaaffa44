// Measurement entry of tools/ok_bench.py: the ordinary-kriging kernels (kernels/ok.hip) timed one by one with HIP
// events next to rocBLAS dgemm on the same two product shapes, called as kernels/btk.hip calls it. Not on any
// product path: ok_run itself makes no rocBLAS call.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../include_internal/region_impl.h"

using namespace shyft_hip_impl;

namespace {

void blas_check(rocblas_status s, const char* what) {
    if (s != rocblas_status_success) throw std::runtime_error(std::string(what) + ": " + rocblas_status_to_string(s));
}

// largest |a - b| through the bit pattern of the non-negative difference (ordered like the integers)
__global__ __launch_bounds__(256) void ok_maxdiff_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                         size_t n, unsigned long long* __restrict__ out) {
    double worst = 0.0;
    for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
        const double d = fabs(a[i] - b[i]);
        worst = d > worst || d != d ? (d != d ? 1.0 / 0.0 : d) : worst;
    }
    atomicMax(out, (unsigned long long)__double_as_longlong(worst));
}

struct event_pair {
    hipEvent_t a = nullptr, b = nullptr;
    event_pair() {
        hip_check(hipEventCreate(&a), "hipEventCreate");
        hip_check(hipEventCreate(&b), "hipEventCreate");
    }
    event_pair(const event_pair&) = delete;
    event_pair& operator=(const event_pair&) = delete;
    ~event_pair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    double ms() const {
        float t = 0.f;
        hip_check(hipEventElapsedTime(&t, a, b), "hipEventElapsedTime");
        return double(t);
    }
};

// splitmix64 -> [0, 1)
double u01(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return double(z >> 11) * (1.0 / 9007199254740992.0);
}

}  // namespace

int shyft_hip_ok_bench(int device, size_t n_sources, size_t n, size_t n_dst, size_t dst_block, int reps,
                       double* out_ms) {
    if (!out_ms) return fail(nullptr, "shyft_hip_ok_bench: null argument");
    try {
        const size_t S = n_sources, N = S + 1, T = n, m = n_dst;
        if (S < 2 || S > 4096 || T == 0 || T > 4096 || m == 0 || m > (size_t(1) << 30) || reps < 1)
            throw std::runtime_error("shyft_hip_ok_bench: shape out of range");
        if (device >= 0) hip_check(hipSetDevice(device), "hipSetDevice");
        const size_t blk = std::min(m, dst_block ? dst_block : ok_default_dst_block());
        const size_t ldw = size_t(ok_product_ldl(int(S))), ldo = size_t(ok_product_ldl(int(T)));
        // generated inputs: points in a 20 km x 20 km x 1 km box, left factors uniform in [-1, 1)
        uint64_t seed = 1;
        std::vector<double> src(3 * S), dst(3 * m), left_t(N * ldw, 0.0), left_cm(N * S), obs_t(S * ldo, 0.0), obs_cm(S * T);
        for (size_t i = 0; i < S; ++i) {
            src[3 * i] = 20000.0 * u01(seed);
            src[3 * i + 1] = 20000.0 * u01(seed);
            src[3 * i + 2] = 1000.0 * u01(seed);
        }
        for (size_t i = 0; i < m; ++i) {
            dst[3 * i] = 20000.0 * u01(seed);
            dst[3 * i + 1] = 20000.0 * u01(seed);
            dst[3 * i + 2] = 1000.0 * u01(seed);
        }
        for (size_t s = 0; s < S; ++s)
            for (size_t j = 0; j < N; ++j) left_t[j * ldw + s] = left_cm[j + s * N] = 2.0 * u01(seed) - 1.0;
        for (size_t t = 0; t < T; ++t)
            for (size_t s = 0; s < S; ++s) obs_t[s * ldo + t] = obs_cm[s + t * S] = 10.0 + 5.0 * (2.0 * u01(seed) - 1.0);

        hipStream_t st = nullptr;
        hip_check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
        std::unique_ptr<std::remove_pointer<hipStream_t>::type, void (*)(hipStream_t)> stream(
            st, [](hipStream_t x) { (void)hipStreamDestroy(x); });
        rocblas_handle blas = nullptr;
        blas_check(rocblas_create_handle(&blas), "rocblas_create_handle");
        std::unique_ptr<std::remove_pointer<rocblas_handle>::type, void (*)(rocblas_handle)> blas_guard(
            blas, [](rocblas_handle h) { (void)rocblas_destroy_handle(h); });
        blas_check(rocblas_set_stream(blas, st), "rocblas_set_stream");

        dbuf<double> d_src, d_dst, d_left_t, d_left_cm, d_obs_t, d_obs_cm, d_BW, d_out, d_Bf, d_Wf, d_outf;
        dbuf<unsigned long long> d_diff;
        auto up = [&](dbuf<double>& b, const std::vector<double>& v) {
            b.alloc(v.size());
            hip_check(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, st), "upload");
        };
        up(d_src, src);
        up(d_dst, dst);
        up(d_left_t, left_t);
        up(d_left_cm, left_cm);
        up(d_obs_t, obs_t);
        up(d_obs_cm, obs_cm);
        d_BW.alloc((2 * S + 1) * blk);
        d_out.alloc(T * m);
        d_Bf.alloc(N * m);
        d_Wf.alloc(S * m);
        d_outf.alloc(T * m);
        d_diff.alloc(1);
        hip_check(hipMemsetAsync(d_diff.p, 0, sizeof(unsigned long long), st), "memset");
        const double c = 1.0, k = -3.0 / 10000.0, zs = 1.0, one = 1.0, zero = 0.0;

        const size_t nblk = (m + blk - 1) / blk;
        std::vector<event_pair> ev(3 * nblk), evb(2);
        double best[5] = {1e300, 1e300, 1e300, 1e300, 1e300};
        for (int rep = 0; rep < reps; ++rep) {
            double* d_B = d_BW.p;
            double* d_W = d_BW.p + N * blk;
            for (size_t b = 0; b < nblk; ++b) {
                const size_t d0 = b * blk, mb = std::min(blk, m - d0);
                hip_check(hipEventRecord(ev[3 * b].a, st), "record");
                hip_check(launch_ok_cov(d_src.p, int(S), d_dst.p + 3 * d0, int(mb), c, k, zs, 0, d_B, mb, st), "cov");
                hip_check(hipEventRecord(ev[3 * b].b, st), "record");
                hip_check(hipEventRecord(ev[3 * b + 1].a, st), "record");
                hip_check(launch_ok_product(d_left_t.p, int(ldw), int(S), d_B, mb, int(N), int(mb), d_W, mb, st), "weights");
                hip_check(hipEventRecord(ev[3 * b + 1].b, st), "record");
                hip_check(hipEventRecord(ev[3 * b + 2].a, st), "record");
                hip_check(launch_ok_product(d_obs_t.p, int(ldo), int(T), d_W, mb, int(S), int(mb), d_out.p + d0, m, st),
                          "values");
                hip_check(hipEventRecord(ev[3 * b + 2].b, st), "record");
            }
            // rocBLAS on the whole shapes, as btk.hip calls it: W' (m x S) = B' (m x N) L (N x S); out' (m x T) = W' obs
            hip_check(launch_ok_cov(d_src.p, int(S), d_dst.p, int(m), c, k, zs, 0, d_Bf.p, m, st), "cov");
            hip_check(hipEventRecord(evb[0].a, st), "record");
            blas_check(rocblas_dgemm(blas, rocblas_operation_none, rocblas_operation_none, rocblas_int(m), rocblas_int(S),
                                     rocblas_int(N), &one, d_Bf.p, rocblas_int(m), d_left_cm.p, rocblas_int(N), &zero,
                                     d_Wf.p, rocblas_int(m)),
                       "dgemm weights");
            hip_check(hipEventRecord(evb[0].b, st), "record");
            hip_check(hipEventRecord(evb[1].a, st), "record");
            blas_check(rocblas_dgemm(blas, rocblas_operation_none, rocblas_operation_none, rocblas_int(m), rocblas_int(T),
                                     rocblas_int(S), &one, d_Wf.p, rocblas_int(m), d_obs_cm.p, rocblas_int(S), &zero,
                                     d_outf.p, rocblas_int(m)),
                       "dgemm values");
            hip_check(hipEventRecord(evb[1].b, st), "record");
            hip_check(hipStreamSynchronize(st), "sync");
            double sum[3] = {0, 0, 0};
            for (size_t b = 0; b < nblk; ++b)
                for (int q = 0; q < 3; ++q) sum[q] += ev[3 * b + q].ms();
            for (int q = 0; q < 3; ++q) best[q] = std::min(best[q], sum[q]);
            best[3] = std::min(best[3], evb[0].ms());
            best[4] = std::min(best[4], evb[1].ms());
        }
        hipLaunchKernelGGL(ok_maxdiff_kernel, dim3(1024), dim3(256), 0, st, d_out.p, d_outf.p, T * m, d_diff.p);
        hip_check(hipGetLastError(), "maxdiff kernel");
        unsigned long long bits = 0;
        hip_check(hipMemcpyAsync(&bits, d_diff.p, sizeof bits, hipMemcpyDeviceToHost, st), "download");
        hip_check(hipStreamSynchronize(st), "sync");
        for (int q = 0; q < 5; ++q) out_ms[q] = best[q];
        double diff;
        static_assert(sizeof diff == sizeof bits, "");
        memcpy(&diff, &bits, sizeof diff);
        out_ms[5] = diff;
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}
