// Ordinary kriging for gfx950 (api/boostpython/api_interpolation.cpp:86-148, core/kriging.h:23-135).
//
// The reference builds A ((n+1) x (n+1): source covariances, a border of ones, A[n][n] = 0) and B ((n+1) x m:
// source-destination covariances over a row of ones), takes the first n rows of A^-1 B as weights W and
// evaluates out[t][d] = sum_s obs[t][s] W[s][d] step by step. Here A^-1 is made on the host (LU with partial
// pivoting) and the two products run on the device through ONE fixed-order fp64 kernel:
//
//   C[r][d] = sum_k L[r][k] R[k][d],   every output one chain acc = fma(L[r][k], R[k][d], acc) from 0.0, k ascending
//
// so the device result is bit-identical to the host restatement ok_host_run below (no rocBLAS, no MFMA: neither
// has a summation order this project can pin). Tiling of the product kernel:
//   - one destination per lane (R loads and C stores coalesced), OK_RT rows per lane as independent FMA chains;
//   - L[r][k] is wave-uniform and comes in k-major (transposed, row count padded to OK_RT) so the OK_RT values
//     of one k are contiguous: scalar loads, used as the SGPR operand of v_fma_f64;
//   - a workgroup is OK_NW waves on the SAME 64 destinations and OK_NW consecutive row tiles; the R panel
//     (OK_KT x 64) is staged through LDS once per workgroup and K tile (double-buffered, one barrier per tile),
//     so R is read from memory once per OK_RT * OK_NW rows.
// Row, destination and K remainders only mask loads and stores; no chain is ever split or reordered.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../detmath/detmath.h"
#include "../include_internal/region_impl.h"

using shyft_hip_impl::hip_check;

namespace {

// cov(src, dst) of the contract: h2 left to right as geo_point::zscaled_distance2 writes it (core/geo_point.h:49-58),
// EXPONENTIAL c exp(h k1), GAUSSIAN c exp(h2 k2) (core/kriging.h:26-64), k = k1 or k2 made once on the host
__host__ __device__ inline double ok_cov(double ax, double ay, double az, double bx, double by, double bz, double c,
                                         double k, double z_scale, bool gaussian) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    const double h2 = dx * dx + dy * dy + dz * dz * z_scale * z_scale;
    return c * detmath::exp((gaussian ? h2 : sqrt(h2)) * k);
}

double ok_k(const ok_args& a) { return a.cov_type == 0 ? -3.0 / (a.a * a.a) : -3.0 / a.a; }

// ---- device kernels ---------------------------------------------------------------------------------------------
constexpr int OK_COV_JB = 16;  // sources per thread of the covariance kernel

// B[j][d] = cov(src_j, dst_d) for j < n_src, B[n_src][d] = 1 (kriging::ordinary::build, core/kriging.h:121-133)
__global__ __launch_bounds__(256) void ok_cov_kernel(const double* __restrict__ src_xyz, int n_src,
                                                     const double* __restrict__ dst_xyz, int n_dst, double c, double k,
                                                     double z_scale, int gaussian, double* __restrict__ B, size_t ldb) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_dst) return;
    const double x = dst_xyz[3 * size_t(d)], y = dst_xyz[3 * size_t(d) + 1], z = dst_xyz[3 * size_t(d) + 2];
    const int j0 = blockIdx.y * OK_COV_JB, j1 = min(j0 + OK_COV_JB, n_src + 1);
    for (int j = j0; j < j1; ++j)
        B[size_t(j) * ldb + d] =
            j == n_src ? 1.0 : ok_cov(src_xyz[3 * j], src_xyz[3 * j + 1], src_xyz[3 * j + 2], x, y, z, c, k, z_scale, gaussian != 0);
}

constexpr int OK_RT = 16;  // rows (FMA chains) per lane
constexpr int OK_NW = 8;   // waves per workgroup = row tiles that share one staged R panel
constexpr int OK_KT = 32;  // k per staged panel
constexpr int OK_PF = OK_KT / OK_NW;  // panel rows each thread stages

template <bool FULL>
__device__ __forceinline__ void ok_tile(double (&acc)[OK_RT], const double* __restrict__ lt, int ldl,
                                        const double* panel, int kn) {
    if (FULL) {
#pragma unroll 4
        for (int k = 0; k < OK_KT; ++k) {
            const double r = panel[k * 64];
#pragma unroll
            for (int i = 0; i < OK_RT; ++i) acc[i] = __builtin_fma(lt[size_t(k) * ldl + i], r, acc[i]);
        }
    } else {
        for (int k = 0; k < kn; ++k) {
            const double r = panel[k * 64];
#pragma unroll
            for (int i = 0; i < OK_RT; ++i) acc[i] = __builtin_fma(lt[size_t(k) * ldl + i], r, acc[i]);
        }
    }
}

// C[r][d] = sum_{k < K} Lt[k][r] R[k][d] for r < rows, d < m. Lt is K x ldl with ldl >= rows rounded up to OK_RT.
__global__ __launch_bounds__(64 * OK_NW) void ok_product_kernel(const double* __restrict__ Lt, int ldl, int rows,
                                                               const double* __restrict__ R, size_t ldr, int K, int m,
                                                               double* __restrict__ C, size_t ldc) {
    __shared__ double panel[2][OK_KT][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    const int d = blockIdx.x * 64 + lane;
    const int r0 = (blockIdx.y * OK_NW + wave) * OK_RT;
    const bool active = r0 < rows;  // wave-uniform; an idle wave still stages its share of the panel
    const bool d_ok = d < m;

    double acc[OK_RT];
#pragma unroll
    for (int i = 0; i < OK_RT; ++i) acc[i] = 0.0;

    double pre[OK_PF];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < OK_PF; ++i) {
            const int k = k0 + wave + OK_NW * i;
            pre[i] = (d_ok && k < K) ? R[size_t(k) * ldr + d] : 0.0;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < OK_PF; ++i) panel[buf][wave + OK_NW * i][lane] = pre[i];
    };

    const int nt = (K + OK_KT - 1) / OK_KT;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const int k0 = t * OK_KT;
        if (t + 1 < nt) fetch(k0 + OK_KT);
        if (active) {
            const double* lt = Lt + size_t(k0) * ldl + r0;
            if (k0 + OK_KT <= K)
                ok_tile<true>(acc, lt, ldl, &panel[t & 1][0][lane], OK_KT);
            else
                ok_tile<false>(acc, lt, ldl, &panel[t & 1][0][lane], K - k0);
        }
        if (t + 1 < nt) stage((t + 1) & 1);
        __syncthreads();
    }
    if (active && d_ok) {
#pragma unroll
        for (int i = 0; i < OK_RT; ++i)
            if (r0 + i < rows) C[size_t(r0 + i) * ldc + d] = acc[i];
    }
}

// inverse by LU with partial pivoting: the algorithm of lu_inverse in kernels/btk.hip (LAPACK getrf/getri semantics)
std::vector<double> lu_inverse(const std::vector<double>& x, size_t n) {
    std::vector<double> lu(x);
    std::vector<size_t> piv(n);
    for (size_t k = 0; k < n; ++k) {
        size_t p = k;
        for (size_t i = k + 1; i < n; ++i)
            if (std::fabs(lu[i * n + k]) > std::fabs(lu[p * n + k])) p = i;
        piv[k] = p;
        if (lu[p * n + k] == 0.0) throw std::runtime_error("inv(): matrix is singular");
        if (p != k)
            for (size_t j = 0; j < n; ++j) std::swap(lu[k * n + j], lu[p * n + j]);
        for (size_t i = k + 1; i < n; ++i) {
            lu[i * n + k] /= lu[k * n + k];
            for (size_t j = k + 1; j < n; ++j) lu[i * n + j] -= lu[i * n + k] * lu[k * n + j];
        }
    }
    std::vector<double> r(n * n), b(n);
    for (size_t col = 0; col < n; ++col) {
        std::fill(b.begin(), b.end(), 0.0);
        b[col] = 1.0;
        for (size_t k = 0; k < n; ++k) std::swap(b[k], b[piv[k]]);
        for (size_t i = 0; i < n; ++i)
            for (size_t k = 0; k < i; ++k) b[i] -= lu[i * n + k] * b[k];
        for (size_t i = n; i-- > 0;) {
            for (size_t k = i + 1; k < n; ++k) b[i] -= lu[i * n + k] * b[k];
            b[i] /= lu[i * n + i];
        }
        for (size_t i = 0; i < n; ++i) r[i * n + col] = b[i];
    }
    return r;
}

// A^-1 of kriging::ordinary::build's A (core/kriging.h:85-98), row-major (n+1) x (n+1)
std::vector<double> ok_system_inverse(const ok_args& a) {
    const size_t n = a.n_sources, N = n + 1;
    const double k = ok_k(a);
    const bool gaussian = a.cov_type == 0;
    std::vector<double> A(N * N, 0.0);
    for (size_t i = 0; i < n; ++i) {
        const double* p = a.src_xyz + 3 * i;
        for (size_t j = i; j < n; ++j) {
            const double* q = a.src_xyz + 3 * j;
            A[i * N + j] = A[j * N + i] = ok_cov(p[0], p[1], p[2], q[0], q[1], q[2], a.c, k, a.z_scale, gaussian);
        }
        A[i * N + n] = A[n * N + i] = 1.0;
    }
    return lu_inverse(A, N);
}

void check_limits(const ok_args& a) {
    if (a.n_sources < 2) throw std::runtime_error("ordinary kriging: needs at least two sources");
    if (a.n_dst > size_t(INT32_MAX) || a.n_sources > 4096)
        throw std::runtime_error("ordinary kriging: too many sources or destinations");
}

}  // namespace

hipError_t launch_ok_cov(const double* d_src_xyz, int n_src, const double* d_dst_xyz, int n_dst, double c, double k,
                         double z_scale, int gaussian, double* d_B, size_t ldb, hipStream_t stream) {
    if (n_dst <= 0) return hipSuccess;
    hipLaunchKernelGGL(ok_cov_kernel, dim3(unsigned((n_dst + 255) / 256), unsigned((n_src + 1 + OK_COV_JB - 1) / OK_COV_JB)),
                       dim3(256), 0, stream, d_src_xyz, n_src, d_dst_xyz, n_dst, c, k, z_scale, gaussian, d_B, ldb);
    return hipGetLastError();
}

int ok_product_ldl(int rows) { return (rows + OK_RT - 1) / OK_RT * OK_RT; }

hipError_t launch_ok_product(const double* d_Lt, int ldl, int rows, const double* d_R, size_t ldr, int K, int m,
                             double* d_C, size_t ldc, hipStream_t stream) {
    if (rows <= 0 || m <= 0) return hipSuccess;
    if (ldl < ok_product_ldl(rows)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ok_product_kernel, dim3(unsigned((m + 63) / 64), unsigned((rows + OK_RT * OK_NW - 1) / (OK_RT * OK_NW))),
                       dim3(64 * OK_NW), 0, stream, d_Lt, ldl, rows, d_R, ldr, K, m, d_C, ldc);
    return hipGetLastError();
}

// measured: 16384 is as fast as any larger block and keeps the scratch for 500 sources at 131 MB
size_t ok_default_dst_block() { return size_t(1) << 14; }

void ok_run(const ok_args& a, hipStream_t stream) {
    const size_t n = a.n_sources, N = n + 1, m = a.n_dst, T = a.n_steps;
    if (m == 0 || T == 0) return;
    check_limits(a);
    const std::vector<double> Ainv = ok_system_inverse(a);
    // both left factors k-major with the row count padded to the row tile: Ainv[0:n]' is N x ldw, obs' is n x ldo
    const size_t ldw = size_t(ok_product_ldl(int(n)));
    std::vector<double> left(N * ldw, 0.0);
    for (size_t s = 0; s < n; ++s)
        for (size_t j = 0; j < N; ++j) left[j * ldw + s] = Ainv[s * N + j];
    const size_t step_block = 4096;  // steps per values pass: bounds obs' and the grid's y
    const size_t ldo = size_t(ok_product_ldl(int(std::min(T, step_block))));
    // a pass stays below 2^30 destinations: the kernels index them with int
    const size_t blk = std::min({m, a.dst_block ? a.dst_block : ok_default_dst_block(), size_t(1) << 30});

    // every count below is > 0: n >= 2 (check_limits), ldw and ldo >= OK_RT, 1 <= blk <= m
    dbuf<double> d_src, d_left, d_obs, d_BW;
    d_src.alloc(3 * n);
    d_left.alloc(left.size());
    d_obs.alloc(n * ldo);
    d_BW.alloc((2 * n + 1) * blk);  // B (N rows) then W (n rows): within 2 (n+1) dst_block doubles
    double* d_B = d_BW.p;
    double* d_W = d_BW.p + N * blk;
    const char* up = "ordinary kriging upload";
    hip_check(hipMemcpyAsync(d_src.p, a.src_xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, stream), up);
    hip_check(hipMemcpyAsync(d_left.p, left.data(), left.size() * sizeof(double), hipMemcpyHostToDevice, stream), up);
    std::vector<double> obs(n * ldo);
    for (size_t t0 = 0; t0 < T; t0 += step_block) {
        const size_t tb = std::min(step_block, T - t0);
        std::fill(obs.begin(), obs.end(), 0.0);
        for (size_t t = 0; t < tb; ++t)
            for (size_t s = 0; s < n; ++s) obs[s * ldo + t] = a.src_values[(t0 + t) * n + s];
        hip_check(hipMemcpyAsync(d_obs.p, obs.data(), obs.size() * sizeof(double), hipMemcpyHostToDevice, stream), up);
        for (size_t d0 = 0; d0 < m; d0 += blk) {
            const size_t mb = std::min(blk, m - d0);
            hip_check(launch_ok_cov(d_src.p, int(n), a.d_dst_xyz + 3 * d0, int(mb), a.c, ok_k(a), a.z_scale,
                                    a.cov_type == 0, d_B, mb, stream),
                      "ordinary kriging covariance kernel");
            hip_check(launch_ok_product(d_left.p, int(ldw), int(n), d_B, mb, int(N), int(mb), d_W, mb, stream),
                      "ordinary kriging weights kernel");
            hip_check(launch_ok_product(d_obs.p, int(ldo), int(tb), d_W, mb, int(n), int(mb),
                                        a.d_out + t0 * a.ld_out + d0, a.ld_out, stream),
                      "ordinary kriging values kernel");
        }
        hip_check(hipStreamSynchronize(stream), "ordinary kriging sync");  // obs is refilled for the next block of steps
    }
}

void ok_host_run(const ok_args& a, double* out) {
    const size_t n = a.n_sources, N = n + 1, m = a.n_dst, T = a.n_steps;
    if (m == 0 || T == 0) return;
    check_limits(a);
    const std::vector<double> Ainv = ok_system_inverse(a);
    const double k = ok_k(a);
    const bool gaussian = a.cov_type == 0;
    std::vector<double> B(N), W(n);
    for (size_t d = 0; d < m; ++d) {
        const double* q = a.dst_xyz + 3 * d;
        for (size_t j = 0; j < n; ++j) {
            const double* p = a.src_xyz + 3 * j;
            B[j] = ok_cov(p[0], p[1], p[2], q[0], q[1], q[2], a.c, k, a.z_scale, gaussian);
        }
        B[n] = 1.0;
        for (size_t s = 0; s < n; ++s) {
            double acc = 0.0;
            for (size_t j = 0; j < N; ++j) acc = __builtin_fma(Ainv[s * N + j], B[j], acc);
            W[s] = acc;
        }
        for (size_t t = 0; t < T; ++t) {
            double acc = 0.0;
            for (size_t s = 0; s < n; ++s) acc = __builtin_fma(a.src_values[t * n + s], W[s], acc);
            out[t * m + d] = acc;
        }
    }
}
