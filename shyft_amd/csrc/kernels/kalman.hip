// Batched Kalman bias filter for gfx950 (core/kalman.h:24-236).
//
// M independent filters of size n (n = n_daily_observations, 1..32) share one time axis and one parameter set;
// one launch runs all T steps, the time loop inside the kernel. Structure-of-arrays, point fastest:
// bias [T][M], x [n][M], k [n][M], P [n*n][M] (row-major i*n+j), out [T][M].
//
// Lane mapping: G lanes per point, G the power of two >= n, so a group never straddles a wave. Lane r of a group
// holds row r of P padded to G columns, x[r], k[r] and row r of W. One step (filter::update, kalman.h:127-145):
//   P = P + W;  tmp = P[ix][ix] + v2;  k[i] = P[i][ix] / tmp;  P[i][j] = P[i][j] - (P[i][ix] * P[ix][j]) / tmp;
//   x[i] = x[i] + k[i] * (b - x[ix])
// all from the pre-update values, every division a division, no FMA contraction (the file is built with
// -ffp-contract=off). ix = fold[t] is wave-uniform, so the own-row element P[r][ix] is a chain of selects and row
// ix, P[ix][ix] and x[ix] are group broadcasts (__shfl(v, ix, G)). Every shuffle sits in wave-uniform control
// flow: finiteness of the bias is per point, so lanes shuffle first and predicate the arithmetic afterwards, and
// lanes of padded rows or of points past M stay in the wave until the loop ends. Padded entries start as +0.0
// and are never written. kalman_host_run is the same arithmetic in plain C++; the kernel is bit-identical to it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../detmath/detmath.h"
#include "../include_internal/device_call.h"

using namespace shyft_hip_impl;

namespace {

constexpr int KALMAN_MAX_N = 32;
constexpr int KALMAN_BLOCK = 256;

__host__ __device__ inline bool kalman_finite(double v) {
    union {
        double d;
        uint64_t u;
    } c;
    c.d = v;
    return (c.u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// state::make_covariance's folded distance (kalman.h:45)
__host__ __device__ inline int kalman_fold_dist(int i, int j, int n) {
    const int d = i > j ? i - j : j - i;
    return d < n - d ? d : n - d;
}

struct kalman_dev_args {
    int n;
    size_t M;
    int T;
    const double* bias;
    const int* fold;
    const double* w;
    double v2;
    int predictor;  // 0 filter mode, 1 predictor mode
    double* x;
    double* k;
    double* P;
    double* out;  // null: no running bias
    int save_every;
    const int* piece_begin;
    const int* piece_ix;
    const double* piece_seconds;
};

template <int G>
__global__ __launch_bounds__(KALMAN_BLOCK) void kalman_run_k(
    const int n, const size_t M, const int T, const double* __restrict__ bias, const int* __restrict__ fold,
    const double* __restrict__ w, const double v2, const int predictor, double* __restrict__ xs, double* __restrict__ ks,
    double* __restrict__ Ps, double* __restrict__ out, const int save_every, const int* __restrict__ piece_begin,
    const int* __restrict__ piece_ix, const double* __restrict__ piece_seconds) {
    const size_t gid = size_t(blockIdx.x) * KALMAN_BLOCK + threadIdx.x;
    const size_t point = gid / G;
    const int r = int(gid % G);
    const bool valid = point < M && r < n;
    const size_t pt = point < M ? point : 0;  // a safe address for the lanes that only keep the wave whole

    double P[G], W[G];
    // The column count of this lane lives in a vector register the compiler cannot see through (one copy per
    // use): as a scalar, or as one shared value, hipcc keeps the G masks j < n in SGPR pairs from the loads over
    // the step loop to the stores and spills SGPRs at G = 32. Loads are unconditional, from element 0 where the
    // lane has no such column.
    const int nv = valid ? n : 0;
    int nl = nv;
    asm volatile("" : "+v"(nl));
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const bool in = j < nl;
        const double p = Ps[in ? (size_t(r) * n + j) * M + pt : 0];
        const double q = w[in ? kalman_fold_dist(r, j, n) : 0];
        P[j] = in ? p : 0.0;
        W[j] = in ? q : 0.0;
    }
    double x = valid ? xs[size_t(r) * M + pt] : 0.0;
    double k = valid ? ks[size_t(r) * M + pt] : 0.0;
    double snap = 0.0;
    const double nan = __builtin_nan("");

    for (int t = 0; t < T; ++t) {
        if (out) {  // wave-uniform: compute_running_bias's profile (kalman.h:215-225), before this step's update
            if (t % save_every == 0) snap = x;
            const int p0 = __builtin_amdgcn_readfirstlane(piece_begin[t]), p1 = __builtin_amdgcn_readfirstlane(piece_begin[t + 1]);
            double area = 0.0, tsum = 0.0;
            for (int p = p0; p < p1; ++p) {
                const double v = __shfl(snap, __builtin_amdgcn_readfirstlane(piece_ix[p]), G);
                const double s = piece_seconds[p];
                if (kalman_finite(v)) {
                    area += v * s;
                    tsum += s;
                }
            }
            if (r == 0 && point < M) out[size_t(t) * M + point] = tsum > 0.0 ? area / tsum : nan;
        }
        const int ix = __builtin_amdgcn_readfirstlane(fold[t]);
        const double b = point < M ? bias[size_t(t) * M + pt] : nan;
        const bool fin = kalman_finite(b);
        const bool grow = fin || !predictor;  // filter mode grows P on a missing bias, predictor mode skips the step
        double own = 0.0;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            P[j] = grow ? P[j] + W[j] : P[j];
            own = j == ix ? P[j] : own;
        }
        const double tmp = __shfl(own, ix, G) + v2;
        const double xix = __shfl(x, ix, G);
        const bool upd = fin && valid;
        int cols = fin ? nv : 0;
        asm volatile("" : "+v"(cols));
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const double rj = __shfl(P[j], ix, G);
            const double pn = P[j] - (own * rj) / tmp;
            P[j] = j < cols ? pn : P[j];
        }
        const double kn = own / tmp;
        const double xn = x + kn * (b - xix);
        k = upd ? kn : k;
        x = upd ? xn : x;
    }

    int ns = nv;
    asm volatile("" : "+v"(ns));
#pragma unroll
    for (int j = 0; j < G; ++j)
        if (j < ns) Ps[(size_t(r) * n + j) * M + point] = P[j];
    if (valid) {
        xs[size_t(r) * M + point] = x;
        ks[size_t(r) * M + point] = k;
    }
}

template <int G>
hipError_t launch_g(const kalman_dev_args& a, hipStream_t s) {
    const size_t threads = a.M * size_t(G);
    const size_t blocks = (threads + KALMAN_BLOCK - 1) / KALMAN_BLOCK;
    hipLaunchKernelGGL(kalman_run_k<G>, dim3((unsigned)blocks), dim3(KALMAN_BLOCK), 0, s, a.n, a.M, a.T, a.bias, a.fold, a.w,
                       a.v2, a.predictor, a.x, a.k, a.P, a.out, a.save_every, a.piece_begin, a.piece_ix, a.piece_seconds);
    return hipGetLastError();
}

hipError_t launch_kalman(const kalman_dev_args& a, hipStream_t s) {
    if (a.n <= 1) return launch_g<1>(a, s);
    if (a.n <= 2) return launch_g<2>(a, s);
    if (a.n <= 4) return launch_g<4>(a, s);
    if (a.n <= 8) return launch_g<8>(a, s);
    if (a.n <= 16) return launch_g<16>(a, s);
    return launch_g<32>(a, s);
}

// the host restatement: one point at a time, the same expressions in the same order
void kalman_host_run(const kalman_dev_args& a) {
    const int n = a.n;
    const size_t M = a.M;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> P(size_t(n) * n), W(size_t(n) * n), Pn(size_t(n) * n), x(n), k(n), snap(n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) W[size_t(i) * n + j] = a.w[kalman_fold_dist(i, j, n)];
    for (size_t m = 0; m < M; ++m) {
        for (int i = 0; i < n * n; ++i) P[i] = a.P[size_t(i) * M + m];
        for (int i = 0; i < n; ++i) {
            x[i] = a.x[size_t(i) * M + m];
            k[i] = a.k[size_t(i) * M + m];
        }
        for (int t = 0; t < a.T; ++t) {
            if (a.out) {
                if (t % a.save_every == 0) snap = x;
                double area = 0.0, tsum = 0.0;
                for (int p = a.piece_begin[t]; p < a.piece_begin[t + 1]; ++p) {
                    const double v = snap[a.piece_ix[p]];
                    const double s = a.piece_seconds[p];
                    if (kalman_finite(v)) {
                        area += v * s;
                        tsum += s;
                    }
                }
                a.out[size_t(t) * M + m] = tsum > 0.0 ? area / tsum : nan;
            }
            const int ix = a.fold[t];
            const double b = a.bias[size_t(t) * M + m];
            const bool fin = kalman_finite(b);
            if (fin || !a.predictor)
                for (int i = 0; i < n * n; ++i) P[i] = P[i] + W[i];
            if (!fin) continue;
            const double tmp = P[size_t(ix) * n + ix] + a.v2;
            const double xix = x[ix];
            for (int i = 0; i < n; ++i) {
                const double own = P[size_t(i) * n + ix];
                for (int j = 0; j < n; ++j) Pn[size_t(i) * n + j] = P[size_t(i) * n + j] - (own * P[size_t(ix) * n + j]) / tmp;
                k[i] = own / tmp;
                x[i] = x[i] + k[i] * (b - xix);
            }
            P.swap(Pn);
        }
        for (int i = 0; i < n * n; ++i) a.P[size_t(i) * M + m] = P[i];
        for (int i = 0; i < n; ++i) {
            a.x[size_t(i) * M + m] = x[i];
            a.k[size_t(i) * M + m] = k[i];
        }
    }
}

// argument checks shared by the device and the host entry; true when there is nothing to do
bool kalman_prepare(const char* who, int n, size_t M, size_t T, const double* bias, const int32_t* fold, const double* w,
                    int mode, const double* x, const double* k, const double* P, const double* out, int save_every,
                    const int32_t* piece_begin, const int32_t* piece_ix, const double* piece_seconds, bool device) {
    if (device && (n < 1 || n > KALMAN_MAX_N))
        throw std::runtime_error("kalman: n_daily_observations must be in 1..32 on the device");
    if (n < 1) throw std::runtime_error("kalman: n_daily_observations must be at least 1");
    if (mode != 0 && mode != 1) throw std::runtime_error("kalman: mode must be 0 (filter) or 1 (predictor)");
    if (M == 0 || T == 0) return true;
    const size_t max_elements = std::numeric_limits<size_t>::max() / sizeof(double);
    if (M > max_elements / T || M > max_elements / (size_t(n) * size_t(n)))
        throw std::runtime_error("kalman: the batch is too large, T x M or n x n x M bytes overflow");
    if (!bias || !fold || !w || !x || !k || !P) throw std::runtime_error(std::string(who) + ": null argument");
    if (T > size_t(std::numeric_limits<int>::max()) - 1) throw std::runtime_error("kalman: too many steps");
    for (size_t t = 0; t < T; ++t)
        if (fold[t] < 0 || fold[t] >= n) throw std::runtime_error("kalman: fold index outside 0..n-1");
    if (out) {
        if (mode != 1) throw std::runtime_error("kalman: the running bias needs predictor mode");
        if (save_every < 1) throw std::runtime_error("kalman: save_every must be at least 1");
        if (!piece_begin || !piece_ix || !piece_seconds) throw std::runtime_error(std::string(who) + ": null argument");
        if (piece_begin[0] != 0) throw std::runtime_error("kalman: piece_begin must start at 0");
        for (size_t t = 0; t < T; ++t)
            if (piece_begin[t + 1] < piece_begin[t]) throw std::runtime_error("kalman: piece_begin must not decrease");
        for (int p = 0; p < piece_begin[T]; ++p)
            if (piece_ix[p] < 0 || piece_ix[p] >= n) throw std::runtime_error("kalman: piece index outside 0..n-1");
    }
    return false;
}

call_record g_kalman;
constexpr const char* KALMAN_UPLOAD = "kalman upload";
constexpr const char* KALMAN_DOWNLOAD = "kalman download";

}  // namespace

extern "C" {

int shyft_hip_kalman_run(int device, int n, size_t M, size_t T, const double* bias, const int32_t* fold, const double* w,
                         double v2, int mode, double* x, double* k, double* P, double* out, int save_every,
                         const int32_t* piece_begin, const int32_t* piece_ix, const double* piece_seconds) {
    try {
        if (kalman_prepare("shyft_hip_kalman_run", n, M, T, bias, fold, w, mode, x, k, P, out, save_every, piece_begin,
                           piece_ix, piece_seconds, true))
            return 0;
        if (M * size_t(KALMAN_MAX_N) / KALMAN_BLOCK + 1 > size_t(std::numeric_limits<int>::max()))
            throw std::runtime_error("kalman: too many points for one launch");
        device_call c(device);
        const size_t nn = size_t(n) * n;
        dbuf<double> d_bias, d_w, d_x, d_k, d_P, d_out, d_sec;
        dbuf<int32_t> d_fold, d_pb, d_pi;
        c.upload(d_bias, bias, T * M, KALMAN_UPLOAD);
        c.upload(d_fold, fold, T, KALMAN_UPLOAD);
        c.upload(d_w, w, size_t(n / 2 + 1), KALMAN_UPLOAD);
        c.upload(d_x, x, size_t(n) * M, KALMAN_UPLOAD);
        c.upload(d_k, k, size_t(n) * M, KALMAN_UPLOAD);
        c.upload(d_P, P, nn * M, KALMAN_UPLOAD);
        kalman_dev_args a{};
        a.n = n;
        a.M = M;
        a.T = int(T);
        a.bias = d_bias.p;
        a.fold = d_fold.p;
        a.w = d_w.p;
        a.v2 = v2;
        a.predictor = mode;
        a.x = d_x.p;
        a.k = d_k.p;
        a.P = d_P.p;
        a.save_every = 1;
        if (out) {
            const size_t np = size_t(piece_begin[T]);
            d_out.alloc(T * M);
            c.upload(d_pb, piece_begin, T + 1, KALMAN_UPLOAD);
            c.upload(d_pi, piece_ix, np, KALMAN_UPLOAD);
            c.upload(d_sec, piece_seconds, np, KALMAN_UPLOAD);
            a.out = d_out.p;
            a.save_every = save_every;
            a.piece_begin = d_pb.p;
            a.piece_ix = d_pi.p;
            a.piece_seconds = d_sec.p;
        }
        c.begin();
        hip_check(launch_kalman(a, c.s), "kalman_run");
        c.end();
        c.download(x, d_x.p, size_t(n) * M, KALMAN_DOWNLOAD);
        c.download(k, d_k.p, size_t(n) * M, KALMAN_DOWNLOAD);
        c.download(P, d_P.p, nn * M, KALMAN_DOWNLOAD);
        if (out) c.download(out, d_out.p, T * M, KALMAN_DOWNLOAD);
        g_kalman.record(c.dev, c.finish("kalman_run"));
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_kalman_run_host(int n, size_t M, size_t T, const double* bias, const int32_t* fold, const double* w, double v2,
                              int mode, double* x, double* k, double* P, double* out, int save_every,
                              const int32_t* piece_begin, const int32_t* piece_ix, const double* piece_seconds) {
    try {
        if (kalman_prepare("shyft_hip_kalman_run_host", n, M, T, bias, fold, w, mode, x, k, P, out, save_every,
                           piece_begin, piece_ix, piece_seconds, false))
            return 0;
        kalman_dev_args a{};
        a.n = n;
        a.M = M;
        a.T = int(T);
        a.bias = bias;
        a.fold = fold;
        a.w = w;
        a.v2 = v2;
        a.predictor = mode;
        a.x = x;
        a.k = k;
        a.P = P;
        a.out = out;
        a.save_every = out ? save_every : 1;
        a.piece_begin = piece_begin;
        a.piece_ix = piece_ix;
        a.piece_seconds = piece_seconds;
        kalman_host_run(a);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_kalman_initial_state(int n, double covariance_init, double hourly_correlation, double process_noise_init,
                                   double* P, double* W) {
    if (n < 0 || (n > 0 && (!P || !W))) return fail(nullptr, "shyft_hip_kalman_initial_state: bad argument");
    const double dt_hours = 24.0 / n;
    const double cw = process_noise_init * process_noise_init;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double c = detmath::pow(hourly_correlation, kalman_fold_dist(i, j, n) * dt_hours);
            P[size_t(i) * n + j] = covariance_init * c;
            W[size_t(i) * n + j] = cw * c;
        }
    return 0;
}

double shyft_hip_kalman_last_ms(int device) { return g_kalman.last_ms.load(device, 0.0); }

}  // extern "C"
