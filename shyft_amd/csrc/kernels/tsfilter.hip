// The point-wise filter series of a batch of S point series for gfx950: convolve_w, derivative, inside and decode
// (core/time_series.h:895-980; core/time_series_dd.h:583-607, 1538-1700; core/time_series_dd.cpp:311-463, 942-948,
// 1409-1445). host/ts_filter.hpp holds the same statements in plain C++ and is the definition of correct; the _host
// entries run those, not this file's.
//
// The series come in the CSR form of shyft_hip_resample: row [S+1] point offsets, t and v [row[S]] point times (int64
// microseconds) and values, t_end [S], fx [S]. An output is one double per input point in the same CSR order. Every
// operation is evaluated as written: int64 tick arithmetic, to_seconds(x) = double(x) / 1e6 as a division, no FMA
// (-ffp-contract=off), isfinite by the exponent bits. No atomics, no inline assembly, and no workgroup ever waits for
// another one.
//
//  DERIVATIVE, INSIDE, DECODE  one lane per point of the flat array, grid-stride; the lane finds its series by
//           csr_series_of and reads the per-series parameters. DERIVATIVE reads the neighbours v[k-1], v[k+1] and the
//           times t[k-1] .. t[k+2] from global memory, each only after the test that keeps it inside the lane's own
//           series; the period end of the series' last point is t_end[s].
//  CONVOLVE_W  out[i] = sum over j = 0 .. K-1, in that order, of w[j] * x[i-j], with the policy's stand-in where
//           i - j < 0. Each lane owns one output point and ONE accumulator, and adds the taps in ascending j with a
//           multiply and then an add. That order is the host's, so the sum is bit-identical to it; partial
//           accumulators, a tree or a fused multiply-add would each round differently.
//    DIRECT one lane per flat point, grid-stride, taps and values from global memory.
//    TILED  one workgroup of TF_BLOCK lanes per tile of TF_TILE consecutive points of one series (tile table built on
//           the host: series, first point). The taps go in chunks of TF_CHUNK: for taps [j0, j0 + C) the workgroup
//           stages the window x[i0 - j0 - C + 1 .. i0 + TILE - 1 - j0] (TILE + C - 1 doubles) and the chunk's weights
//           into LDS. Lane l, tap j0 + jj reads window slot l - jj + C - 1: neighbouring lanes read neighbouring
//           doubles, and the weight is one address for the whole workgroup (a broadcast read).
//
// Index safety. The host checks before any launch that row[0] == 0 and row is non-decreasing, so row[S] = np points
// were uploaded; that w_row is a CSR of the uploaded weights and w_of[s] < W; that every tile (s, i0) has s < S and
// 0 <= i0 < n_s. A pointwise lane's k is < np by its grid-stride test and csr_series_of gives the s with
// row[s] <= k < row[s+1]. DERIVATIVE reads k - 1 only with k > row[s], k + 1 only with k + 1 < row[s+1], and k + 2
// only with k + 2 < row[s+1]. CONVOLVE_W reads x[r0 + i - j] only with 0 <= i - j and i < n, so never below the series'
// first point r0 = row[s] (the previous series) nor at or above row[s+1]; x[r0] only with n > 0. The TILED window is
// filled only from series indexes in [0, n), any other slot is set to 0.0 and never used by a valid lane; window slots
// are l - jj + C - 1 with 0 <= l < TILE and 0 <= jj < C, inside [0, TILE + C - 1). Stores go to out[r0 + i], i < n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/shyft_hip.h"
#include "../device/csr_series.h"
#include "../device/ts_area.h"
#include "../host/ts_filter.hpp"
#include "../include_internal/device_call.h"
#include "../include_internal/series_args.h"

using namespace shyft_hip_impl;

namespace {

constexpr int TF_BLOCK = 256;                    // 4 wavefronts
constexpr int TF_TILE = 256;                     // output points per workgroup of the tiled convolution
constexpr int TF_CHUNK = 256;                    // taps per staged window
constexpr int TF_WINDOW = TF_TILE + TF_CHUNK - 1;
constexpr size_t TF_MAX_K = 65536;               // the device entry's cap on the weights of one profile
// AUTO takes TILED from this many weights on, when the tiles are at least a quarter full on average. Measured once
// (DESIGN.md 3.14): TILED was faster from 2 weights on for long series and at 64-point series, DIRECT at 16-point ones.
constexpr size_t TF_AUTO_MIN_K = 2;
static_assert(TF_TILE == TF_BLOCK, "one lane per point of a tile");

// ---- derivative --------------------------------------------------------------------------------------------------------
struct tf_deriv_args {
    int64_t np, S;
    const int64_t* row;
    const int64_t* t;
    const double* v;
    const int64_t* t_end;
    const int32_t* fx;
    const int64_t* fixed_dt;
    const int32_t* method;
    double* out;
};

// derivative_fx_value of host/ts_filter.hpp for the flat point k of the series [r0, r1), n = r1 - r0 >= 2
__device__ inline double tf_derivative_fx(const tf_deriv_args& a, int64_t s, int64_t r0, int64_t r1, int64_t k) {
    const double nan = rs_nan();
    const int64_t dt = a.fixed_dt[s];
    const int32_t dm = a.method[s];
    const bool first = k == r0, last = k + 1 == r1;
    const double v1 = a.v[k];
    const bool f1 = rs_finite(v1);
    if (dt > 0) {
        if (dm == 0 || dm == 3) {
            if (first) {
                const double v2 = a.v[k + 1];
                return f1 ? (rs_finite(v2) ? (v2 - v1) / rs_seconds(2 * dt) : 0.0) : nan;
            }
            const double v0 = a.v[k - 1];
            if (last) return f1 ? (rs_finite(v0) ? (v1 - v0) / rs_seconds(2 * dt) : 0.0) : nan;
            if (!f1) return nan;
            const double v2 = a.v[k + 1];
            if (rs_finite(v0)) {
                if (rs_finite(v2)) return (v2 - v0) / rs_seconds(2 * dt);
                return (v1 - v0) / rs_seconds(2 * dt);
            }
            if (rs_finite(v2)) return (v2 - v1) / rs_seconds(2 * dt);
            return 0.0;
        }
        if (dm == 1) {
            if (last) return f1 ? 0.0 : nan;
            const double v2 = a.v[k + 1];
            return f1 ? (rs_finite(v2) ? (v2 - v1) / rs_seconds(dt) : 0.0) : nan;
        }
        if (first) return f1 ? 0.0 : nan;
        const double v0 = a.v[k - 1];
        return f1 ? (rs_finite(v0) ? (v1 - v0) / rs_seconds(dt) : 0.0) : nan;
    }
    // variable intervals; the end of period j is t[j + 1], t_end[s] for the series' last point
    const int64_t te = a.t_end[s];
    const int64_t tk = a.t[k];
    const int64_t pe1 = last ? te : a.t[k + 1];  // the end of period k
    if (dm == 0 || dm == 3) {
        if (first) {
            const double v2 = a.v[k + 1];
            const int64_t pe2 = k + 2 < r1 ? a.t[k + 2] : te;  // the end of period k + 1
            return f1 ? (rs_finite(v2) ? (v2 - v1) / rs_seconds(pe2 - tk) : 0.0) : nan;
        }
        const double v0 = a.v[k - 1];
        const int64_t t0 = a.t[k - 1];
        if (last) {
            if (f1) {
                if (rs_finite(v0)) return (v1 - v0) / rs_seconds(te - t0);
                return 0.0;
            }
            return nan;
        }
        if (!f1) return nan;
        const double v2 = a.v[k + 1];
        const int64_t t2 = a.t[k + 1];
        const int64_t pe2 = k + 2 < r1 ? a.t[k + 2] : te;
        if (rs_finite(v0)) {
            if (rs_finite(v2)) return 2 * (v2 - v0) / rs_seconds((t2 - t0) + (pe2 - tk));  // the end of period k - 1 is t[k]
            return (v1 - v0) / rs_seconds(pe1 - t0);
        } else if (rs_finite(v2)) {
            return (v2 - v1) / rs_seconds(pe2 - tk);
        }
        return 0.0;
    }
    if (dm == 1) {
        if (last) return f1 ? 0.0 : nan;
        if (!f1) return nan;
        const double v2 = a.v[k + 1];
        if (!rs_finite(v2)) return 0.0;
        const int64_t t2 = a.t[k + 1];
        const int64_t pe2 = k + 2 < r1 ? a.t[k + 2] : te;
        return 2 * (v2 - v1) / rs_seconds((t2 - tk) + (pe2 - pe1));
    }
    if (first) return f1 ? 0.0 : nan;
    if (!f1) return nan;
    const double v0 = a.v[k - 1];
    if (!rs_finite(v0)) return 0.0;
    const int64_t t0 = a.t[k - 1];
    return 2 * (v1 - v0) / rs_seconds((tk - t0) + (pe1 - tk));  // the end of period k - 1 is t[k]
}

__global__ __launch_bounds__(TF_BLOCK) void tf_derivative_kernel(tf_deriv_args a) {
    const int64_t stride = int64_t(gridDim.x) * TF_BLOCK;
    for (int64_t k = int64_t(blockIdx.x) * TF_BLOCK + threadIdx.x; k < a.np; k += stride) {
        const int64_t s = csr_series_of(a.row, a.S, k);
        const int64_t r0 = a.row[s], r1 = a.row[s + 1];
        double r;
        if (a.fx[s] == int32_t(shyft_hip::host::POINT_INSTANT_VALUE)) {
            if (k + 1 < r1) r = (a.v[k + 1] - a.v[k]) / rs_seconds(a.t[k + 1] - a.t[k]);
            else r = rs_nan();
        } else if (r1 - r0 < 2) {
            r = rs_finite(a.v[k]) ? 0.0 : rs_nan();
        } else {
            r = tf_derivative_fx(a, s, r0, r1, k);
        }
        a.out[k] = r;
    }
}

// ---- inside and decode -------------------------------------------------------------------------------------------------
struct tf_inside_args {
    int64_t np, S;
    const int64_t* row;
    const double* v;
    const double* min_x;
    const double* max_x;
    const double* nan_x;
    const double* x_inside;
    const double* x_outside;
    double* out;
};

__global__ __launch_bounds__(TF_BLOCK) void tf_inside_kernel(tf_inside_args a) {
    const int64_t stride = int64_t(gridDim.x) * TF_BLOCK;
    for (int64_t k = int64_t(blockIdx.x) * TF_BLOCK + threadIdx.x; k < a.np; k += stride) {
        const int64_t s = csr_series_of(a.row, a.S, k);
        const double x = a.v[k];
        const double min_x = a.min_x[s], max_x = a.max_x[s];
        double r;
        if (!rs_finite(x)) r = a.nan_x[s];
        else if (rs_finite(min_x) && x < min_x) r = a.x_outside[s];
        else if (rs_finite(max_x) && x >= max_x) r = a.x_outside[s];
        else r = a.x_inside[s];
        a.out[k] = r;
    }
}

struct tf_decode_args {
    int64_t np, S;
    const int64_t* row;
    const double* v;
    const int32_t* start_bit;
    const int32_t* n_bits;
    double* out;
};

__global__ __launch_bounds__(TF_BLOCK) void tf_decode_kernel(tf_decode_args a) {
    const int64_t stride = int64_t(gridDim.x) * TF_BLOCK;
    for (int64_t k = int64_t(blockIdx.x) * TF_BLOCK + threadIdx.x; k < a.np; k += stride) {
        const int64_t s = csr_series_of(a.row, a.S, k);
        const double x = a.v[k];
        double r = rs_nan();
        if (rs_finite(x) && !(x < 0) && !(x > double(uint64_t(1) << 52))) {
            // 1 <= n_bits <= 51 (checked on the host): the mask of bitmask<uint64_t>(n_bits)
            const uint64_t mask = ~uint64_t(0) >> (64 - unsigned(a.n_bits[s]));
            r = double((uint64_t(x) >> unsigned(a.start_bit[s])) & mask);
        }
        a.out[k] = r;
    }
}

// ---- convolve_w --------------------------------------------------------------------------------------------------------
struct tf_conv_args {
    int64_t np, S, ntiles;
    const int64_t* row;
    const double* v;
    const int64_t* w_row;
    const double* w;
    const int64_t* w_of;
    const int32_t* policy;
    const int64_t* tile_s;   // [ntiles] the series of a tile (TILED)
    const int64_t* tile_i0;  // [ntiles] its first point inside the series (TILED)
    double* out;
};

// the stand-in term of tap j > i (time_series.h:972-973)
__device__ inline double tf_before_first(int32_t policy, double wj, double x0) {
    return policy == int32_t(shyft_hip::host::USE_FIRST) ? wj * x0
                                                          : (policy == int32_t(shyft_hip::host::USE_ZERO) ? 0.0 : rs_nan());
}

__global__ __launch_bounds__(TF_BLOCK) void tf_convolve_direct_kernel(tf_conv_args a) {
    const int64_t stride = int64_t(gridDim.x) * TF_BLOCK;
    for (int64_t k = int64_t(blockIdx.x) * TF_BLOCK + threadIdx.x; k < a.np; k += stride) {
        const int64_t s = csr_series_of(a.row, a.S, k);
        const int64_t r0 = a.row[s];
        const int64_t i = k - r0;
        const int64_t wb = a.w_row[a.w_of[s]], K = a.w_row[a.w_of[s] + 1] - wb;
        const int32_t policy = a.policy[s];
        const double x0 = a.v[r0];
        const double* __restrict__ w = a.w + wb;
        const int64_t inside = K < i + 1 ? K : i + 1;  // the taps j <= i
        double acc = 0.0;
        for (int64_t j = 0; j < inside; ++j) acc += w[j] * a.v[k - j];
        for (int64_t j = inside; j < K; ++j) acc += tf_before_first(policy, w[j], x0);
        a.out[k] = acc;
    }
}

__global__ __launch_bounds__(TF_BLOCK) void tf_convolve_tiled_kernel(tf_conv_args a) {
    __shared__ double xs[TF_WINDOW];
    __shared__ double ws[TF_CHUNK];
    const int l = int(threadIdx.x);
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {  // uniform over the workgroup
        const int64_t s = a.tile_s[tile], i0 = a.tile_i0[tile];
        const int64_t r0 = a.row[s], n = a.row[s + 1] - r0;
        const int64_t wb = a.w_row[a.w_of[s]], K = a.w_row[a.w_of[s] + 1] - wb;
        const int32_t policy = a.policy[s];
        const double x0 = a.v[r0];  // n > 0: the tile has a point
        const int64_t i = i0 + l;
        const bool valid = i < n;
        double acc = 0.0;
        for (int64_t j0 = 0; j0 < K; j0 += TF_CHUNK) {  // uniform
            const int cnt = int(K - j0 < TF_CHUNK ? K - j0 : TF_CHUNK);
            const int64_t lo = i0 - j0 - (TF_CHUNK - 1);  // the series index of window slot 0
            __syncthreads();                              // the previous chunk (or tile) has been read
            for (int m = l; m < TF_WINDOW; m += TF_BLOCK) {
                const int64_t g = lo + m;
                xs[m] = (g >= 0 && g < n) ? a.v[r0 + g] : 0.0;
            }
            if (l < cnt) ws[l] = a.w[wb + j0 + l];
            __syncthreads();
            if (valid) {
                const double* __restrict__ x = xs + l + (TF_CHUNK - 1);  // x[-jj] is series index i - j0 - jj
                // the taps of this chunk with j <= i; for every tile past the start of its series that is all of them
                const int64_t left = i - j0 + 1;
                const int inside = left <= 0 ? 0 : (left < cnt ? int(left) : cnt);
#pragma unroll 4
                for (int jj = 0; jj < inside; ++jj) acc += ws[jj] * x[-jj];
                for (int jj = inside; jj < cnt; ++jj) acc += tf_before_first(policy, ws[jj], x0);
            }
        }
        if (valid) a.out[r0 + i] = acc;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// The argument checks of the series, shared by the device and the host entries (include_internal/series_args.h); true
// when there is nothing to do.
bool tf_prepare(const char* who, size_t S, const int64_t* row, const int64_t* t, const double* v, const int64_t* t_end,
                const int32_t* fx, const double* out) {
    if (S == 0) return true;
    check_point_series(who, "ts_filter", S, row, t, v, t_end, fx);
    if (row[S] == 0) return true;
    if (!out) throw std::runtime_error(std::string(who) + ": null argument");
    return false;
}

void tf_prepare_convolve(const char* who, size_t S, size_t W, const int64_t* w_row, const double* w, const int64_t* w_of,
                         const int32_t* policy) {
    if (!w_row || !w_of || !policy) throw std::runtime_error(std::string(who) + ": null argument");
    if (w_row[0] != 0) throw std::runtime_error("convolve_w: w_row[0] must be 0");
    for (size_t p = 0; p < W; ++p)
        if (w_row[p + 1] < w_row[p]) throw std::runtime_error("convolve_w: w_row must not decrease");
    if (w_row[W] > 0 && !w) throw std::runtime_error(std::string(who) + ": null argument");
    for (size_t s = 0; s < S; ++s) {
        if (w_of[s] < 0 || size_t(w_of[s]) >= W) throw std::runtime_error("convolve_w: w_of is out of range");
        if (policy[s] < 0 || policy[s] > 2) throw std::runtime_error("convolve_w: policy must be USE_FIRST, USE_ZERO or USE_NAN");
    }
}

void tf_prepare_derivative(const char* who, size_t S, const int64_t* row, const int64_t* t, const int64_t* t_end,
                           const int64_t* fixed_dt, const int32_t* method) {
    if (!fixed_dt || !method) throw std::runtime_error(std::string(who) + ": null argument");
    for (size_t s = 0; s < S; ++s) {
        if (method[s] < 0 || method[s] > 3)
            throw std::runtime_error("derivative: method must be DEFAULT, FORWARD, BACKWARD or CENTER");
        if (fixed_dt[s] < 0) throw std::runtime_error("derivative: fixed_dt must not be negative");
        if (fixed_dt[s] == 0 || row[s] == row[s + 1]) continue;
        bool even = t_end[s] - t[row[s + 1] - 1] == fixed_dt[s];
        for (int64_t k = row[s] + 1; even && k < row[s + 1]; ++k) even = t[k] - t[k - 1] == fixed_dt[s];
        if (!even) throw std::runtime_error("derivative: fixed_dt is not the spacing of the series");
    }
}

void tf_prepare_decode(const char* who, size_t S, const int32_t* start_bit, const int32_t* n_bits) {
    if (!start_bit || !n_bits) throw std::runtime_error(std::string(who) + ": null argument");
    for (size_t s = 0; s < S; ++s) shyft_hip::host::check_decode_arguments(start_bit[s], n_bits[s]);
}

call_record g_tf;
std::atomic<int> g_tf_path{SHYFT_HIP_TSFILTER_PATH_AUTO};
constexpr const char* TF_UPLOAD = "tsfilter upload";

// one lane per job; the grid-stride loops take what the grid does not
unsigned tf_grid(size_t jobs) { return launch_blocks((jobs + TF_BLOCK - 1) / TF_BLOCK); }

}  // namespace

extern "C" {

int shyft_hip_ts_convolve_w(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                            const int64_t* t_end, const int32_t* fx, size_t W, const int64_t* w_row, const double* w,
                            const int64_t* w_of, const int32_t* policy, double* out) {
    try {
        if (tf_prepare("shyft_hip_ts_convolve_w", S, row, t, v, t_end, fx, out)) return 0;
        tf_prepare_convolve("shyft_hip_ts_convolve_w", S, W, w_row, w, w_of, policy);
        size_t k_max = 0;
        for (size_t s = 0; s < S; ++s) {
            if (row[s] == row[s + 1]) continue;
            const size_t K = size_t(w_row[w_of[s] + 1] - w_row[w_of[s]]);
            if (K > TF_MAX_K)
                throw std::runtime_error("convolve_w: more than 65536 weights in a profile are not supported on the device");
            k_max = K > k_max ? K : k_max;
        }
        const size_t np = size_t(row[S]);
        std::vector<int64_t> tile_s, tile_i0;  // one entry per TF_TILE points of a series
        for (size_t s = 0; s < S; ++s)
            for (int64_t i0 = 0; i0 < row[s + 1] - row[s]; i0 += TF_TILE) {
                tile_s.push_back(int64_t(s));
                tile_i0.push_back(i0);
            }
        const size_t ntiles = tile_s.size();
        const int knob = g_tf_path.load();
        const bool tiled = knob == SHYFT_HIP_TSFILTER_PATH_TILED ||
                           (knob == SHYFT_HIP_TSFILTER_PATH_AUTO && k_max >= TF_AUTO_MIN_K && np >= ntiles * (TF_TILE / 4));
        device_call c(device);
        dbuf<int64_t> d_row, d_wrow, d_wof, d_tile_s, d_tile_i0;
        dbuf<double> d_v, d_w, d_out;
        dbuf<int32_t> d_policy;
        c.upload(d_row, row, S + 1, TF_UPLOAD);
        c.upload(d_v, v, np, TF_UPLOAD);
        c.upload(d_wrow, w_row, W + 1, TF_UPLOAD);
        c.upload(d_w, w, size_t(w_row[W]), TF_UPLOAD);
        c.upload(d_wof, w_of, S, TF_UPLOAD);
        c.upload(d_policy, policy, S, TF_UPLOAD);
        if (tiled) {
            c.upload(d_tile_s, tile_s.data(), ntiles, TF_UPLOAD);
            c.upload(d_tile_i0, tile_i0.data(), ntiles, TF_UPLOAD);
        }
        d_out.alloc(np);
        tf_conv_args a{int64_t(np), int64_t(S), int64_t(ntiles), d_row.p, d_v.p, d_wrow.p, d_w.p, d_wof.p, d_policy.p,
                       d_tile_s.p, d_tile_i0.p, d_out.p};
        c.begin();
        if (tiled) {
            hipLaunchKernelGGL(tf_convolve_tiled_kernel, dim3(launch_blocks(ntiles)), dim3(TF_BLOCK), 0, c.s, a);
        } else {
            hipLaunchKernelGGL(tf_convolve_direct_kernel, dim3(tf_grid(np)), dim3(TF_BLOCK), 0, c.s, a);
        }
        hip_check(hipGetLastError(), "tsfilter convolve_w");
        g_tf.finish(c, "tsfilter", out, d_out.p, np, tiled ? SHYFT_HIP_TSFILTER_PATH_TILED : SHYFT_HIP_TSFILTER_PATH_DIRECT);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_convolve_w_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                 const int64_t* t_end, const int32_t* fx, size_t W, const int64_t* w_row,
                                 const double* w, const int64_t* w_of, const int32_t* policy, double* out) {
    namespace h = shyft_hip::host;
    (void)device;
    try {
        if (tf_prepare("shyft_hip_ts_convolve_w_host", S, row, t, v, t_end, fx, out)) return 0;
        tf_prepare_convolve("shyft_hip_ts_convolve_w_host", S, W, w_row, w, w_of, policy);
        for (size_t s = 0; s < S; ++s) {
            const h::point_ts ts = point_series(s, row, t, v, t_end, fx);
            const int64_t wb = w_row[w_of[s]];
            const size_t K = size_t(w_row[w_of[s] + 1] - wb);
            for (size_t i = 0; i < ts.size(); ++i)
                out[row[s] + int64_t(i)] = h::convolve_w_value(ts, w + wb, K, h::convolve_policy(policy[s]), i);
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_derivative(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                            const int64_t* t_end, const int32_t* fx, const int64_t* fixed_dt, const int32_t* method,
                            double* out) {
    try {
        if (tf_prepare("shyft_hip_ts_derivative", S, row, t, v, t_end, fx, out)) return 0;
        tf_prepare_derivative("shyft_hip_ts_derivative", S, row, t, t_end, fixed_dt, method);
        device_call c(device);
        const size_t np = size_t(row[S]);
        dbuf<int64_t> d_row, d_t, d_tend, d_dt;
        dbuf<double> d_v, d_out;
        dbuf<int32_t> d_fx, d_method;
        c.upload(d_row, row, S + 1, TF_UPLOAD);
        c.upload(d_t, t, np, TF_UPLOAD);
        c.upload(d_v, v, np, TF_UPLOAD);
        c.upload(d_tend, t_end, S, TF_UPLOAD);
        c.upload(d_fx, fx, S, TF_UPLOAD);
        c.upload(d_dt, fixed_dt, S, TF_UPLOAD);
        c.upload(d_method, method, S, TF_UPLOAD);
        d_out.alloc(np);
        tf_deriv_args a{int64_t(np), int64_t(S), d_row.p, d_t.p, d_v.p, d_tend.p, d_fx.p, d_dt.p, d_method.p, d_out.p};
        c.begin();
        hipLaunchKernelGGL(tf_derivative_kernel, dim3(tf_grid(np)), dim3(TF_BLOCK), 0, c.s, a);
        hip_check(hipGetLastError(), "tsfilter derivative");
        g_tf.finish(c, "tsfilter", out, d_out.p, np);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_derivative_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                 const int64_t* t_end, const int32_t* fx, const int64_t* fixed_dt,
                                 const int32_t* method, double* out) {
    namespace h = shyft_hip::host;
    (void)device;
    try {
        if (tf_prepare("shyft_hip_ts_derivative_host", S, row, t, v, t_end, fx, out)) return 0;
        tf_prepare_derivative("shyft_hip_ts_derivative_host", S, row, t, t_end, fixed_dt, method);
        for (size_t s = 0; s < S; ++s) {
            const h::point_ts ts = point_series(s, row, t, v, t_end, fx);
            for (size_t i = 0; i < ts.size(); ++i)
                out[row[s] + int64_t(i)] = h::derivative_value(ts, fixed_dt[s], h::derivative_method(method[s]), i);
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_inside(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                        const int64_t* t_end, const int32_t* fx, const double* min_x, const double* max_x,
                        const double* nan_x, const double* x_inside, const double* x_outside, double* out) {
    try {
        if (tf_prepare("shyft_hip_ts_inside", S, row, t, v, t_end, fx, out)) return 0;
        if (!min_x || !max_x || !nan_x || !x_inside || !x_outside)
            throw std::runtime_error("shyft_hip_ts_inside: null argument");
        device_call c(device);
        const size_t np = size_t(row[S]);
        dbuf<int64_t> d_row;
        dbuf<double> d_v, d_min, d_max, d_nan, d_in, d_outside, d_out;
        c.upload(d_row, row, S + 1, TF_UPLOAD);
        c.upload(d_v, v, np, TF_UPLOAD);
        c.upload(d_min, min_x, S, TF_UPLOAD);
        c.upload(d_max, max_x, S, TF_UPLOAD);
        c.upload(d_nan, nan_x, S, TF_UPLOAD);
        c.upload(d_in, x_inside, S, TF_UPLOAD);
        c.upload(d_outside, x_outside, S, TF_UPLOAD);
        d_out.alloc(np);
        tf_inside_args a{int64_t(np), int64_t(S), d_row.p, d_v.p, d_min.p, d_max.p, d_nan.p, d_in.p, d_outside.p, d_out.p};
        c.begin();
        hipLaunchKernelGGL(tf_inside_kernel, dim3(tf_grid(np)), dim3(TF_BLOCK), 0, c.s, a);
        hip_check(hipGetLastError(), "tsfilter inside");
        g_tf.finish(c, "tsfilter", out, d_out.p, np);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_inside_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, const double* min_x, const double* max_x,
                             const double* nan_x, const double* x_inside, const double* x_outside, double* out) {
    namespace h = shyft_hip::host;
    (void)device;
    try {
        if (tf_prepare("shyft_hip_ts_inside_host", S, row, t, v, t_end, fx, out)) return 0;
        if (!min_x || !max_x || !nan_x || !x_inside || !x_outside)
            throw std::runtime_error("shyft_hip_ts_inside_host: null argument");
        for (size_t s = 0; s < S; ++s) {
            h::inside_parameter p;
            p.min_x = min_x[s];
            p.max_x = max_x[s];
            p.nan_x = nan_x[s];
            p.x_inside = x_inside[s];
            p.x_outside = x_outside[s];
            for (int64_t k = row[s]; k < row[s + 1]; ++k) out[k] = p.inside_value(v[k]);
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_decode(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                        const int64_t* t_end, const int32_t* fx, const int32_t* start_bit, const int32_t* n_bits,
                        double* out) {
    try {
        if (tf_prepare("shyft_hip_ts_decode", S, row, t, v, t_end, fx, out)) return 0;
        tf_prepare_decode("shyft_hip_ts_decode", S, start_bit, n_bits);
        device_call c(device);
        const size_t np = size_t(row[S]);
        dbuf<int64_t> d_row;
        dbuf<double> d_v, d_out;
        dbuf<int32_t> d_start, d_bits;
        c.upload(d_row, row, S + 1, TF_UPLOAD);
        c.upload(d_v, v, np, TF_UPLOAD);
        c.upload(d_start, start_bit, S, TF_UPLOAD);
        c.upload(d_bits, n_bits, S, TF_UPLOAD);
        d_out.alloc(np);
        tf_decode_args a{int64_t(np), int64_t(S), d_row.p, d_v.p, d_start.p, d_bits.p, d_out.p};
        c.begin();
        hipLaunchKernelGGL(tf_decode_kernel, dim3(tf_grid(np)), dim3(TF_BLOCK), 0, c.s, a);
        hip_check(hipGetLastError(), "tsfilter decode");
        g_tf.finish(c, "tsfilter", out, d_out.p, np);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_decode_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, const int32_t* start_bit, const int32_t* n_bits,
                             double* out) {
    namespace h = shyft_hip::host;
    (void)device;
    try {
        if (tf_prepare("shyft_hip_ts_decode_host", S, row, t, v, t_end, fx, out)) return 0;
        tf_prepare_decode("shyft_hip_ts_decode_host", S, start_bit, n_bits);
        for (size_t s = 0; s < S; ++s) {
            const h::bit_decoder d{unsigned(start_bit[s]), unsigned(n_bits[s])};
            for (int64_t k = row[s]; k < row[s + 1]; ++k) out[k] = d.decode(v[k]);
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

double shyft_hip_tsfilter_last_ms(int device) { return g_tf.last_ms.load(device, 0.0); }

uint64_t shyft_hip_tsfilter_calls(int device) { return g_tf.calls.load(device, 0); }

int shyft_hip_tsfilter_last_path(int device) { return g_tf.last_path.load(device, SHYFT_HIP_TSFILTER_PATH_AUTO); }

int shyft_hip_tsfilter_set_path(int path) {
    if (path != SHYFT_HIP_TSFILTER_PATH_AUTO && path != SHYFT_HIP_TSFILTER_PATH_DIRECT &&
        path != SHYFT_HIP_TSFILTER_PATH_TILED)
        return fail(nullptr, "tsfilter: path must be AUTO, DIRECT or TILED");
    g_tf_path.store(path);
    return 0;
}

}  // extern "C"
