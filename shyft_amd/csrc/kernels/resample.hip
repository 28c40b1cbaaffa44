// Batched resampling of point series onto a fixed_dt axis for gfx950: the true average, the integral and the
// accumulated integral of S series over T intervals (core/time_series.h:202-310, 2033-2120;
// core/time_series_dd.h:532-538, 672-679).
//
// The S series come in CSR form: row [S+1] point offsets, t and v [row[S]] point times (int64 microseconds) and
// values, t_end [S] the end of each series' last interval, fx [S] the point type. The target axis is
// (ta_t0, ta_dt, T). out is [T][S], series fastest. A job is one (series, interval); every job is independent: it
// finds its own start point by binary search (point_dt::open_range_index_of, core/time_axis.h:329-374) and walks the
// points of its period as accumulate_value does (core/time_series.h:202-288). host/time_series.hpp holds the same
// statements in plain C++ and is the definition of correct; shyft_hip_resample_host runs those, not this file's.
//
//  AVERAGE     average_accessor::value(i): NaN when time(i) >= the series' end, else area / to_seconds(tsum), NaN
//              without covered time.
//  INTEGRAL    integral_ts::value(i): the area of period i, NaN when tsum == 0; no end-of-series rule.
//  ACCUMULATE  accumulate_accessor::value(i) driven in ascending i. Two kernels. The first stores 0.0 in row 0 and in
//              row i >= 1 the area of [time(i-1), time(i)), or NaN when time(i) >= the series' end. The second runs
//              one lane per series down the rows in order: row 1 is taken as it is (the accessor assigns the first
//              sum), every later row is q = q + row, one rounded add each in the accessor's order, and a NaN stays.
//
// Every operation is evaluated as written: int64 tick arithmetic, to_seconds(x) = double(x) / 1e6 as a division,
// no FMA (-ffp-contract=off), isfinite by the exponent bits. No atomics, no inline assembly.
//
// Two launch shapes for the first kernel. DIRECT: one lane per job, jobs numbered series-fastest, each lane stores
// its own result (coalesced stores, scattered point reads). TILED: a workgroup takes RS_TILE_S series x 64 intervals;
// a wavefront runs 64 neighbouring intervals of one series (neighbouring lanes read neighbouring points), parks the
// results in a padded LDS tile, and after a workgroup barrier the tile is stored series-fastest. Both loop
// grid-stride with 64-bit indexes; the loop count of TILED is uniform over the workgroup, so every lane meets every
// barrier.
//
// Index safety. The host checks before the launch that row[0] == 0 and row is non-decreasing, so a series' points
// are t[row[s] .. row[s+1]) inside the uploaded row[S] points, and that its times increase strictly and t_end lies
// after the last. rs_area (device/ts_area.h, shared with kernels/tsprep.hip) reads point k only with k < n: the start index is at most n - 1, every read is followed
// by the test `k == n` which ends the walk, and the one place where the reference reads without that test (a
// one-point series whose point lies inside a period that starts before it, where the reference throws from
// point_dt::time) is refused by the host check and, should it reach the device, ends the walk with NaN. A series
// with no points is never read. An interval index is < T and a series index < S, so out is written inside [T][S]
// only: DIRECT by job < T*S; TILED by its `i < T && s < S` tests. The LDS tile is [64][RS_TILE_S + 1] doubles and is
// indexed by lane < 64 and a series slot < RS_TILE_S. ta_t0 + T * ta_dt is checked on the host not to overflow.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../device/ts_area.h"
#include "../host/time_series.hpp"
#include "../include_internal/device_call.h"
#include "../include_internal/series_args.h"

using namespace shyft_hip_impl;

namespace {

constexpr int RS_BLOCK = 256;   // 4 wavefronts
constexpr int RS_TILE_S = 16;   // series per TILED workgroup tile: 128-byte runs in the [T][S] store
constexpr int RS_TILE_T = 64;   // intervals per tile: one per lane
constexpr int RS_TILE_LD = RS_TILE_S + 1;
constexpr int RS_SCAN_ROWS = 8;  // rows the ACCUMULATE scan loads ahead of its adds

struct rs_args {
    int mode;
    size_t S, T;
    const int64_t* row;
    const int64_t* t;
    const double* v;
    const int64_t* t_end;
    const int32_t* fx;
    int64_t ta_t0, ta_dt;
    double* out;
};

// one (series, interval) job; s < S, i < T
__device__ inline double rs_job(const rs_args& a, size_t s, size_t i) {
    const int64_t r0 = a.row[s];
    const int64_t n = a.row[s + 1] - r0;
    const int64_t src_end = n > 0 ? a.t_end[s] : 0;  // total_period().end of an empty series is 0
    const bool linear = a.fx[s] == int32_t(shyft_hip::host::POINT_INSTANT_VALUE);
    const int64_t ti = a.ta_t0 + int64_t(i) * a.ta_dt;
    int64_t ps, pe;
    if (a.mode == SHYFT_HIP_RESAMPLE_ACCUMULATE) {
        if (i == 0) return 0.0;
        if (ti >= src_end) return rs_nan();
        ps = ti - a.ta_dt;
        pe = ti;
    } else {
        if (a.mode == SHYFT_HIP_RESAMPLE_AVERAGE && ti >= src_end) return rs_nan();
        ps = ti;
        pe = ti + a.ta_dt;
    }
    if (n <= 0) return rs_nan();
    int64_t tsum = 0;
    const double area = rs_area(a.t + r0, a.v + r0, n, a.t_end[s], ps, pe, linear, tsum);
    if (a.mode == SHYFT_HIP_RESAMPLE_AVERAGE) return tsum > 0 ? area / rs_seconds(tsum) : rs_nan();
    return area;
}

__global__ __launch_bounds__(RS_BLOCK) void resample_direct_kernel(rs_args a) {
    const size_t jobs = a.T * a.S;
    const size_t stride = size_t(gridDim.x) * RS_BLOCK;
    for (size_t j = size_t(blockIdx.x) * RS_BLOCK + threadIdx.x; j < jobs; j += stride)
        a.out[j] = rs_job(a, j % a.S, j / a.S);
}

__global__ __launch_bounds__(RS_BLOCK) void resample_tiled_kernel(rs_args a) {
    __shared__ double tile[RS_TILE_T * RS_TILE_LD];
    const size_t tiles_s = (a.S + RS_TILE_S - 1) / RS_TILE_S;
    const size_t tiles_t = (a.T + RS_TILE_T - 1) / RS_TILE_T;
    const size_t tiles = tiles_s * tiles_t;
    const int lane = int(threadIdx.x & 63), wave = int(threadIdx.x >> 6);
    for (size_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {  // uniform over the workgroup
        const size_t s0 = (tl % tiles_s) * RS_TILE_S, i0 = (tl / tiles_s) * RS_TILE_T;
        const size_t i = i0 + size_t(lane);
        for (int k = wave; k < RS_TILE_S; k += RS_BLOCK / 64) {
            const size_t s = s0 + size_t(k);
            if (s < a.S && i < a.T) tile[lane * RS_TILE_LD + k] = rs_job(a, s, i);
        }
        __syncthreads();
        for (int e = int(threadIdx.x); e < RS_TILE_T * RS_TILE_S; e += RS_BLOCK) {
            const int k = e % RS_TILE_S, r = e / RS_TILE_S;
            const size_t s = s0 + size_t(k), ii = i0 + size_t(r);
            if (s < a.S && ii < a.T) a.out[ii * a.S + s] = tile[r * RS_TILE_LD + k];
        }
        __syncthreads();  // the tile is reused by the next round
    }
}

// ACCUMULATE, second step: one lane per series adds the rows in order (accumulate_accessor::value, :2112-2116)
__global__ __launch_bounds__(RS_BLOCK) void resample_scan_kernel(size_t S, size_t T, double* out) {
    const size_t stride = size_t(gridDim.x) * RS_BLOCK;
    for (size_t s = size_t(blockIdx.x) * RS_BLOCK + threadIdx.x; s < S; s += stride) {
        double q = 0.0;
        for (size_t i0 = 1; i0 < T; i0 += RS_SCAN_ROWS) {
            double d[RS_SCAN_ROWS];  // the loads of a batch of rows are issued together; the adds keep their order
#pragma unroll
            for (int u = 0; u < RS_SCAN_ROWS; ++u) d[u] = i0 + u < T ? out[(i0 + u) * S + s] : 0.0;
#pragma unroll
            for (int u = 0; u < RS_SCAN_ROWS; ++u) {
                const size_t i = i0 + u;
                if (i < T) {
                    q = i == 1 ? d[u] : q + d[u];
                    if (q != q) q = rs_nan();
                    out[i * S + s] = q;
                }
            }
        }
    }
}

// Argument checks shared by the device and the host entry: the axis and the batch here, the series through
// include_internal/series_args.h; true when there is nothing to do. The axis' share of the quarter-range test and the
// one-point rule keep their place after the checks of their series and before those of the next one.
bool rs_prepare(const char* who, int mode, size_t S, const int64_t* row, const int64_t* t, const double* v,
                const int64_t* t_end, const int32_t* fx, int64_t ta_t0, int64_t ta_dt, size_t T, const double* out) {
    if (mode != SHYFT_HIP_RESAMPLE_AVERAGE && mode != SHYFT_HIP_RESAMPLE_INTEGRAL && mode != SHYFT_HIP_RESAMPLE_ACCUMULATE)
        throw std::runtime_error("resample: mode must be AVERAGE, INTEGRAL or ACCUMULATE");
    if (S == 0 || T == 0) return true;
    if (!(ta_dt > 0)) throw std::runtime_error("resample: the time-axis needs a delta-t larger than 0");
    const int64_t i64max = std::numeric_limits<int64_t>::max(), i64min = std::numeric_limits<int64_t>::min();
    if (T > size_t(i64max / ta_dt) || ta_t0 > i64max - int64_t(T) * ta_dt)
        throw std::runtime_error("resample: the time-axis does not fit in 64-bit microseconds");
    if (T > std::numeric_limits<size_t>::max() / sizeof(double) / S) throw std::runtime_error("resample: the batch is too large");
    if (!out) throw std::runtime_error(std::string(who) + ": null argument");
    check_point_series_rows(who, "resample", S, row, t, v, t_end, fx);
    const int64_t ta_end = ta_t0 + int64_t(T) * ta_dt;
    for (size_t s = 0; s < S; ++s) {
        check_point_series_at("resample", s, row, t, t_end, fx);
        const int64_t b = row[s], e = row[s + 1];
        if (b == e) continue;
        // the sums to_seconds(px.start + px.end) and p.end - p.start stay inside int64
        if (ta_t0 < i64min / 4 || ta_end > i64max / 4)
            throw std::runtime_error("resample: times beyond a quarter of the 64-bit range are not supported");
        if (e - b == 1) {
            // accumulate_value reads point 1 of a one-point series when the point lies inside a period that starts
            // before it; the reference throws out of point_dt::time (core/time_axis.h:317-322)
            const int64_t last = mode == SHYFT_HIP_RESAMPLE_ACCUMULATE ? ta_end - ta_dt : ta_end;
            if (t[b] > ta_t0 && t[b] < last && (t[b] - ta_t0) % ta_dt != 0)
                throw std::runtime_error("point_dt.time(i): a one-point series cannot be integrated over a period "
                                         "that starts before its point and holds it");
        }
    }
    return false;
}

call_record g_rs;
std::atomic<int> g_rs_path{SHYFT_HIP_RESAMPLE_PATH_AUTO};
constexpr const char* RS_UPLOAD = "resample upload";

}  // namespace

extern "C" {

int shyft_hip_resample(int device, int mode, size_t S, const int64_t* row, const int64_t* t, const double* v,
                       const int64_t* t_end, const int32_t* fx, int64_t ta_t0, int64_t ta_dt, size_t T, double* out) {
    try {
        if (rs_prepare("shyft_hip_resample", mode, S, row, t, v, t_end, fx, ta_t0, ta_dt, T, out)) return 0;
        device_call c(device);
        const size_t np = size_t(row[S]);
        dbuf<int64_t> d_row, d_t, d_tend;
        dbuf<double> d_v, d_out;
        dbuf<int32_t> d_fx;
        c.upload(d_row, row, S + 1, RS_UPLOAD);
        c.upload(d_t, t, np, RS_UPLOAD);
        c.upload(d_v, v, np, RS_UPLOAD);
        c.upload(d_tend, t_end, S, RS_UPLOAD);
        c.upload(d_fx, fx, S, RS_UPLOAD);
        d_out.alloc(T * S);
        rs_args a{};
        a.mode = mode;
        a.S = S;
        a.T = T;
        a.row = d_row.p;
        a.t = d_t.p;
        a.v = d_v.p;
        a.t_end = d_tend.p;
        a.fx = d_fx.p;
        a.ta_t0 = ta_t0;
        a.ta_dt = ta_dt;
        a.out = d_out.p;
        const int knob = g_rs_path.load();
        const bool tiled = knob == SHYFT_HIP_RESAMPLE_PATH_TILED ||
                           (knob == SHYFT_HIP_RESAMPLE_PATH_AUTO && T >= size_t(RS_TILE_T));
        c.begin();
        if (tiled) {
            const size_t tiles = ((S + RS_TILE_S - 1) / RS_TILE_S) * ((T + RS_TILE_T - 1) / RS_TILE_T);
            hipLaunchKernelGGL(resample_tiled_kernel, dim3(launch_blocks(tiles)), dim3(RS_BLOCK), 0, c.s, a);
        } else {
            hipLaunchKernelGGL(resample_direct_kernel, dim3(launch_blocks((T * S + RS_BLOCK - 1) / RS_BLOCK)),
                               dim3(RS_BLOCK), 0, c.s, a);
        }
        hip_check(hipGetLastError(), "resample");
        if (mode == SHYFT_HIP_RESAMPLE_ACCUMULATE) {
            hipLaunchKernelGGL(resample_scan_kernel, dim3(launch_blocks((S + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0,
                               c.s, S, T, d_out.p);
            hip_check(hipGetLastError(), "resample scan");
        }
        g_rs.finish(c, "resample", out, d_out.p, T * S, tiled ? SHYFT_HIP_RESAMPLE_PATH_TILED : SHYFT_HIP_RESAMPLE_PATH_DIRECT);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_resample_host(int device, int mode, size_t S, const int64_t* row, const int64_t* t, const double* v,
                            const int64_t* t_end, const int32_t* fx, int64_t ta_t0, int64_t ta_dt, size_t T,
                            double* out) {
    namespace h = shyft_hip::host;
    (void)device;
    try {
        if (rs_prepare("shyft_hip_resample_host", mode, S, row, t, v, t_end, fx, ta_t0, ta_dt, T, out)) return 0;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const h::fixed_dt ta(ta_t0, ta_dt, T);
        for (size_t s = 0; s < S; ++s) {
            const h::point_ts source = point_series(s, row, t, v, t_end, fx);
            const bool linear = source.fx == h::POINT_INSTANT_VALUE;
            if (mode == SHYFT_HIP_RESAMPLE_AVERAGE) {
                const std::vector<double> r = h::average_values(source, ta);
                for (size_t i = 0; i < T; ++i) out[i * S + s] = r[i];
            } else if (mode == SHYFT_HIP_RESAMPLE_INTEGRAL) {  // integral_ts::value (time_series_dd.h:532-538)
                for (size_t i = 0; i < T; ++i) {
                    size_t ix_hint = 0;
                    h::utctimespan tsum = 0;
                    out[i * S + s] = h::accumulate_value(source, ta.period(i), ix_hint, tsum, linear);
                }
            } else {  // accumulate_ts::values over accumulate_accessor::value (time_series.h:2100-2120), USE_NAN
                size_t last_idx = 0, q_idx = h::npos;
                double q_value = 0.0;
                for (size_t i = 0; i < T; ++i) {
                    if (i == 0) {
                        out[s] = 0.0;
                        continue;
                    }
                    if (ta.time(i) >= source.total_period().end) {
                        q_value = nan;
                    } else {
                        h::utctimespan tsum = 0;
                        const h::utctime te = ta.time(i);
                        if (i > q_idx && q_idx != h::npos)
                            q_value += h::accumulate_value(source, h::utcperiod(ta.time(q_idx), te), last_idx, tsum, linear);
                        else
                            q_value = h::accumulate_value(source, h::utcperiod(ta.time(0), te), last_idx, tsum, linear);
                    }
                    q_idx = i;
                    out[i * S + s] = q_value;
                }
            }
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

double shyft_hip_resample_last_ms(int device) { return g_rs.last_ms.load(device, 0.0); }

uint64_t shyft_hip_resample_calls(int device) { return g_rs.calls.load(device, 0); }

int shyft_hip_resample_last_path(int device) { return g_rs.last_path.load(device, SHYFT_HIP_RESAMPLE_PATH_AUTO); }

int shyft_hip_resample_set_path(int path) {
    if (path != SHYFT_HIP_RESAMPLE_PATH_AUTO && path != SHYFT_HIP_RESAMPLE_PATH_DIRECT &&
        path != SHYFT_HIP_RESAMPLE_PATH_TILED)
        return fail(nullptr, "resample: path must be AUTO, DIRECT or TILED");
    g_rs_path.store(path);
    return 0;
}

}  // extern "C"
