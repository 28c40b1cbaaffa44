// Percentiles of a vector of point series on a fixed_dt axis for gfx950: calculate_percentiles with skip_nans
// (core/time_series_statistics.h:184-246) over S views of R stored series, one fused launch. It replaces one
// average_accessor pass per series, a full sort per interval and two extract_statistic_from_vector passes.
//
// The stored series come in the CSR form of shyft_hip_resample: row [R+1], t and v [row[R]], t_end [R], fx [R]. A view
// is (src, shift): stored series src with every point time and its t_end moved by shift microseconds (time_shift_ts,
// core/time_series_dd.h:707-751), so the partitions of one long record (partition_by, core/time_series.h:2451-2494)
// are uploaded once. The sample of (view s, interval i) is average_accessor::value(i) with USE_NAN, mode AVERAGE of
// kernels/resample.hip: rs_area (device/ts_area.h) over the view's moved times, divided by to_seconds of the covered
// time. It goes from rs_area straight into the sort; no [T][S] table is written to memory. out is [n_pct][T].
// host/ts_percentiles.hpp holds the same statements in plain C++ and is the definition of correct;
// shyft_hip_ts_percentiles_host runs those, not this file's.
//
//  keys     every sample maps to the order-preserving 64-bit key of device/workgroup.h, a non-finite one to the
//           all-ones sentinel (above the key of every finite value), so the order statistics are exact integer
//           selections. +0.0 and -0.0 are different keys that compare equal as doubles: the sign of a zero result is
//           unspecified, as for the cell percentiles.
//  WAVE     S <= 64: one wavefront per interval, four intervals per workgroup. Lane s evaluates view s; the 64 keys are
//           bitonic-sorted across the lanes with cross-lane moves, no LDS and no barrier; nf, the number of finite
//           samples, comes from a ballot.
//  LDS      S <= SHYFT_HIP_TS_PERCENTILES_MAX_SERIES: one workgroup per interval. Lanes stride over the views, compact
//           the finite keys into a power-of-two LDS array (at most 32 KiB; the slot comes from an integer LDS counter,
//           and as a full sort follows the order of arrival cannot change a result), pad it with sentinels and
//           bitonic-sort it there (lds_sort_pad and lds_bitonic_sort of device/workgroup.h, which
//           pct_lds_sort_kernel of kernels/percentiles.hip calls too).
//  0..100   reads ranks min(rank, nf - 1) through pct_make_plan; lower + delta * (upper - lower) is a separately
//           rounded multiply and add (-ffp-contract=off).
//  -1       the sorted finite samples added in sorted order by one lane, divided by nf: the host's sum, bit for bit.
//  +-1000   not order statistics of the averages but extract_statistic_from_vector with nan_min / nan_max
//           (time_series_statistics.h:24-90, :221-226): the fold over the raw point values inside the interval, across
//           all views. Only evaluated when pct holds one of them.
//
// The extremes in closed form. host/ts_percentiles.hpp extract_statistics_into runs, for one view with moved times
// t[0..n) and the contiguous periods [ps_i, pe_i) of the axis, pe_i == ps_(i+1):
//     is = index_of(ta.time(0))         the last k with t[k] <= ps_0, or npos when n == 0, ps_0 < t[0] or ps_0 >= t_end
//     for each i:
//       if is == npos: if t[0] is inside period i then is = 0, else emit NaN and go on
//       if is < n and t[is] < ps_i: ++is          (once)
//       while is < n and t[is] < pe_i: fold v[is]; ++is
// Started from a k with t[k] <= ps_0, the single ++is leaves is at the first point >= ps_0 (t[k + 1] > ps_0 by the
// choice of k). The while loop then folds exactly the points inside [ps_i, pe_i) and leaves is at the first point
// >= pe_i = ps_(i+1), so in every later interval the ++is test is false and the loop again folds exactly the points
// inside the interval. Started from npos with ps_0 < t[0], every interval before the one that holds t[0] holds no
// point and emits NaN, the fold over nothing; from that interval on is = 0 is the first point >= ps_i and the same
// holds. Started from npos with ps_0 >= t_end, or with n == 0, no point lies at or after ps_0 and everything is NaN.
// So interval i of one view is the nan_min / nan_max fold over { v[k] : ps_i <= t[k] < pe_i }, found by two lower-bound
// searches over the stored times for ps_i - shift and pe_i - shift, and nothing for a view whose moved t_end is at or
// before ta.time(0) or that has no points. nan_min / nan_max over finite values are min / max, which in key space are
// integer min / max: exact and free of order (up to the sign of a zero), reduced over the wavefront by cross-lane
// moves and over the workgroup through LDS.
//
// Every operation is evaluated as written: int64 tick arithmetic, to_seconds(x) = double(x) / 1e6 as a division, no FMA
// (-ffp-contract=off), isfinite by the exponent bits. No floating-point atomics, no global atomics, no inline assembly.
//
// Index safety. The host checks before the launch that row[0] == 0 and row is non-decreasing, so stored series r has
// the points t[row[r] .. row[r+1]) inside the uploaded row[R] points, that its times increase strictly and t_end lies
// after the last, and that every src[s] is in [0, R). A view index is < S and an interval index < T. rs_area reads
// point k only with k < n (device/ts_area.h); a series without points is never read. A lower-bound search (first_false,
// device/workgroup.h) reads t[m] with lo <= m < hi <= n only, and the fold runs over [lo, hi) inside [0, n). ps - shift and pe - shift cannot
// overflow: the host keeps the axis, the shifts and the moved series inside a quarter of the int64 range. The WAVE
// sort moves keys between the 64 lanes of a wavefront and reads lane min(rank, nf - 1) < 64. The LDS array has P
// keys, P the power of two >= S sized by the launcher; at most S <= P slots are taken by the compaction, the pad and
// the sort index below Q <= P, the power of two >= nf (device/workgroup.h), and ranks are read at min(rank, nf - 1). out is written at
// [e][i] with e < n_pct and i < T only. An interval without a finite sample writes NaN and reads no key.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../device/pct_plan.h"
#include "../device/ts_area.h"
#include "../device/workgroup.h"
#include "../host/ts_percentiles.hpp"
#include "../include_internal/device_call.h"
#include "../include_internal/kernels.h"
#include "../include_internal/series_args.h"

using namespace shyft_hip_impl;

namespace {

constexpr int TP_BLOCK = 256;  // 4 wavefronts
constexpr int TP_WAVES = TP_BLOCK / 64;
constexpr int TP_WAVE_MAX = 64;  // views of the WAVE shape: one per lane
constexpr uint64_t TP_NONE_MIN = ~0ull;  // above every finite key: no finite point folded yet (and the sort's sentinel)
constexpr uint64_t TP_NONE_MAX = 0ull;   // below every finite key

struct tp_args {
    int S;
    int64_t T;
    int sort, any_avg, extremes;  // an entry other than +-1000; an entry -1; an entry +-1000
    const int64_t* row;
    const int64_t* t;
    const double* v;
    const int64_t* t_end;
    const int32_t* fx;
    const int32_t* src;
    const int64_t* shift;
    int64_t ta_t0, ta_dt;
    pct_list pl;
    double* out;
};

// average_accessor::value of view s over [ps, ps + ta_dt); s < S
__device__ inline double tp_sample(const tp_args& a, int s, int64_t ps) {
    const int32_t r = a.src[s];
    const int64_t r0 = a.row[r];
    const int64_t n = a.row[r + 1] - r0;
    if (n <= 0) return rs_nan();
    const int64_t sh = a.shift[s];
    const int64_t te = a.t_end[r] + sh;
    if (ps >= te) return rs_nan();
    const bool linear = a.fx[r] == int32_t(shyft_hip::host::POINT_INSTANT_VALUE);
    int64_t tsum = 0;
    const double area = rs_area(a.t + r0, a.v + r0, n, te, ps, ps + a.ta_dt, linear, tsum, sh);
    return tsum > 0 ? area / rs_seconds(tsum) : rs_nan();
}

// the finite point values of view s inside [ps, pe) folded into kmin / kmax in key space (the closed form above)
__device__ inline void tp_extremes(const tp_args& a, int s, int64_t ps, int64_t pe, uint64_t& kmin, uint64_t& kmax) {
    const int32_t r = a.src[s];
    const int64_t r0 = a.row[r];
    const int64_t n = a.row[r + 1] - r0;
    if (n <= 0) return;
    const int64_t sh = a.shift[s];
    if (a.t_end[r] + sh <= a.ta_t0) return;
    const int64_t* __restrict__ t = a.t + r0;
    const double* __restrict__ v = a.v + r0;
    // the first points at or after ps and pe on the stored times
    const int64_t lo = first_false(int64_t(0), n, [&](int64_t m) { return t[m] < ps - sh; });
    const int64_t hi = first_false(lo, n, [&](int64_t m) { return t[m] < pe - sh; });
    for (int64_t k = lo; k < hi; ++k) {
        uint64_t key;
        if (key_of(v[k], key)) {
            kmin = key < kmin ? key : kmin;
            kmax = key > kmax ? key : kmax;
        }
    }
}

// entry e of one interval from the plan's two sorted samples, the sorted sum and the folded extremes
__device__ inline double tp_entry(int64_t p, const pct_plan& q, double lower, double upper, double avg, uint64_t kmin,
                                  uint64_t kmax) {
    if (p == -1000) return kmin == TP_NONE_MIN ? rs_nan() : value_of(kmin);
    if (p == 1000) return kmax == TP_NONE_MAX ? rs_nan() : value_of(kmax);
    if (q.kind == PCT_AVG) return avg;
    if (q.kind == PCT_NAN) return rs_nan();
    return pct_value(q, lower, upper);
}

// WAVE: S <= 64. The interval loop is uniform over a wavefront, so all 64 lanes take part in every cross-lane move.
__global__ __launch_bounds__(TP_BLOCK) void ts_percentiles_wave_kernel(tp_args a) {
    const int lane = int(threadIdx.x & 63), wave = int(threadIdx.x >> 6);
    for (int64_t i = int64_t(blockIdx.x) * TP_WAVES + wave; i < a.T; i += int64_t(gridDim.x) * TP_WAVES) {
        const int64_t ps = a.ta_t0 + i * a.ta_dt, pe = ps + a.ta_dt;
        uint64_t key = TP_NONE_MIN;
        bool finite = false;
        if (a.sort && lane < a.S) {
            finite = key_of(tp_sample(a, lane, ps), key);
            if (!finite) key = TP_NONE_MIN;
        }
        const int nf = __popcll(__ballot(finite));
        double avg = rs_nan();
        if (a.sort) {
            key = wave_bitonic_sort(key, lane);
            if (a.any_avg && nf > 0) {
                double sum = 0.0;
                for (int r = 0; r < nf; ++r) sum += value_of(__shfl(key, r, 64));  // in sorted order, as the host adds
                avg = sum / double(nf);
            }
        }
        uint64_t kmin = TP_NONE_MIN, kmax = TP_NONE_MAX;
        if (a.extremes) {
            if (lane < a.S) tp_extremes(a, lane, ps, pe, kmin, kmax);
            kmin = wave_reduce(kmin, op_min());
            kmax = wave_reduce(kmax, op_max());
        }
        const int e = lane < a.pl.n ? lane : 0;
        const int64_t p = a.pl.p[e];
        const pct_plan q = pct_make_plan(p, nf);
        const int last = nf > 0 ? nf - 1 : 0;
        const double lower = value_of(__shfl(key, int(q.lo) < last ? int(q.lo) : last, 64));
        const double upper = value_of(__shfl(key, int(q.hi) < last ? int(q.hi) : last, 64));
        if (lane < a.pl.n) a.out[int64_t(e) * a.T + i] = tp_entry(p, q, lower, upper, avg, kmin, kmax);
    }
}

// LDS: one workgroup per interval; keys[P] in dynamic LDS. The interval loop is uniform over the workgroup, so every
// lane meets every barrier.
__global__ __launch_bounds__(TP_BLOCK) void ts_percentiles_lds_kernel(tp_args a, int P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tp_smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(tp_smem);
    __shared__ uint32_t n_fin;
    __shared__ double avg_s;
    __shared__ uint64_t part_min[TP_WAVES], part_max[TP_WAVES];
    const int lane = int(threadIdx.x & 63), wave = int(threadIdx.x >> 6);
    if (a.S > P) return;  // never: the launcher sizes P from S
    for (int64_t i = blockIdx.x; i < a.T; i += gridDim.x) {
        const int64_t ps = a.ta_t0 + i * a.ta_dt, pe = ps + a.ta_dt;
        int nf = 0;
        if (a.sort) {
            if (threadIdx.x == 0) n_fin = 0u;
            __syncthreads();
            // compact the finite keys (their order in LDS is arbitrary: the sort follows); at most S <= P slots
            for (int s = int(threadIdx.x); s < a.S; s += TP_BLOCK) {
                uint64_t key;
                if (key_of(tp_sample(a, s, ps), key)) keys[atomicAdd(&n_fin, 1u)] = key;
            }
            __syncthreads();
            nf = int(n_fin);
            const int Q = lds_sort_pad<false>(keys, nullptr, nf, int(threadIdx.x), TP_BLOCK);  // power of two >= nf, <= P
            __syncthreads();
            lds_bitonic_sort<false, false>(keys, nullptr, Q, int(threadIdx.x), TP_BLOCK);
        }
        // one lane adds the sorted samples in order, as the host does, while the other wavefronts fold the extremes
        if (threadIdx.x == 0 && a.any_avg) {
            double sum = 0.0;
            for (int r = 0; r < nf; ++r) sum += value_of(keys[r]);
            avg_s = nf > 0 ? sum / double(nf) : rs_nan();
        }
        if (a.extremes) {
            uint64_t kmin = TP_NONE_MIN, kmax = TP_NONE_MAX;
            for (int s = int(threadIdx.x); s < a.S; s += TP_BLOCK) tp_extremes(a, s, ps, pe, kmin, kmax);
            kmin = wave_reduce(kmin, op_min());
            kmax = wave_reduce(kmax, op_max());
            if (lane == 0) {
                part_min[wave] = kmin;
                part_max[wave] = kmax;
            }
        }
        __syncthreads();
        if (int(threadIdx.x) < a.pl.n) {
            const int e = int(threadIdx.x);
            const int64_t p = a.pl.p[e];
            const pct_plan q = pct_make_plan(p, nf);
            uint64_t kmin = TP_NONE_MIN, kmax = TP_NONE_MAX;
            if (a.extremes)
                for (int w = 0; w < TP_WAVES; ++w) {
                    kmin = part_min[w] < kmin ? part_min[w] : kmin;
                    kmax = part_max[w] > kmax ? part_max[w] : kmax;
                }
            double lower = rs_nan(), upper = rs_nan();
            if (q.kind == PCT_SINGLE || q.kind == PCT_LERP) {  // nf > 0
                const uint32_t last = uint32_t(nf - 1);
                lower = value_of(keys[q.lo < last ? q.lo : last]);
                upper = value_of(keys[q.hi < last ? q.hi : last]);
            }
            a.out[int64_t(e) * a.T + i] = tp_entry(p, q, lower, upper, a.any_avg ? avg_s : rs_nan(), kmin, kmax);
        }
        __syncthreads();  // keys, avg_s and the parts are reused by the next round
    }
}

// Argument checks shared by the device and the host entry: the axis and the batch here, the stored series through
// include_internal/series_args.h, the views through host/ts_percentiles.hpp; true when there is nothing to do.
bool tp_prepare(const char* who, size_t R, const int64_t* row, const int64_t* t, const double* v, const int64_t* t_end,
                const int32_t* fx, size_t S, const int32_t* src, const int64_t* shift, int64_t ta_t0, int64_t ta_dt,
                size_t T, const int64_t* pct, size_t n_pct, const double* out) {
    namespace h = shyft_hip::host;
    if (S == 0 || T == 0 || n_pct == 0) return true;
    if (!(ta_dt > 0)) throw std::runtime_error("ts_percentiles: the time-axis needs a delta-t larger than 0");
    const int64_t i64max = std::numeric_limits<int64_t>::max();
    if (T > size_t(i64max / ta_dt) || ta_t0 > i64max - int64_t(T) * ta_dt)
        throw std::runtime_error("ts_percentiles: the time-axis does not fit in 64-bit microseconds");
    if (T > std::numeric_limits<size_t>::max() / sizeof(double) / n_pct ||
        T > std::numeric_limits<size_t>::max() / sizeof(double) / S)
        throw std::runtime_error("ts_percentiles: the batch is too large");
    if (!out || !pct || !src || !shift) throw std::runtime_error(std::string(who) + ": null argument");
    check_point_series(who, "ts_percentiles", R, row, t, v, t_end, fx);
    h::check_views(R, row, t, t_end, S, src, shift, h::fixed_dt(ta_t0, ta_dt, T));
    return false;
}

call_record g_tp;
std::atomic<int> g_tp_path{SHYFT_HIP_TS_PERCENTILES_PATH_AUTO};
constexpr const char* TP_UPLOAD = "ts_percentiles upload";

}  // namespace

extern "C" {

int shyft_hip_ts_percentiles(int device, size_t R, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, size_t S, const int32_t* src,
                             const int64_t* shift, int64_t ta_t0, int64_t ta_dt, size_t T, const int64_t* pct,
                             size_t n_pct, double* out) {
    try {
        if (S == 0 || T == 0 || n_pct == 0) return 0;
        if (n_pct > size_t(SHYFT_HIP_PERCENTILES_MAX))
            throw std::runtime_error("ts_percentiles: more than SHYFT_HIP_PERCENTILES_MAX = " +
                                     std::to_string(SHYFT_HIP_PERCENTILES_MAX) + " percentiles are not supported on the device");
        if (S > size_t(SHYFT_HIP_TS_PERCENTILES_MAX_SERIES))
            throw std::runtime_error("ts_percentiles: more than SHYFT_HIP_TS_PERCENTILES_MAX_SERIES = " +
                                     std::to_string(SHYFT_HIP_TS_PERCENTILES_MAX_SERIES) + " series are not supported on the device");
        const int knob = g_tp_path.load();
        if (knob == SHYFT_HIP_TS_PERCENTILES_PATH_WAVE && S > size_t(TP_WAVE_MAX))
            throw std::runtime_error("ts_percentiles: the WAVE path takes at most 64 series");
        if (tp_prepare("shyft_hip_ts_percentiles", R, row, t, v, t_end, fx, S, src, shift, ta_t0, ta_dt, T, pct, n_pct, out))
            return 0;
        device_call c(device);
        const size_t np = size_t(row[R]);
        dbuf<int64_t> d_row, d_t, d_tend, d_shift;
        dbuf<double> d_v, d_out;
        dbuf<int32_t> d_fx, d_src;
        c.upload(d_row, row, R + 1, TP_UPLOAD);
        c.upload(d_t, t, np, TP_UPLOAD);
        c.upload(d_v, v, np, TP_UPLOAD);
        c.upload(d_tend, t_end, R, TP_UPLOAD);
        c.upload(d_fx, fx, R, TP_UPLOAD);
        c.upload(d_src, src, S, TP_UPLOAD);
        c.upload(d_shift, shift, S, TP_UPLOAD);
        d_out.alloc(n_pct * T);
        tp_args a{};
        a.S = int(S);
        a.T = int64_t(T);
        a.pl.n = int(n_pct);
        for (size_t k = 0; k < n_pct; ++k) {
            a.pl.p[k] = pct[k];
            if (pct[k] == -1000 || pct[k] == 1000) a.extremes = 1;
            else a.sort = 1;
            if (pct[k] == -1) a.any_avg = 1;
        }
        a.row = d_row.p;
        a.t = d_t.p;
        a.v = d_v.p;
        a.t_end = d_tend.p;
        a.fx = d_fx.p;
        a.src = d_src.p;
        a.shift = d_shift.p;
        a.ta_t0 = ta_t0;
        a.ta_dt = ta_dt;
        a.out = d_out.p;
        const bool wave = knob == SHYFT_HIP_TS_PERCENTILES_PATH_WAVE ||
                          (knob == SHYFT_HIP_TS_PERCENTILES_PATH_AUTO && S <= size_t(TP_WAVE_MAX));
        c.begin();
        if (wave) {
            hipLaunchKernelGGL(ts_percentiles_wave_kernel, dim3(launch_blocks((T + TP_WAVES - 1) / TP_WAVES)),
                               dim3(TP_BLOCK), 0, c.s, a);
        } else {
            int P = 1;
            while (size_t(P) < S) P <<= 1;
            hipLaunchKernelGGL(ts_percentiles_lds_kernel, dim3(launch_blocks(T)), dim3(TP_BLOCK),
                               size_t(P) * sizeof(uint64_t), c.s, a, P);
        }
        hip_check(hipGetLastError(), "ts_percentiles");
        g_tp.finish(c, "ts_percentiles", out, d_out.p, n_pct * T,
                    wave ? SHYFT_HIP_TS_PERCENTILES_PATH_WAVE : SHYFT_HIP_TS_PERCENTILES_PATH_LDS);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_percentiles_host(int device, size_t R, const int64_t* row, const int64_t* t, const double* v,
                                  const int64_t* t_end, const int32_t* fx, size_t S, const int32_t* src,
                                  const int64_t* shift, int64_t ta_t0, int64_t ta_dt, size_t T, const int64_t* pct,
                                  size_t n_pct, double* out) {
    namespace h = shyft_hip::host;
    (void)device;
    try {
        if (tp_prepare("shyft_hip_ts_percentiles_host", R, row, t, v, t_end, fx, S, src, shift, ta_t0, ta_dt, T, pct, n_pct,
                       out))
            return 0;
        std::vector<h::point_ts> rows;
        rows.reserve(R);
        for (size_t r = 0; r < R; ++r) rows.push_back(point_series(r, row, t, v, t_end, fx));
        h::ts_percentiles(rows, S, src, shift, h::fixed_dt(ta_t0, ta_dt, T), pct, n_pct, out);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

double shyft_hip_ts_percentiles_last_ms(int device) { return g_tp.last_ms.load(device, 0.0); }

uint64_t shyft_hip_ts_percentiles_calls(int device) { return g_tp.calls.load(device, 0); }

int shyft_hip_ts_percentiles_last_path(int device) {
    return g_tp.last_path.load(device, SHYFT_HIP_TS_PERCENTILES_PATH_AUTO);
}

int shyft_hip_ts_percentiles_set_path(int path) {
    if (path != SHYFT_HIP_TS_PERCENTILES_PATH_AUTO && path != SHYFT_HIP_TS_PERCENTILES_PATH_WAVE &&
        path != SHYFT_HIP_TS_PERCENTILES_PATH_LDS)
        return fail(nullptr, "ts_percentiles: path must be AUTO, WAVE or LDS");
    g_tp_path.store(path);
    return 0;
}

}  // extern "C"
