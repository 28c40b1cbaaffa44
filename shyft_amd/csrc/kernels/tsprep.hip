// Observation preparation of a batch of S point series for gfx950: rating curve, ice-packing detection, ice-packing
// recession and min-max check with linear fill (core/time_series.h:1255-1546, 1653-1831;
// core/time_series_dd.h:1186-1365, 1456-1478; core/time_series_dd.cpp:1335-1376). host/ts_prep.hpp holds the same
// statements in plain C++ and is the definition of correct; the _host entries run those, not this file's.
//
// The series come in the CSR form of shyft_hip_resample: row [S+1] point offsets, t and v [row[S]] point times (int64
// microseconds) and values, t_end [S], fx [S]. An output is one double per input point (per query for ice-packing), in
// the same CSR order. Every operation is evaluated as written: int64 tick arithmetic, to_seconds(x) = double(x) / 1e6
// as a division, no FMA (-ffp-contract=off), isfinite by the exponent bits, exp and pow from detmath. No atomics, no
// inline assembly, and no workgroup ever waits for another one.
//
//  RATING   one lane per point, grid-stride. Parameter packs are a three-level CSR: pack_row [P+1] -> curve start
//           times curve_t [C] -> curve_row [C+1] -> segments seg [G][4] = lower, a, b, c; pack_of [S] names the pack of
//           a series. rating_curve_parameters::flow(t, level): lower_bound over the curve times, then
//           rating_curve_function::flow: lower_bound over `lower < level`.
//  ICE      one lane per query; queries have their own CSR (qrow [S+1], qt). ice_packing_ts::detect_ice_packing(t):
//           rs_area (device/ts_area.h, the device form of accumulate_value) over [t - window, t) after the policy's
//           clip. Neighbouring lanes are neighbouring queries of one series.
//  RECESSION and FILL are index scans over the flat point array, each in three launches: tp_scan_block_kernel (a
//           workgroup scans TP_SPAN keys: per-lane runs, then block_scan of device/workgroup.h over the lanes, and stores
//           the running maxima and its aggregate), tp_scan_agg_kernel (one workgroup scans the aggregates in order), and
//           the finish kernel, which combines the two and computes the value exactly as the host statement does.
//
// Why the scans equal the literal walks.
//  RECESSION (ice_packing_recession_ts::evaluate). Let ice(k) be "indicator k finite and > 0.5". For a point i with
//  ice(i) the walk `while (f_ix > 0 && ice > limit) { ice = ind(--f_ix); if (!isfinite(ice)) return nan; }` steps
//  down from i and ends at the largest k < i with not ice(k): there it either returns NaN (indicator k not finite) or
//  leaves the loop (indicator k <= 0.5) with f_ix = k. Without such a k inside the series it ends at point 0 of the
//  series, whose indicator was finite and > 0.5, with f_ix = 0. Point 0 itself never enters the loop. The key of point
//  k is k when not ice(k) and -1 otherwise; the inclusive prefix maximum at i - 1 is that largest k, or an index below
//  the series' row[s] (a neighbour's point, or -1), which means none.
//  FILL (qac_ts::_fill_value). Let p be the largest valid index < i and q the smallest valid index > i in the series.
//  The outer walk passes invalid points j in (p, i) first; their t_i - t_j is smaller than t_i - t_p, so the
//  `t - t0 > max_timespan` test returns NaN there only if it also does at p. At p the inner walk passes invalid points
//  k in (i, q) whose t_k - t_p is smaller than t_q - t_p, so again only q can decide. Without a q the inner loop runs
//  out and every earlier j either fails the span test or runs out the same way: NaN. Without a p the outer walk ends
//  in NaN. So the value is NaN when p or q is missing or t_i - t_p or t_q - t_p exceeds max_timespan, and the line
//  through (t_p, x_p), (t_q, x_q) otherwise. p is the prefix maximum of (valid(k) ? k : -1) at i - 1; q comes from the
//  same scan over the mirrored positions r = np - 1 - k, at the mirror of i + 1. Indexes are global and monotone, so
//  the scans need no segment flags: a p below row[s] or a q at or above row[s+1] means none.
//
// Index safety. The host checks before any launch that row[0] == 0 and row is non-decreasing, so row[S] = np points
// were uploaded, that times increase strictly in a series and t_end lies after the last, that pack_of[s] < P and the
// three CSR levels of the packs are non-decreasing and end at the uploaded sizes, and that qrow is a CSR of nq
// queries. A lane's point k (or query j) is < np (< nq) by its grid-stride test; csr_series_of (device/csr_series.h)
// returns the s < S with row[s] <= k < row[s+1], which exists because k < row[S]. RATING's two searches (first_false,
// device/workgroup.h) ask about curves in [c0, c1) and segments in [g0, g1) only; it reads curve it in [c0, c1) after
// the `c0 == c1` test and segment g in [g0, g1) after `g0 == g1`. ICE passes rs_area the n > 0 points of one series (device/ts_area.h
// states its own reads). The scan kernels read key sources at positions < np only and write L at positions < np and
// agg at block indexes < nb; LDS is indexed by the wavefront number < 4 (block_scan, device/workgroup.h). The finish kernels read L[k - 1] only with
// k > row[s] >= 0, the mirrored L at np - 2 - k only with k + 1 < row[s+1] <= np, agg[b - 1] only with b > 0, and
// points p, q, stop only after the tests row[s] <= p, q < row[s+1], row[s] <= stop < k. RECESSION reads point k + 1
// only with k + 1 < row[s+1].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../detmath/detmath.h"
#include "../device/csr_series.h"
#include "../device/ts_area.h"
#include "../device/workgroup.h"
#include "../host/ts_prep.hpp"
#include "../include_internal/device_call.h"
#include "../include_internal/series_args.h"

using namespace shyft_hip_impl;

namespace {

constexpr int TP_BLOCK = 256;                      // 4 wavefronts
constexpr int TP_ITEMS = 4;                        // keys per lane
constexpr int TP_SPAN = TP_BLOCK * TP_ITEMS;       // keys per workgroup of the scan
constexpr int TP_KEY_RECESSION = 0, TP_KEY_FILL = 1, TP_KEY_FILL_MIRROR = 2;

// qac_parameter::is_ok_quality (time_series_dd.h:1463-1471)
__device__ inline bool tp_ok(double x, double min_x, double max_x) {
    if (!rs_finite(x)) return false;
    if (rs_finite(min_x) && x < min_x) return false;
    if (rs_finite(max_x) && x > max_x) return false;
    return true;
}

// ---- rating curve ------------------------------------------------------------------------------------------------------
struct tp_rating_args {
    int64_t np, S;
    const int64_t* row;
    const int64_t* t;
    const double* v;
    const int64_t* pack_of;
    const int64_t* pack_row;
    const int64_t* curve_t;
    const int64_t* curve_row;
    const double* seg;
    double* out;
};

__global__ __launch_bounds__(TP_BLOCK) void tp_rating_kernel(tp_rating_args a) {
    const int64_t stride = int64_t(gridDim.x) * TP_BLOCK;
    for (int64_t k = int64_t(blockIdx.x) * TP_BLOCK + threadIdx.x; k < a.np; k += stride) {
        const int64_t s = csr_series_of(a.row, a.S, k);
        const int64_t p = a.pack_of[s];
        const int64_t c0 = a.pack_row[p], c1 = a.pack_row[p + 1];
        const int64_t tk = a.t[k];
        const double level = a.v[k];
        double r = rs_nan();
        if (c0 != c1) {
            // lower_bound: the first curve with start >= tk
            int64_t it = first_false(c0, c1, [&](int64_t m) { return a.curve_t[m] < tk; });
            bool none = false;
            if (it == c0 && a.curve_t[it] > tk) none = true;
            else if (it == c1 || a.curve_t[it] > tk) --it;
            if (!none) {
                const int64_t g0 = a.curve_row[it], g1 = a.curve_row[it + 1];
                if (g0 != g1) {
                    // lower_bound on `lower < level`
                    const int64_t l2 = first_false(g0, g1, [&](int64_t m) { return a.seg[4 * m] < level; });
                    int64_t g = -1;
                    if (l2 != g1 && level == a.seg[4 * l2]) g = l2;
                    else if (l2 != g0) g = l2 - 1;
                    if (g >= 0) r = a.seg[4 * g + 1] * detmath::pow(level - a.seg[4 * g + 2], a.seg[4 * g + 3]);
                }
            }
        }
        a.out[k] = r;
    }
}

// ---- ice packing -------------------------------------------------------------------------------------------------------
struct tp_ice_args {
    int64_t nq, S;
    const int64_t* row;
    const int64_t* t;
    const double* v;
    const int64_t* t_end;
    const int32_t* fx;
    const int64_t* qrow;
    const int64_t* qt;
    const int64_t* window;
    const double* threshold;
    const int32_t* policy;
    double* out;
};

__global__ __launch_bounds__(TP_BLOCK) void tp_ice_kernel(tp_ice_args a) {
    const int64_t stride = int64_t(gridDim.x) * TP_BLOCK;
    for (int64_t j = int64_t(blockIdx.x) * TP_BLOCK + threadIdx.x; j < a.nq; j += stride) {
        const int64_t s = csr_series_of(a.qrow, a.S, j);
        const int64_t r0 = a.row[s], n = a.row[s + 1] - r0;
        const int64_t tp_start = n > 0 ? a.t[r0] : 0;  // total_period() of an empty series is [0, 0)
        const int32_t policy = a.policy[s];
        const int64_t pe = a.qt[j];
        int64_t ps = pe - a.window[s];
        if (policy != int32_t(shyft_hip::host::DISALLOW_MISSING)) {
            if (ps < tp_start) ps = rs_min(tp_start, pe);
        }
        double r;
        if (pe - ps == 0) {
            r = 0.0;
        } else if (n <= 0) {
            r = rs_nan();
        } else {
            int64_t tsum = 0;
            const double p_sum = rs_area(a.t + r0, a.v + r0, n, a.t_end[s], ps, pe,
                                         a.fx[s] == int32_t(shyft_hip::host::POINT_INSTANT_VALUE), tsum);
            if (!rs_finite(p_sum) || tsum == 0) r = rs_nan();
            else if (policy == int32_t(shyft_hip::host::ALLOW_ANY_MISSING) || tsum == pe - ps)
                r = p_sum / rs_seconds(tsum) < a.threshold[s] ? 1.0 : 0.0;
            else r = rs_nan();
        }
        a.out[j] = r;
    }
}

// ---- the index scan ----------------------------------------------------------------------------------------------------
struct tp_scan_args {
    int kind;
    int64_t np, S, nb;
    const int64_t* row;
    const double* src;    // the indicator (RECESSION) or the values (FILL)
    const double* min_x;  // [S], FILL
    const double* max_x;  // [S], FILL
    int64_t* L;           // [np] running maximum inside each workgroup span
    int64_t* agg;         // [nb] the maximum of each span; after tp_scan_agg_kernel the running maximum over spans
};

__device__ inline int64_t tp_max(int64_t a, int64_t b) { return a > b ? a : b; }

// The scans are inclusive running maxima over the workgroup's lanes in thread order, -1 for none (block_scan,
// device/workgroup.h; every lane of the workgroup calls it).
static_assert(TP_BLOCK == SCAN_BLOCK, "block_scan takes a workgroup of TP_BLOCK lanes");

__global__ __launch_bounds__(TP_BLOCK) void tp_scan_block_kernel(tp_scan_args a) {
    __shared__ int64_t wsum[TP_BLOCK / 64];
    for (int64_t b = blockIdx.x; b < a.nb; b += gridDim.x) {  // uniform over the workgroup
        const int64_t p0 = b * TP_SPAN + int64_t(threadIdx.x) * TP_ITEMS;
        int64_t m[TP_ITEMS];
        int64_t run = -1, s = -1;
#pragma unroll
        for (int u = 0; u < TP_ITEMS; ++u) {
            const int64_t pos = p0 + u;
            int64_t key = -1;
            if (pos < a.np) {
                const int64_t k = a.kind == TP_KEY_FILL_MIRROR ? a.np - 1 - pos : pos;
                const double x = a.src[k];
                if (a.kind == TP_KEY_RECESSION) {
                    if (!(rs_finite(x) && x > 0.5)) key = pos;
                } else {
                    if (s < 0 || k < a.row[s] || k >= a.row[s + 1]) s = csr_series_of(a.row, a.S, k);
                    if (tp_ok(x, a.min_x[s], a.max_x[s])) key = pos;
                }
            }
            run = tp_max(run, key);
            m[u] = run;
        }
        int64_t total;
        const int64_t incl = block_scan(run, op_max(), int64_t(-1), wsum, total);
        // the maximum over the lanes before this one: block_scan leaves the wavefronts' maxima in wsum
        int64_t before = __shfl_up(incl, 1, 64);
        if ((threadIdx.x & 63) == 0) {
            before = -1;
            for (int w = 0; w < int(threadIdx.x >> 6); ++w) before = tp_max(before, wsum[w]);
        }
#pragma unroll
        for (int u = 0; u < TP_ITEMS; ++u)
            if (p0 + u < a.np) a.L[p0 + u] = tp_max(before, m[u]);
        if (threadIdx.x == 0) a.agg[b] = total;
    }
}

// one workgroup: agg[b] becomes the maximum of agg[0 .. b]
__global__ __launch_bounds__(TP_BLOCK) void tp_scan_agg_kernel(int64_t nb, int64_t* agg) {
    __shared__ int64_t wsum[TP_BLOCK / 64];
    int64_t carry = -1;
    for (int64_t b0 = 0; b0 < nb; b0 += TP_BLOCK) {  // uniform over the workgroup
        const int64_t b = b0 + threadIdx.x;
        int64_t total;
        const int64_t incl = block_scan(b < nb ? agg[b] : int64_t(-1), op_max(), int64_t(-1), wsum, total);
        if (b < nb) agg[b] = tp_max(incl, carry);
        carry = tp_max(carry, total);
    }
}

// the running maximum at position pos < np, over all positions 0 .. pos
__device__ inline int64_t tp_scanned(const int64_t* __restrict__ L, const int64_t* __restrict__ agg, int64_t pos) {
    const int64_t b = pos / TP_SPAN;
    const int64_t x = L[pos];
    return b > 0 ? tp_max(x, agg[b - 1]) : x;
}

struct tp_rec_args {
    int64_t np, S;
    const int64_t* row;
    const int64_t* t;
    const double* v;
    const int32_t* fx;
    const double* ice;
    const double* alpha;
    const double* qmin;
    const int64_t* L;
    const int64_t* agg;
    double* out;
};

__global__ __launch_bounds__(TP_BLOCK) void tp_rec_finish_kernel(tp_rec_args a) {
    const int64_t stride = int64_t(gridDim.x) * TP_BLOCK;
    for (int64_t k = int64_t(blockIdx.x) * TP_BLOCK + threadIdx.x; k < a.np; k += stride) {
        const int64_t s = csr_series_of(a.row, a.S, k);
        const int64_t r0 = a.row[s], r1 = a.row[s + 1];
        const double ice = a.ice[k];
        double r;
        if (!rs_finite(ice)) {
            r = rs_nan();
        } else if (ice > 0.5) {
            int64_t stop = r0;
            bool lost = false;
            if (k > r0) {
                const int64_t j = tp_scanned(a.L, a.agg, k - 1);
                if (j >= r0) {
                    stop = j;
                    lost = !rs_finite(a.ice[j]);
                }
            }
            if (lost) {
                r = rs_nan();
            } else {
                const double qs = a.v[stop];
                const int64_t ts = a.t[stop];
                const double qbf = a.qmin[s];
                const double alpha = a.alpha[s];
                r = qbf + (qs - qbf) * detmath::exp(-alpha * rs_seconds(a.t[k] - ts));
            }
        } else {  // flow_ts(t) at its own point k (point_ts::operator(), host/time_series.hpp)
            if (a.fx[s] == int32_t(shyft_hip::host::POINT_INSTANT_VALUE) && k + 1 < r1) {
                const double sl = (a.v[k + 1] - a.v[k]) / rs_seconds(a.t[k + 1] - a.t[k]);
                r = a.v[k] + sl * rs_seconds(a.t[k] - a.t[k]);
            } else {
                r = a.v[k];
            }
        }
        a.out[k] = r;
    }
}

struct tp_fill_args {
    int64_t np, S;
    const int64_t* row;
    const int64_t* t;
    const double* v;
    const double* min_x;
    const double* max_x;
    const int64_t* max_timespan;
    const int64_t* Lp;
    const int64_t* aggp;
    const int64_t* Lq;
    const int64_t* aggq;
    double* out;
};

__global__ __launch_bounds__(TP_BLOCK) void tp_fill_finish_kernel(tp_fill_args a) {
    const int64_t stride = int64_t(gridDim.x) * TP_BLOCK;
    for (int64_t k = int64_t(blockIdx.x) * TP_BLOCK + threadIdx.x; k < a.np; k += stride) {
        const int64_t s = csr_series_of(a.row, a.S, k);
        const int64_t r0 = a.row[s], r1 = a.row[s + 1];
        const double x = a.v[k];
        double r = rs_nan();
        if (tp_ok(x, a.min_x[s], a.max_x[s])) {
            r = x;
        } else {
            const int64_t span = a.max_timespan[s];
            if (!(k == r0 || k + 1 >= r1 || span == 0)) {
                const int64_t tk = a.t[k];
                const int64_t p = tp_scanned(a.Lp, a.aggp, k - 1);
                if (p >= r0 && !(tk - a.t[p] > span)) {
                    const int64_t mq = tp_scanned(a.Lq, a.aggq, a.np - 2 - k);  // the mirror of k + 1
                    const int64_t q = mq < 0 ? a.np : a.np - 1 - mq;
                    if (q < r1) {
                        const int64_t t0 = a.t[p], t1 = a.t[q];
                        if (!(t1 - t0 > span)) {
                            const double x0 = a.v[p], x1 = a.v[q];
                            const double sl = (x1 - x0) / rs_seconds(t1 - t0);
                            const double ic = x0 - sl * rs_seconds(t0);
                            r = sl * rs_seconds(tk) + ic;
                        }
                    }
                }
            }
        }
        a.out[k] = r;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// The argument checks of the series, shared by the device and the host entries (include_internal/series_args.h); true
// when there is nothing to do.
bool tp_prepare(const char* who, size_t S, const int64_t* row, const int64_t* t, const double* v, const int64_t* t_end,
                const int32_t* fx) {
    if (S == 0) return true;
    check_point_series(who, "tsprep", S, row, t, v, t_end, fx);
    return false;
}

// rating: the packs' CSR, pack_of, and the reference's "no rating-curve segments" for a curve without segments that a
// point of a series would use (rating_curve_function::flow throws when it is asked, time_series.h:1396-1397)
void tp_prepare_rating(size_t S, const int64_t* row, const int64_t* t, size_t P, const int64_t* pack_row,
                       const int64_t* curve_t, const int64_t* curve_row, const double* seg, const int64_t* pack_of) {
    if (!pack_of) throw std::runtime_error("shyft_hip_ts_rating_curve: null argument");
    if (P == 0) throw std::runtime_error("rating_curve: at least one parameter pack is needed");
    if (!pack_row || !curve_row) throw std::runtime_error("shyft_hip_ts_rating_curve: null argument");
    if (pack_row[0] != 0 || curve_row[0] != 0) throw std::runtime_error("rating_curve: pack_row[0] and curve_row[0] must be 0");
    for (size_t p = 0; p < P; ++p)
        if (pack_row[p + 1] < pack_row[p]) throw std::runtime_error("rating_curve: pack_row must not decrease");
    const int64_t C = pack_row[P];
    if (C > 0 && !curve_t) throw std::runtime_error("shyft_hip_ts_rating_curve: null argument");
    for (int64_t c = 0; c < C; ++c)
        if (curve_row[c + 1] < curve_row[c]) throw std::runtime_error("rating_curve: curve_row must not decrease");
    if (curve_row[C] > 0 && !seg) throw std::runtime_error("shyft_hip_ts_rating_curve: null argument");
    for (size_t p = 0; p < P; ++p)
        for (int64_t c = pack_row[p] + 1; c < pack_row[p + 1]; ++c)
            if (!(curve_t[c - 1] < curve_t[c])) throw std::runtime_error("rating_curve: the curve times of a pack must increase");
    for (int64_t c = 0; c < C; ++c)
        for (int64_t g = curve_row[c] + 1; g < curve_row[c + 1]; ++g)
            if (!(seg[4 * (g - 1)] <= seg[4 * g]))
                throw std::runtime_error("rating_curve: the segments of a curve must be sorted on lower");
    for (size_t s = 0; s < S; ++s) {
        if (pack_of[s] < 0 || size_t(pack_of[s]) >= P) throw std::runtime_error("rating_curve: pack_of is out of range");
        const int64_t b = row[s], e = row[s + 1];
        if (b == e) continue;
        const int64_t c0 = pack_row[pack_of[s]], c1 = pack_row[pack_of[s] + 1];
        for (int64_t c = c0; c < c1; ++c) {
            if (curve_row[c] != curve_row[c + 1]) continue;
            // curve c serves the points with curve_t[c] <= time < curve_t[c + 1] (the last one all later points)
            const int64_t* lo = std::lower_bound(t + b, t + e, curve_t[c]);
            if (lo != t + e && (c + 1 == c1 || *lo < curve_t[c + 1])) throw std::runtime_error("no rating-curve segments");
        }
    }
}

void tp_prepare_ice(size_t S, const int64_t* row, const int64_t* t, const int64_t* qrow, const int64_t* qt,
                    const int64_t* window, const double* threshold, const int32_t* policy) {
    if (!qrow || !window || !threshold || !policy) throw std::runtime_error("shyft_hip_ts_ice_packing: null argument");
    check_csr_rows("tsprep", S, qrow);
    if (qrow[S] > 0 && !qt) throw std::runtime_error("shyft_hip_ts_ice_packing: null argument");
    const int64_t i64max = std::numeric_limits<int64_t>::max(), i64min = std::numeric_limits<int64_t>::min();
    for (size_t s = 0; s < S; ++s) {
        if (policy[s] < 0 || policy[s] > 2)
            throw std::runtime_error("ice_packing: policy must be DISALLOW_MISSING, ALLOW_INITIAL_MISSING or ALLOW_ANY_MISSING");
        if (window[s] < 0 || window[s] > i64max / 4)
            throw std::runtime_error("ice_packing: the window must lie in 0 .. a quarter of the 64-bit range");
        for (int64_t j = qrow[s]; j < qrow[s + 1]; ++j) {
            if (qt[j] < i64min / 4 || qt[j] > i64max / 4)
                throw std::runtime_error("tsprep: times beyond a quarter of the 64-bit range are not supported");
            // accumulate_value reads point 1 of a one-point series when the point lies inside a period that starts
            // before it; the reference throws out of point_dt::time (core/time_axis.h:317-322). The clipping policies
            // start the period at the point.
            if (row[s + 1] - row[s] == 1 && policy[s] == int32_t(shyft_hip::host::DISALLOW_MISSING) &&
                qt[j] - window[s] < t[row[s]] && t[row[s]] < qt[j])
                throw std::runtime_error("point_dt.time(i): a one-point series cannot be integrated over a period "
                                         "that starts before its point and holds it");
        }
    }
}

void tp_prepare_recession(size_t S, const int64_t* row, const int64_t* t, const int64_t* t_end, const double* ice,
                          const int64_t* ice_start, const int64_t* ice_end, const double* alpha, const double* qmin) {
    namespace h = shyft_hip::host;
    if (!ice_start || !ice_end || !alpha || !qmin || (row[S] > 0 && !ice))
        throw std::runtime_error("shyft_hip_ts_ice_packing_recession: null argument");
    for (size_t s = 0; s < S; ++s)
        if (row[s + 1] > row[s])  // evaluate() checks when a point is asked for
            h::ensure_overlap(h::utcperiod(ice_start[s], ice_end[s]), h::utcperiod(t[row[s]], t_end[s]));
}

call_record g_tp;
constexpr const char* TP_UPLOAD = "tsprep upload";

// one lane per job; the grid-stride loops take what the grid does not
unsigned tp_grid(size_t jobs) { return launch_blocks((jobs + TP_BLOCK - 1) / TP_BLOCK); }

// the two scan launches of one key kind; L [np] and agg [nb] are allocated here
void tp_scan(device_call& c, int kind, int64_t np, int64_t S, const int64_t* d_row, const double* d_src,
             const double* d_min, const double* d_max, dbuf<int64_t>& L, dbuf<int64_t>& agg) {
    const int64_t nb = (np + TP_SPAN - 1) / TP_SPAN;
    L.alloc(size_t(np));
    agg.alloc(size_t(nb));
    tp_scan_args a{};
    a.kind = kind;
    a.np = np;
    a.S = S;
    a.nb = nb;
    a.row = d_row;
    a.src = d_src;
    a.min_x = d_min;
    a.max_x = d_max;
    a.L = L.p;
    a.agg = agg.p;
    hipLaunchKernelGGL(tp_scan_block_kernel, dim3(launch_blocks(size_t(nb))), dim3(TP_BLOCK), 0, c.s, a);
    hip_check(hipGetLastError(), "tsprep scan");
    hipLaunchKernelGGL(tp_scan_agg_kernel, dim3(1), dim3(TP_BLOCK), 0, c.s, nb, agg.p);
    hip_check(hipGetLastError(), "tsprep scan of the aggregates");
}

}  // namespace

extern "C" {

int shyft_hip_ts_rating_curve(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                              const int64_t* t_end, const int32_t* fx, size_t P, const int64_t* pack_row,
                              const int64_t* curve_t, const int64_t* curve_row, const double* seg, const int64_t* pack_of,
                              double* out) {
    try {
        if (tp_prepare("shyft_hip_ts_rating_curve", S, row, t, v, t_end, fx) || row[S] == 0) return 0;
        if (!out) throw std::runtime_error("shyft_hip_ts_rating_curve: null argument");
        tp_prepare_rating(S, row, t, P, pack_row, curve_t, curve_row, seg, pack_of);
        device_call c(device);
        const size_t np = size_t(row[S]), C = size_t(pack_row[P]), G = size_t(curve_row[C]);
        dbuf<int64_t> d_row, d_t, d_pack_of, d_pack_row, d_curve_t, d_curve_row;
        dbuf<double> d_v, d_seg, d_out;
        c.upload(d_row, row, S + 1, TP_UPLOAD);
        c.upload(d_t, t, np, TP_UPLOAD);
        c.upload(d_v, v, np, TP_UPLOAD);
        c.upload(d_pack_of, pack_of, S, TP_UPLOAD);
        c.upload(d_pack_row, pack_row, P + 1, TP_UPLOAD);
        c.upload(d_curve_t, curve_t, C, TP_UPLOAD);
        c.upload(d_curve_row, curve_row, C + 1, TP_UPLOAD);
        c.upload(d_seg, seg, 4 * G, TP_UPLOAD);
        d_out.alloc(np);
        tp_rating_args a{int64_t(np), int64_t(S), d_row.p, d_t.p, d_v.p, d_pack_of.p, d_pack_row.p, d_curve_t.p,
                         d_curve_row.p, d_seg.p, d_out.p};
        c.begin();
        hipLaunchKernelGGL(tp_rating_kernel, dim3(tp_grid(np)), dim3(TP_BLOCK), 0, c.s, a);
        hip_check(hipGetLastError(), "tsprep rating");
        g_tp.finish(c, "tsprep", out, d_out.p, np);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_rating_curve_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                   const int64_t* t_end, const int32_t* fx, size_t P, const int64_t* pack_row,
                                   const int64_t* curve_t, const int64_t* curve_row, const double* seg,
                                   const int64_t* pack_of, double* out) {
    namespace h = shyft_hip::host;
    (void)device;
    try {
        if (tp_prepare("shyft_hip_ts_rating_curve_host", S, row, t, v, t_end, fx) || row[S] == 0) return 0;
        if (!out) throw std::runtime_error("shyft_hip_ts_rating_curve_host: null argument");
        tp_prepare_rating(S, row, t, P, pack_row, curve_t, curve_row, seg, pack_of);
        std::vector<h::rating_curve_parameters> packs(P);
        for (size_t p = 0; p < P; ++p)
            for (int64_t c = pack_row[p]; c < pack_row[p + 1]; ++c) {
                std::vector<h::rating_curve_segment> segs;
                for (int64_t g = curve_row[c]; g < curve_row[c + 1]; ++g)
                    segs.emplace_back(seg[4 * g], seg[4 * g + 1], seg[4 * g + 2], seg[4 * g + 3]);
                h::rating_curve_function f;
                f.segments = std::move(segs);  // sorted already (checked), equal lowers keep their order
                packs[p].add_curve(curve_t[c], f);
            }
        for (size_t s = 0; s < S; ++s) {
            const h::point_ts level = point_series(s, row, t, v, t_end, fx);
            const std::vector<double> r = h::rating_curve_values(level, packs[pack_of[s]]);
            std::copy(r.begin(), r.end(), out + row[s]);
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_ice_packing(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, const int64_t* qrow, const int64_t* qt,
                             const int64_t* window, const double* threshold, const int32_t* policy, double* out) {
    try {
        if (tp_prepare("shyft_hip_ts_ice_packing", S, row, t, v, t_end, fx)) return 0;
        tp_prepare_ice(S, row, t, qrow, qt, window, threshold, policy);
        if (qrow[S] == 0) return 0;
        if (!out) throw std::runtime_error("shyft_hip_ts_ice_packing: null argument");
        device_call c(device);
        const size_t np = size_t(row[S]), nq = size_t(qrow[S]);
        dbuf<int64_t> d_row, d_t, d_tend, d_qrow, d_qt, d_window;
        dbuf<double> d_v, d_thr, d_out;
        dbuf<int32_t> d_fx, d_policy;
        c.upload(d_row, row, S + 1, TP_UPLOAD);
        c.upload(d_t, t, np, TP_UPLOAD);
        c.upload(d_v, v, np, TP_UPLOAD);
        c.upload(d_tend, t_end, S, TP_UPLOAD);
        c.upload(d_fx, fx, S, TP_UPLOAD);
        c.upload(d_qrow, qrow, S + 1, TP_UPLOAD);
        c.upload(d_qt, qt, nq, TP_UPLOAD);
        c.upload(d_window, window, S, TP_UPLOAD);
        c.upload(d_thr, threshold, S, TP_UPLOAD);
        c.upload(d_policy, policy, S, TP_UPLOAD);
        d_out.alloc(nq);
        tp_ice_args a{int64_t(nq), int64_t(S), d_row.p, d_t.p, d_v.p, d_tend.p, d_fx.p, d_qrow.p, d_qt.p, d_window.p,
                      d_thr.p, d_policy.p, d_out.p};
        c.begin();
        hipLaunchKernelGGL(tp_ice_kernel, dim3(tp_grid(nq)), dim3(TP_BLOCK), 0, c.s, a);
        hip_check(hipGetLastError(), "tsprep ice packing");
        g_tp.finish(c, "tsprep", out, d_out.p, nq);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_ice_packing_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                  const int64_t* t_end, const int32_t* fx, const int64_t* qrow, const int64_t* qt,
                                  const int64_t* window, const double* threshold, const int32_t* policy, double* out) {
    namespace h = shyft_hip::host;
    (void)device;
    try {
        if (tp_prepare("shyft_hip_ts_ice_packing_host", S, row, t, v, t_end, fx)) return 0;
        tp_prepare_ice(S, row, t, qrow, qt, window, threshold, policy);
        if (qrow[S] == 0) return 0;
        if (!out) throw std::runtime_error("shyft_hip_ts_ice_packing_host: null argument");
        for (size_t s = 0; s < S; ++s) {
            const h::point_ts temp = point_series(s, row, t, v, t_end, fx);
            const h::ice_packing_parameters ip{window[s], threshold[s]};
            for (int64_t j = qrow[s]; j < qrow[s + 1]; ++j)
                out[j] = h::detect_ice_packing(temp, ip, h::ice_packing_temperature_policy(policy[s]), qt[j]);
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_ice_packing_recession(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                       const int64_t* t_end, const int32_t* fx, const double* ice,
                                       const int64_t* ice_start, const int64_t* ice_end, const double* alpha,
                                       const double* recession_minimum, double* out) {
    try {
        if (tp_prepare("shyft_hip_ts_ice_packing_recession", S, row, t, v, t_end, fx) || row[S] == 0) return 0;
        if (!out) throw std::runtime_error("shyft_hip_ts_ice_packing_recession: null argument");
        tp_prepare_recession(S, row, t, t_end, ice, ice_start, ice_end, alpha, recession_minimum);
        device_call c(device);
        const size_t np = size_t(row[S]);
        dbuf<int64_t> d_row, d_t, L, agg;
        dbuf<double> d_v, d_ice, d_alpha, d_qmin, d_out;
        dbuf<int32_t> d_fx;
        c.upload(d_row, row, S + 1, TP_UPLOAD);
        c.upload(d_t, t, np, TP_UPLOAD);
        c.upload(d_v, v, np, TP_UPLOAD);
        c.upload(d_fx, fx, S, TP_UPLOAD);
        c.upload(d_ice, ice, np, TP_UPLOAD);
        c.upload(d_alpha, alpha, S, TP_UPLOAD);
        c.upload(d_qmin, recession_minimum, S, TP_UPLOAD);
        d_out.alloc(np);
        c.begin();
        tp_scan(c, TP_KEY_RECESSION, int64_t(np), int64_t(S), d_row.p, d_ice.p, nullptr, nullptr, L, agg);
        tp_rec_args a{int64_t(np), int64_t(S), d_row.p, d_t.p, d_v.p, d_fx.p, d_ice.p, d_alpha.p, d_qmin.p, L.p, agg.p,
                      d_out.p};
        hipLaunchKernelGGL(tp_rec_finish_kernel, dim3(tp_grid(np)), dim3(TP_BLOCK), 0, c.s, a);
        hip_check(hipGetLastError(), "tsprep recession");
        g_tp.finish(c, "tsprep", out, d_out.p, np);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_ice_packing_recession_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                            const int64_t* t_end, const int32_t* fx, const double* ice,
                                            const int64_t* ice_start, const int64_t* ice_end, const double* alpha,
                                            const double* recession_minimum, double* out) {
    namespace h = shyft_hip::host;
    (void)device;
    try {
        if (tp_prepare("shyft_hip_ts_ice_packing_recession_host", S, row, t, v, t_end, fx) || row[S] == 0) return 0;
        if (!out) throw std::runtime_error("shyft_hip_ts_ice_packing_recession_host: null argument");
        tp_prepare_recession(S, row, t, t_end, ice, ice_start, ice_end, alpha, recession_minimum);
        for (size_t s = 0; s < S; ++s) {
            const h::point_ts flow = point_series(s, row, t, v, t_end, fx);
            const std::vector<double> ice_at(ice + row[s], ice + row[s + 1]);
            const h::ice_packing_recession_parameters ipr{alpha[s], recession_minimum[s]};
            for (size_t i = 0; i < flow.size(); ++i) out[row[s] + int64_t(i)] = h::ice_packing_recession_value(flow, ice_at, ipr, i);
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_min_max_fill(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                              const int64_t* t_end, const int32_t* fx, const double* min_x, const double* max_x,
                              const int64_t* max_timespan, double* out) {
    try {
        if (tp_prepare("shyft_hip_ts_min_max_fill", S, row, t, v, t_end, fx) || row[S] == 0) return 0;
        if (!out || !min_x || !max_x || !max_timespan) throw std::runtime_error("shyft_hip_ts_min_max_fill: null argument");
        device_call c(device);
        const size_t np = size_t(row[S]);
        dbuf<int64_t> d_row, d_t, d_span, Lp, aggp, Lq, aggq;
        dbuf<double> d_v, d_min, d_max, d_out;
        c.upload(d_row, row, S + 1, TP_UPLOAD);
        c.upload(d_t, t, np, TP_UPLOAD);
        c.upload(d_v, v, np, TP_UPLOAD);
        c.upload(d_min, min_x, S, TP_UPLOAD);
        c.upload(d_max, max_x, S, TP_UPLOAD);
        c.upload(d_span, max_timespan, S, TP_UPLOAD);
        d_out.alloc(np);
        c.begin();
        tp_scan(c, TP_KEY_FILL, int64_t(np), int64_t(S), d_row.p, d_v.p, d_min.p, d_max.p, Lp, aggp);
        tp_scan(c, TP_KEY_FILL_MIRROR, int64_t(np), int64_t(S), d_row.p, d_v.p, d_min.p, d_max.p, Lq, aggq);
        tp_fill_args a{int64_t(np), int64_t(S), d_row.p, d_t.p, d_v.p, d_min.p, d_max.p, d_span.p, Lp.p, aggp.p, Lq.p,
                       aggq.p, d_out.p};
        hipLaunchKernelGGL(tp_fill_finish_kernel, dim3(tp_grid(np)), dim3(TP_BLOCK), 0, c.s, a);
        hip_check(hipGetLastError(), "tsprep fill");
        g_tp.finish(c, "tsprep", out, d_out.p, np);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_min_max_fill_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                   const int64_t* t_end, const int32_t* fx, const double* min_x, const double* max_x,
                                   const int64_t* max_timespan, double* out) {
    namespace h = shyft_hip::host;
    (void)device;
    try {
        if (tp_prepare("shyft_hip_ts_min_max_fill_host", S, row, t, v, t_end, fx) || row[S] == 0) return 0;
        if (!out || !min_x || !max_x || !max_timespan)
            throw std::runtime_error("shyft_hip_ts_min_max_fill_host: null argument");
        for (size_t s = 0; s < S; ++s) {
            const h::point_ts ts = point_series(s, row, t, v, t_end, fx);
            h::qac_parameter p;
            p.max_timespan = max_timespan[s];
            p.min_x = min_x[s];
            p.max_x = max_x[s];
            for (size_t i = 0; i < ts.size(); ++i) out[row[s] + int64_t(i)] = h::qac_value(ts, p, i);
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

double shyft_hip_tsprep_last_ms(int device) { return g_tp.last_ms.load(device, 0.0); }

uint64_t shyft_hip_tsprep_calls(int device) { return g_tp.calls.load(device, 0); }

}  // extern "C"
