// Percentiles of a vector of point series on a fixed_dt axis: calculate_percentiles with skip_nans = true
// (core/time_series_statistics.h:184-246), restated for S views of R stored series. The definition of correct for
// kernels/ts_percentiles.hip; shyft_hip_ts_percentiles_host runs these statements.
//
// A view is (src, shift): stored series src seen `shift` microseconds later, every point time and t_end moved by
// shift (time_shift_ts, core/time_series_dd.h:707-751). Several views may share one stored series, so the partitions
// of one long record (partition_by, core/time_series.h:2451-2494) are stored once.
//
//  samples     average_accessor::value(i) of every view (average_values / accumulate_value of time_series.hpp), the
//              non-finite ones dropped, the rest fully sorted (:199-207, :115-124).
//  0..100      R7 with the eps = 1e-30 rules (:133-153), through pct_make_plan of device/pct_plan.h.
//  -1          the sum of the sorted samples, added in that order, over their count (:127-132).
//  -1000/+1000 not order statistics of the averages: extract_statistic_from_vector with nan_min / nan_max (:24-90,
//              :221-226), the fold over the raw point values whose times lie inside each interval, across all views.
//  other       NaN, as is every entry of an interval without a finite sample.
//
// The average of a stair-case view is taken of the stored series over the period moved back by shift: accumulate_value
// compares times and takes to_seconds of differences only on that branch, so the bits are those of the moved series.
// The linear branch takes to_seconds of absolute times (r.t, px.start + px.end), so a linear view with a shift is
// averaged over a moved copy of its series.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../device/pct_plan.h"
#include "time_series.hpp"

namespace shyft_hip::host {

// nan_max / nan_min (time_series_statistics.h:24-39): the fold ignores non-finite values
inline double nan_max(double r, double x) {
    if (!std::isfinite(x)) return r;
    if (!std::isfinite(r)) return x;
    return std::max(r, x);
}
inline double nan_min(double r, double x) {
    if (!std::isfinite(x)) return r;
    if (!std::isfinite(r)) return x;
    return std::min(r, x);
}

// a stored series seen `shift` later
struct shifted_view {
    const point_ts* src;
    utctimespan shift;
    size_t size() const { return src->size(); }
    utctime time(size_t i) const { return src->t[i] + shift; }
    double value(size_t i) const { return src->v[i]; }
    size_t index_of(utctime tx) const { return host::index_of(*src, tx - shift); }
};

// extract_statistics (time_series_statistics.h:41-75), statement by statement; added to r by fx, interval by
// interval, as extract_statistic_from_vector does with the vector of each series (:77-90). A series without points
// gives NaN everywhere (the reference would ask it for time(0)).
template <class Fx>
inline void extract_statistics_into(const shifted_view& ts, const fixed_dt& ta, Fx&& fx, bool first,
                                    std::vector<double>& v_x) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t is_max = ts.size();
    size_t is = ta.size() ? ts.index_of(ta.time(0)) : npos;  // ix_map.src_index(0)
    for (size_t i = 0; i < ta.size(); ++i) {
        const utcperiod p = ta.period(i);
        double rv = nan;
        bool emit_now = false;
        if (is == npos) {  // in the beginning of the axis: nothing yet
            if (is_max && p.contains(ts.time(0))) is = 0;
            else emit_now = true;
        }
        if (!emit_now) {
            if (is < is_max && ts.time(is) < p.start) ++is;  // the point left of the interval
            while (is < is_max && ts.time(is) < p.end) {
                rv = fx(rv, ts.value(is));
                ++is;
            }
        }
        v_x[i] = first ? rv : fx(v_x[i], rv);
    }
}

// calculate_percentiles_excel_method_full_sort for one entry over the sorted finite samples (:115-160)
inline double percentile_of_sorted(const std::vector<double>& samples, int64_t p) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const pct_plan q = pct_make_plan(p, int(samples.size()));
    if (q.kind == PCT_AVG) {
        double sum = 0;
        for (double x : samples) sum += x;
        return sum / int(samples.size());
    }
    if (q.kind == PCT_SINGLE) return samples[q.lo];
    if (q.kind == PCT_LERP) {
        const double lower = samples[q.lo], upper = samples[q.hi];
        return lower + q.delta * (upper - lower);
    }
    return nan;
}

// The points [first, last) of a stored series that the views of it can read when every period start and end, taken
// back by the views' shifts, lies in [lo, hi]: from the last point at or before lo (the one index_of and
// open_range_index_of of the earliest start give) up to and including the first point at or after hi (where
// accumulate_value's walk of the latest period ends: its `r.t >= p.end` test and its end-of-points test add the same
// nothing there, and the extremes' `time(is) < p.end` is false). A series that keeps its first point behaves as
// before a start before it, one that keeps its last with t_end unchanged as before at and after its end. Two points
// are kept where the series has two, so the one-point rule sees what it saw. A vector of long records on a short
// axis is then copied and uploaded in the axis' window only.
inline std::pair<size_t, size_t> view_window(const point_ts& ts, utctime lo, utctime hi) {
    const size_t n = ts.size();
    if (n <= 2 || lo > hi) return {0, n};
    size_t first = size_t(std::upper_bound(ts.t.begin(), ts.t.end(), lo) - ts.t.begin());
    first = first ? first - 1 : 0;
    size_t last = size_t(std::lower_bound(ts.t.begin(), ts.t.end(), hi) - ts.t.begin());
    last = last < n ? last + 1 : n;
    if (last < first + 2) {
        if (first + 2 <= n) last = first + 2;
        else first = last - 2;
    }
    return {first, last};
}

// The checks of the views, after those of the R stored series in CSR form: src in range, the moved series inside a
// quarter of the 64-bit range, and the one-point rule of shyft_hip_resample on the moved periods.
inline void check_views(size_t R, const int64_t* row, const int64_t* t, const int64_t* t_end, size_t S, const int32_t* src,
                        const int64_t* shift, const fixed_dt& ta) {
    const int64_t q_max = std::numeric_limits<int64_t>::max() / 4, q_min = std::numeric_limits<int64_t>::min() / 4;
    const utctime ta_end = ta.t + utctimespan(ta.n) * ta.dt;
    for (size_t s = 0; s < S; ++s) {
        if (src[s] < 0 || size_t(src[s]) >= R)
            throw std::runtime_error("ts_percentiles: view " + std::to_string(s) + " has src " + std::to_string(src[s]) +
                                     " outside the " + std::to_string(R) + " series");
        const int64_t b = row[src[s]], e = row[src[s] + 1];
        if (b == e) continue;
        if (shift[s] > q_max || shift[s] < q_min || t[b] + shift[s] < q_min || t_end[src[s]] + shift[s] > q_max ||
            ta.t < q_min || ta_end > q_max)
            throw std::runtime_error("ts_percentiles: times beyond a quarter of the 64-bit range are not supported");
        if (e - b == 1) {
            // accumulate_value reads point 1 of a one-point series when the point lies inside a period that starts
            // before it; the reference throws out of point_dt::time (core/time_axis.h:317-322)
            const utctime t0 = t[b] + shift[s];
            if (t0 > ta.t && t0 < ta_end && (t0 - ta.t) % ta.dt != 0)
                throw std::runtime_error("point_dt.time(i): a one-point series cannot be integrated over a period "
                                         "that starts before its point and holds it");
        }
    }
}

// out [n_pct][T]. rows are the R stored series, already checked; ta.dt > 0.
inline void ts_percentiles(const std::vector<point_ts>& rows, size_t S, const int32_t* src, const int64_t* shift,
                           const fixed_dt& ta, const int64_t* pct, size_t n_pct, double* out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t T = ta.size();
    if (T == 0 || n_pct == 0) return;
    bool any_avg = false, any_min = false, any_max = false;
    for (size_t k = 0; k < n_pct; ++k) {
        if (pct[k] == -1000) any_min = true;
        else if (pct[k] == 1000) any_max = true;
        else any_avg = true;
    }
    std::vector<double> table;  // [T][S] the sample of every (interval, view)
    if (any_avg) {
        table.resize(T * S);
        point_ts moved;
        for (size_t s = 0; s < S; ++s) {
            const point_ts& stored = rows[size_t(src[s])];
            std::vector<double> r;
            if (shift[s] != 0 && stored.fx == POINT_INSTANT_VALUE) {
                moved = stored;
                for (auto& x : moved.t) x += shift[s];
                moved.t_end += shift[s];
                r = average_values(moved, ta);
            } else {
                r = average_values(stored, fixed_dt(ta.t - shift[s], ta.dt, T));
            }
            for (size_t i = 0; i < T; ++i) table[i * S + s] = r[i];
        }
    }
    std::vector<double> v_min, v_max;
    for (int hi = 0; hi < 2; ++hi) {
        if (!(hi ? any_max : any_min)) continue;
        std::vector<double>& v_x = hi ? v_max : v_min;
        v_x.assign(T, nan);  // no view at all: NaN
        for (size_t s = 0; s < S; ++s) {
            const shifted_view view{&rows[size_t(src[s])], shift[s]};
            if (hi) extract_statistics_into(view, ta, nan_max, s == 0, v_x);
            else extract_statistics_into(view, ta, nan_min, s == 0, v_x);
        }
    }
    std::vector<double> samples;
    samples.reserve(S);
    for (size_t i = 0; i < T; ++i) {
        if (any_avg) {
            samples.clear();
            for (size_t s = 0; s < S; ++s)
                if (std::isfinite(table[i * S + s])) samples.push_back(table[i * S + s]);
            std::sort(samples.begin(), samples.end());
        }
        for (size_t k = 0; k < n_pct; ++k) {
            if (pct[k] == -1000) out[k * T + i] = v_min[i];
            else if (pct[k] == 1000) out[k * T + i] = v_max[i];
            else out[k * T + i] = percentile_of_sorted(samples, pct[k]);
        }
    }
}

}  // namespace shyft_hip::host
