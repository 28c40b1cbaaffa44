// Host restatements of the observation-preparation series of the reference, statement by statement, on
// host::point_ts (C++17, no device code). They are the definition of correct for kernels/tsprep.hip, whose device
// entries are bit-identical to them; the _host entries of the C ABI run these on one thread.
//
//  rating_curve_segment / _function / _parameters, rating_curve_values   core/time_series.h:1255-1546, 1603, 1641-1644
//  ice_packing_parameters, ice_packing_temperature_policy, ice_packing   core/time_series.h:1653-1831
//  ice_packing_recession_parameters, ice_packing_recession               core/time_series_dd.h:1186-1365
//  qac_parameter, min_max_check_linear_fill (qac_ts::value, _fill_value) core/time_series_dd.h:1456-1478,
//                                                                        core/time_series_dd.cpp:1335-1376
// exp and pow are detmath::exp and detmath::pow, as everywhere else in the engine.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../../detmath/detmath.h"
#include "time_series.hpp"

namespace shyft_hip::host {

// ---- rating curve (time_series.h:1255-1546) ---------------------------------------------------------------------------
struct rating_curve_segment {
    double lower = 0.0, a = 0.0, b = 0.0, c = 0.0;
    rating_curve_segment() = default;
    rating_curve_segment(double lower_, double a_, double b_, double c_) : lower(lower_), a(a_), b(b_), c(c_) {}
    bool valid(double level) const { return lower <= level; }                        // :1280-1282
    double flow(double level) const { return a * detmath::pow(level - b, c); }        // :1291-1293
    bool operator<(const rating_curve_segment& o) const { return lower < o.lower; }  // :1318-1320
    bool operator<(double value) const { return lower < value; }                     // :1323-1325
};

struct rating_curve_function {
    std::vector<rating_curve_segment> segments;  // sorted ascending on lower
    rating_curve_function() = default;
    // :1335-1340; std::sort leaves the order of two segments with equal lower unspecified, so such a list is refused
    explicit rating_curve_function(std::vector<rating_curve_segment> segment_vector, bool sorted = false)
        : segments(std::move(segment_vector)) {
        if (!sorted) {
            std::sort(segments.begin(), segments.end());
            for (size_t i = 1; i < segments.size(); ++i)
                if (segments[i - 1].lower == segments[i].lower)
                    throw std::runtime_error("rating_curve_function: two segments with equal lower in an unsorted list");
        }
    }
    size_t size() const { return segments.size(); }
    void add_segment(const rating_curve_segment& seg) {  // :1389-1391
        segments.emplace(std::upper_bound(segments.begin(), segments.end(), seg), seg);
    }
    void add_segment(double lower, double a, double b, double c) { add_segment(rating_curve_segment(lower, a, b, c)); }
    double flow(const double level) const {  // :1395-1408
        if (segments.size() == 0) throw std::runtime_error("no rating-curve segments");
        auto it = std::lower_bound(segments.cbegin(), segments.cend(), level);
        if (it != segments.cend() && level == it->lower) {
            return it->flow(level);
        } else if (it != segments.cbegin()) {  // not at beginning -> compute with the previous segment
            return (it - 1)->flow(level);
        } else {  // before the first segment -> no flow
            return std::numeric_limits<double>::quiet_NaN();
        }
    }
};

struct rating_curve_parameters {
    std::vector<std::pair<utctime, rating_curve_function>> curves;  // the reference's std::map: unique, ascending t
    void add_curve(utctime t, const rating_curve_function& rcf) {   // std::map::emplace keeps an existing key (:1483-1490)
        auto it = std::lower_bound(curves.begin(), curves.end(), t,
                                   [](const std::pair<utctime, rating_curve_function>& l, utctime r) { return l.first < r; });
        if (it != curves.end() && it->first == t) return;
        curves.emplace(it, t, rcf);
    }
    double flow(utctime t, double level) const {  // :1493-1506
        // the reference dereferences cbegin() of an empty map here; the rule of :1511 for no curves is NaN
        if (curves.empty()) return std::numeric_limits<double>::quiet_NaN();
        auto it = std::lower_bound(curves.cbegin(), curves.cend(), t,
                                   [](const std::pair<utctime, rating_curve_function>& l, utctime r) { return l.first < r; });
        if (it == curves.cbegin() && it->first > t) {
            return std::numeric_limits<double>::quiet_NaN();
        } else if (it == curves.cend() || it->first > t) {  // the last curve is valid indefinitely
            it--;
        }
        return it->second.flow(level);
    }
};

// rating_curve_ts::value(i) = rc_param.flow(time(i), level_ts.value(i)) (:1641-1644); the level's point type (:1603)
inline std::vector<double> rating_curve_values(const point_ts& level, const rating_curve_parameters& rc) {
    std::vector<double> r(level.size());
    for (size_t i = 0; i < level.size(); ++i) r[i] = rc.flow(level.time(i), level.value(i));
    return r;
}

// ---- ice packing (time_series.h:1653-1831) ------------------------------------------------------------------------------
struct ice_packing_parameters {
    utctimespan window = 0;       // ticks
    double threshold_temp = 0.0;
};
enum ice_packing_temperature_policy : int { DISALLOW_MISSING = 0, ALLOW_INITIAL_MISSING = 1, ALLOW_ANY_MISSING = 2 };

// ice_packing_ts::detect_ice_packing(t) (:1808-1831)
inline double detect_ice_packing(const point_ts& temp, const ice_packing_parameters& ip, ice_packing_temperature_policy policy,
                                 utctime t) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    utcperiod p(t - ip.window, t);
    if (policy != DISALLOW_MISSING) {
        if (p.start < temp.total_period().start) p.start = std::min(temp.total_period().start, p.end);
    }
    if (p.timespan() == utctimespan{0}) return 0.0;  // clipped to zero, or window 0: no ice-packing
    utctimespan t_sum = 0;
    size_t ix_hint = npos;
    double p_sum = accumulate_value(temp, p, ix_hint, t_sum, temp.fx == POINT_INSTANT_VALUE);
    if (!std::isfinite(p_sum) || t_sum == utctimespan{0}) return nan;
    if (policy == ALLOW_ANY_MISSING || (t_sum == p.timespan()))  // compared in integer ticks
        return p_sum / to_seconds(t_sum) < ip.threshold_temp ? 1.0 : 0.0;
    return nan;
}

// ---- ice packing recession (time_series_dd.h:1186-1365) -----------------------------------------------------------------
struct ice_packing_recession_parameters {
    double alpha = 0.0;
    double recession_minimum = 0.0;
};

// ensure_overlap (:1358-1362) with utcperiod::contains(utcperiod) (utctime_utilities.h:93)
inline void ensure_overlap(const utcperiod& ice, const utcperiod& flow) {
    if (!(ice.valid() && flow.valid() && flow.start >= ice.start && flow.end <= ice.end))
        throw std::runtime_error("ice_packing_recession_ts: total period of flow ts should equal or be contained in ice "
                                 "packing ts total period");
}

// ice_packing_recession_ts::evaluate(time(i)) (:1323-1354) with the indicator taken at the flow's own time points:
// ice[k] is ice_packing_ts(flow.time(k))
inline double ice_packing_recession_value(const point_ts& flow, const std::vector<double>& ice_at,
                                          const ice_packing_recession_parameters& ipr, size_t i) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const utctime t = flow.time(i);
    double ice = ice_at[i];
    if (!std::isfinite(ice)) return nan;
    const double indicator_limit = 0.5;
    if (ice > indicator_limit) {
        size_t f_ix = i;  // flow_ts.index_of(time(i))
        while (f_ix > 0 && ice > indicator_limit) {
            ice = ice_at[--f_ix];
            if (!std::isfinite(ice)) return nan;
        }
        const double qs = flow.value(f_ix);
        const utctime ts = flow.time(f_ix);
        const double qbf = ipr.recession_minimum;
        const double alpha = ipr.alpha;
        return qbf + (qs - qbf) * detmath::exp(-alpha * to_seconds(t - ts));
    } else {
        return flow(t);
    }
}

// ---- min-max check with linear fill (time_series_dd.h:1456-1478; time_series_dd.cpp:1335-1376) --------------------------
struct qac_parameter {
    utctimespan max_timespan = std::numeric_limits<int64_t>::max();
    double min_x = std::numeric_limits<double>::quiet_NaN();
    double max_x = std::numeric_limits<double>::quiet_NaN();
    bool is_ok_quality(const double& x) const noexcept {  // :1463-1471
        if (!std::isfinite(x)) return false;
        if (std::isfinite(min_x) && x < min_x) return false;
        if (std::isfinite(max_x) && x > max_x) return false;
        return true;
    }
};

// qac_ts::_fill_value(i) without a replacement series (time_series_dd.cpp:1335-1367)
inline double qac_fill_value(const point_ts& ts, const qac_parameter& p, size_t i) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    auto t = ts.time(i);
    const size_t n = ts.size();
    if (i == 0 || i + 1 >= n || p.max_timespan == utctimespan{0}) return nan;
    size_t j = i;
    while (j--) {  // find the previous valid point
        utctime t0 = ts.time(j);
        if (t - t0 > p.max_timespan) return nan;
        double x0 = ts.value(j);
        if (p.is_ok_quality(x0)) {
            for (size_t k = i + 1; k < n; ++k) {  // then the next valid point
                utctime t1 = ts.time(k);
                if (t1 - t0 > p.max_timespan) return nan;
                double x1 = ts.value(k);
                if (p.is_ok_quality(x1)) {
                    double a = (x1 - x0) / to_seconds(t1 - t0);
                    double b = x0 - a * to_seconds(t0);
                    double xt = a * to_seconds(t) + b;
                    return xt;
                }
            }
        }
    }
    return nan;
}

// qac_ts::value(i) (time_series_dd.cpp:1369-1376)
inline double qac_value(const point_ts& ts, const qac_parameter& p, size_t i) {
    double x = ts.value(i);
    if (p.is_ok_quality(x)) return x;
    return qac_fill_value(ts, p, i);
}

}  // namespace shyft_hip::host
