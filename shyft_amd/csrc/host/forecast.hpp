// Forecast skill by lead time and the forecast merge (C++17, no device code): core/time_series_merge.h restated
// statement by statement on point_ts of host/time_series.hpp, with int64 microseconds.
//
//  slice_averages           average_accessor<ts, fixed_dt(t0, dt, n)>::value(i) with USE_NAN, the n slice averages
//                           that ats_vector::average_slice and nash_sutcliffe take (time_series_dd.cpp:1137-1165).
//  forecast_nash_sutcliffe  time_series_merge.h:123-144: the slice averages of every forecast and of the observation
//                           on the forecast's own axis, appended forecast-major, then 1 - the goal function.
//  forecast_merge           time_series_merge.h:47-99: one slice of every forecast spliced into a point series.
//
// This header is the definition of correct for kernels/forecast.hip: shyft_hip_forecast_skill_host runs these
// functions, and the device result is bit-identical to them.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "time_series.hpp"

namespace shyft_hip::host {

// average_accessor<ts, fixed_dt>(ts, fixed_dt(t0, dt, n)).value(i) for every i
inline std::vector<double> slice_averages(const point_ts& ts, utctime t0, utctimespan dt, size_t n) {
    return average_values(ts, fixed_dt(t0, dt, n));
}

// 1 - E of nash_sutcliffe_goal_function (core/time_series.h:2316-2344) without its size test: two sequential passes
// in index order over the pairs where both values are finite. goal::nash_sutcliffe of host/calibration.hpp is the
// same formula; that header brings the whole region model with it, which the kernel library does not include, so the
// statement stands here a second time. No special cases: without finite pairs 0/0, a constant observation x/0.
inline double nash_sutcliffe_goal(const std::vector<double>& obs, const std::vector<double>& sim) {
    double err2 = 0.0, mean = 0.0;
    size_t count = 0;
    for (size_t i = 0; i < obs.size(); ++i)
        if (std::isfinite(obs[i]) && std::isfinite(sim[i])) {
            const double d = obs[i] - sim[i];
            err2 += d * d;
            mean += obs[i];
            ++count;
        }
    mean /= double(count);
    double var2 = 0.0;
    for (size_t i = 0; i < obs.size(); ++i)
        if (std::isfinite(obs[i]) && std::isfinite(sim[i])) {
            const double d = obs[i] - mean;
            var2 += d * d;
        }
    return err2 / var2;
}

// The two vectors of time_series_merge.h:129-139: for each forecast in order the n slice averages of the forecast
// (vs) and of obs (vo) on the axis (forecast.time(0) + t0_offset, dt, n), appended. obs == nullptr is an observation
// that is not there: NaN throughout.
inline void forecast_slices(const std::vector<const point_ts*>& tsv, const point_ts* obs, utctimespan t0_offset,
                            utctimespan dt, size_t n, std::vector<double>& vs, std::vector<double>& vo) {
    for (const point_ts* ts : tsv) {
        if (ts->size() == 0) throw std::runtime_error("forecast_skill: a forecast has no points");
        const utctime t0 = ts->t.front() + t0_offset;
        const std::vector<double> s = slice_averages(*ts, t0, dt, n);
        vs.insert(vs.end(), s.begin(), s.end());
        if (obs && obs->size()) {
            const std::vector<double> o = slice_averages(*obs, t0, dt, n);
            vo.insert(vo.end(), o.begin(), o.end());
        } else {
            vo.insert(vo.end(), n, std::numeric_limits<double>::quiet_NaN());
        }
    }
}

// nash_sutcliffe(tsv, obs, t0_offset, dt, n) (time_series_merge.h:123-144). The reference returns NaN for an empty
// vector or observation before it builds anything, and its goal function throws for n == 0.
inline double forecast_nash_sutcliffe(const std::vector<const point_ts*>& tsv, const point_ts& obs, utctimespan t0_offset,
                                      utctimespan dt, size_t n) {
    if (tsv.empty() || obs.size() == 0) return std::numeric_limits<double>::quiet_NaN();
    std::vector<double> vs, vo;
    vs.reserve(n * tsv.size());
    vo.reserve(n * tsv.size());
    forecast_slices(tsv, &obs, t0_offset, dt, n, vs, vo);
    if (vs.empty()) throw std::runtime_error("nash_sutcliffe needs equal sized ts accessors with elements >1");
    return 1.0 - nash_sutcliffe_goal(vo, vs);
}

inline double forecast_nash_sutcliffe(const std::vector<point_ts>& tsv, const point_ts& obs, utctimespan t0_offset,
                                      utctimespan dt, size_t n) {
    std::vector<const point_ts*> p;
    for (const point_ts& ts : tsv) p.push_back(&ts);
    return forecast_nash_sutcliffe(p, obs, t0_offset, dt, n);
}

// forecast_merge(tsv, t0_offset, dt) (time_series_merge.h:47-99): from each forecast the slice
// [time(0) + t0_offset, + dt), stretched backwards over a gap left by the forecast before it and forwards (dt_extra)
// up to the first point of the next one.
//
// The reference's two walks test `ts.time(ix) < ..` before `ix < ts.size()`, so on an apoint_ts they throw out of
// time(i) whenever a walk reaches the end of a forecast; that includes the index_of == npos branch, which starts at the
// last point and always ends that way. That is kept as an error here, and no point past the last is read. A forecast
// without points makes the reference throw from time(0); it is an error here too.
inline point_ts forecast_merge(const std::vector<const point_ts*>& tsv, utctimespan t0_offset, utctimespan dt) {
    if (tsv.empty()) return point_ts();
    auto time_at = [&](size_t i, size_t ix) {
        if (ix >= tsv[i]->size())
            throw std::runtime_error("forecast_merge: forecast " + std::to_string(i) + " ends inside its slice");
        return tsv[i]->t[ix];
    };
    for (size_t i = 0; i < tsv.size(); ++i)
        if (tsv[i]->size() == 0)
            throw std::runtime_error("forecast_merge: forecast " + std::to_string(i) + " has no points");
    std::vector<utctime> tv;
    std::vector<double> vv;
    utctime t_previous_end = tsv.front()->t[0] + t0_offset;
    for (size_t i = 0; i < tsv.size(); ++i) {
        const point_ts& ts = *tsv[i];
        utctime t_start = ts.t[0] + t0_offset;  // where we want to extract data
        size_t ix;
        if (t_start > t_previous_end) {  // fill the gap until the slice starts
            ix = index_of(ts, t_previous_end);
            if (ix == npos) ix = 0;  // the forecast starts after t_previous_end: from its first point
            while (time_at(i, ix) < t_start) {
                tv.push_back(ts.t[ix]);
                vv.push_back(ts.v[ix]);
                ++ix;
            }
        } else {  // ordinary case, this forecast falls into place
            if (t_start < t_previous_end) t_start = t_previous_end;
            ix = index_of(ts, t_start);
            if (ix == npos) ix = ts.size() - 1;  // t_start is after the last interval: the last value
        }
        utctimespan dt_extra = 0;  // a missing next forecast is filled from this one
        if (i + 1 < tsv.size()) dt_extra = std::max(utctimespan(0), tsv[i + 1]->t[0] - (t_start + dt));
        const utctime t_end = t_start + dt + dt_extra;
        while (time_at(i, ix) < t_end) {
            tv.push_back(ts.t[ix]);
            vv.push_back(ts.v[ix]);
            ++ix;
        }
        t_previous_end = t_end;
    }
    return point_ts(std::move(tv), t_previous_end, std::move(vv), tsv.front()->fx);
}

}  // namespace shyft_hip::host
