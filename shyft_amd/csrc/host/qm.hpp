// Quantile mapping of weighted forecasts onto historical scenarios (core/time_series_qm.h), restated function by
// function in plain C++. map_step is one time step of quantile_mapping (:296-351) on dense rows and is the definition
// of correct for kernels/qm.hip (shyft_hip_quantile_map_host runs it; the device result is bit-identical to it);
// step_modes is what quantile_mapping derives from the times; plan and historical_tail are the time-axis work of
// quantile_map_forecast (:401-450). No device code here.
//
// Where the reference leaves a result open, this restatement fixes it:
//  - quantile_index (:34-52) orders the finite values of a step with std::sort, which leaves the order of equal
//    values open. Here ties go by ascending series index (+0.0 and -0.0 are equal, so they tie). This is one of the
//    orders the reference may produce.
//  - compute_interp_weighted_quantiles (:139-170) with one quantile (one finite scenario) has q_i = NaN, never enters
//    its loop and reads value(size_t(-1)). Here the result is value(0), as compute_weighted_quantiles (:80-100)
//    gives for one quantile by its own arithmetic.
//  - a weight that is not finite and > 0 makes the reference's loops run forever or divide by zero; the entries
//    refuse such weights.
//
// The running q_j walks of :88-98 and :146-153 have a closed form over the sequential prefix sums, which is what the
// kernel evaluates rank by rank:
//   plain:  cum[0] = 0, cum[j+1] = cum[j] + weight(j); quantile i is value(min(first j with !(cum[j+1] < q_i), n-1))
//   interp: width[j] = 0.5*weight(j-1) + 0.5*weight(j) (weight(-1) = 0), mid[j] = mid[j-1] + width[j];
//           j = first j with mid[j] > q_i, else n-1; flat value(j) when j == 0 or (j == n-1 and q_i >= mid[j]), else
//           value(j-1) + ((value(j) - value(j-1)) / width[j]) * (q_i - (mid[j] - width[j]))
// with q_i = (1.0/(n_q-1))*i. The sums are formed one rounded add at a time in rank order, never reassociated.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "time_series.hpp"

namespace shyft_hip::host::qm {

enum step_mode : int32_t { PRIOR = 0, QM = 1, QM_BLEND = 2 };  // SHYFT_HIP_QM_PRIOR / _QM / _QM_BLEND

constexpr utctime no_utctime = std::numeric_limits<int64_t>::min();  // utctime_utilities.h:38
inline bool is_valid(utctime t) { return t != no_utctime; }           // utctime_utilities.h:45

// the reference's utcperiod (utctime_utilities.h:86-91): default-constructed invalid
struct period {
    utctime start = no_utctime, end = no_utctime;
    period() = default;
    period(utctime s, utctime e) : start(s), end(e) {}
    bool valid() const { return start != no_utctime && end != no_utctime && start <= end; }
    bool contains(utctime t) const { return is_valid(t) && valid() ? t >= start && t < end : false; }
};

struct step_scratch {
    std::vector<int> fi, pi;       // quantile_index of the step: forecasts, scenarios
    std::vector<double> a, width;  // cum[j+1] or mid[j]; width[j]
};

// One step of quantile_mapping (:325-347). fc [F] and pri [P] are the averaged values of the step (NaN = not covered),
// w [F] the unpacked weights; out [P].
inline void map_step(size_t F, size_t P, const double* fc, const double* w, const double* pri, int mode,
                     double interp_weight, bool interpolated_quantiles, double* out, step_scratch& s) {
    // quantile_index (:40-50): the finite ones, ascending by value, ties by ascending index (stable from index order)
    auto order = [](size_t n, const double* v, std::vector<int>& ix) {
        ix.clear();
        for (size_t i = 0; i < n; ++i)
            if (std::isfinite(v[i])) ix.push_back(int(i));
        std::stable_sort(ix.begin(), ix.end(), [v](int a, int b) { return v[a] < v[b]; });
    };
    order(F, fc, s.fi);
    const size_t n = s.fi.size();
    if (mode == PRIOR || n == 0) {  // :345-347
        for (size_t i = 0; i < P; ++i) out[i] = pri[i];
        return;
    }
    order(P, pri, s.pi);
    const size_t n_q = s.pi.size();
    for (size_t i = 0; i < P; ++i) out[i] = std::numeric_limits<double>::quiet_NaN();  // :322-324
    if (n_q == 0) return;
    auto value = [&](size_t j) { return fc[s.fi[j]]; };
    double w_sum = 0.0;  // wvo_accessor (:197-203)
    for (size_t j = 0; j < n; ++j) w_sum += w[s.fi[j]];
    auto weight = [&](size_t j) { return w[s.fi[j]] / w_sum; };  // :208
    s.a.resize(n);
    s.width.resize(n);
    if (!interpolated_quantiles) {
        double c = 0.0;
        for (size_t j = 0; j < n; ++j) {
            c = c + weight(j);
            s.a[j] = c;
        }
    } else {
        double mid = 0.0, w_j = 0.0;
        for (size_t j = 0; j < n; ++j) {
            double width = 0.5 * w_j;  // :149-152
            w_j = weight(j);
            width += 0.5 * w_j;
            mid += width;
            s.a[j] = mid;
            s.width[j] = width;
        }
    }
    const double q_step = 1.0 / double(n_q - 1);  // :81, :140; inf for one quantile
    for (size_t i = 0; i < n_q; ++i) {
        const double q_i = q_step * double(i);
        double q;
        if (!interpolated_quantiles) {
            size_t j = 0;
            while (j < n && s.a[j] < q_i) ++j;
            q = value(std::min(j, n - 1));
        } else if (n_q == 1) {
            q = value(0);
        } else {
            size_t j = 0;
            while (j < n && !(s.a[j] > q_i)) ++j;
            j = std::min(j, n - 1);
            if (j == 0 || (j + 1 == n && q_i >= s.a[j])) {  // :157-159
                q = value(j);
            } else {  // :161-165
                const double interp_start = value(j - 1);
                const double interp_end = value(j);
                const double inclination = (interp_end - interp_start) / s.width[j];
                const double offset = s.a[j] - s.width[j];
                q = interp_start + inclination * (q_i - offset);
            }
        }
        const size_t k = size_t(s.pi[i]);
        out[k] = mode == QM_BLEND ? (1.0 - interp_weight) * q + interp_weight * pri[k] : q;  // :341, :343
    }
}

// compute_cover_period (:220-233) over the total periods of the forecasts
inline period compute_cover_period(const std::vector<const point_ts*>& tsv) {
    period fc_period;
    for (const point_ts* ts : tsv) {
        const utcperiod tp = ts->total_period();
        const period p = ts->size() ? period(tp.start, tp.end) : period();
        if (!fc_period.valid()) {
            fc_period = p;
        } else {
            fc_period.start = std::min(fc_period.start, p.start);
            fc_period.end = std::max(fc_period.end, p.end);
        }
    }
    return fc_period;
}

// compute_interpolation_period (:236-248)
inline period compute_interpolation_period(period fc_period, utctime interpolation_start, utctime interpolation_end,
                                           utctime t_end) {
    period interpolation_period;
    if (is_valid(interpolation_start)) {
        interpolation_period = period(interpolation_start, t_end);
        if (is_valid(interpolation_end)) interpolation_period.end = interpolation_end;
        interpolation_period.start = std::min(fc_period.end, interpolation_period.start);
        interpolation_period.end = std::min(fc_period.end, interpolation_period.end);
    }
    return interpolation_period;
}

// What quantile_mapping (:310-311, :328, :335-339) decides from the times alone, per step of its axis; a step
// without a finite forecast is PRIOR whatever its mode (the step itself sees that).
inline void step_modes(const fixed_dt& time_axis, period fc_period, utctime interpolation_start,
                       utctime interpolation_end, std::vector<int32_t>& mode, std::vector<double>& interp_weight) {
    mode.assign(time_axis.size(), PRIOR);
    interp_weight.assign(time_axis.size(), 0.0);
    if (time_axis.size() == 0) return;
    const period ip = compute_interpolation_period(fc_period, interpolation_start, interpolation_end,
                                                   time_axis.time(time_axis.size() - 1));
    for (size_t t = 0; t < time_axis.size(); ++t) {
        const utctime tt = time_axis.time(t);
        if (!(!is_valid(ip.end) || tt < ip.end)) continue;  // :328
        if (ip.contains(tt) || ip.end == tt) {              // :335-339
            mode[t] = QM_BLEND;
            interp_weight[t] = to_seconds(tt - ip.start) / to_seconds(ip.end - ip.start);
        } else {
            mode[t] = QM;
        }
    }
}

// The time-axis work of quantile_map_forecast (:416-422): how many leading steps of time_axis are quantile mapped.
struct plan_t {
    period fc_period;
    size_t qm_n_steps = 0;
    fixed_dt qm_time_axis;
};
inline plan_t plan(const std::vector<const point_ts*>& forecasts_unpacked, const fixed_dt& time_axis,
                   utctime interpolation_start, utctime interpolation_end) {
    plan_t r;
    r.fc_period = compute_cover_period(forecasts_unpacked);
    const utctime ta_last_step = time_axis.time(time_axis.size() - 1);
    const period ip = compute_interpolation_period(r.fc_period, interpolation_start, interpolation_end, ta_last_step);
    const utctime qm_end = ip.valid() ? ip.end : r.fc_period.end;
    const size_t qm_ix_end = time_axis.index_of(qm_end);
    r.qm_n_steps = qm_ix_end == npos ? time_axis.size() : qm_ix_end + 1;
    r.qm_time_axis = fixed_dt(time_axis.t, time_axis.dt, r.qm_n_steps);  // slice(0, qm_n_steps)
    return r;
}

// merge_qm_result's historical part (:369-372) on ta_ext = time_axis.slice(qm_n_steps, size - qm_n_steps) (:447)
inline std::vector<double> historical_tail(const point_ts& historical_ts, const fixed_dt& time_axis, size_t qm_n_steps) {
    const fixed_dt ta_ext(time_axis.t + utctimespan(qm_n_steps) * time_axis.dt, time_axis.dt,
                          time_axis.size() - qm_n_steps);
    return historical_ts.fx == POINT_AVERAGE_VALUE ? accumulate_stair_case(ta_ext, historical_ts, true)
                                                   : accumulate_linear(ta_ext, historical_ts, true);
}

}  // namespace shyft_hip::host::qm
