// Kalman bias prediction of the forecast post-processing flow (core/kalman.h:24-236): parameter, state, filter and
// bias_predictor with the reference's defaults and constructors. A filter here is the batched arithmetic of
// kernels/kalman.hip at M = 1 on its host path (shyft_hip_kalman_run_host), so these objects need no device; the
// step-uniform tables that the batched entry takes (fold, w, the running-bias pieces) are built here too.
#pragma once
#include <algorithm>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/shyft_hip.h"
#include "time_series.hpp"

namespace shyft_hip::host::kalman {

inline void kalman_check(int status) {
    if (status != 0) {
        const char* m = shyft_hip_last_error(nullptr);
        throw std::runtime_error(m ? m : "shyft_hip error");
    }
}

// kalman.h:24-51
struct state {
    std::vector<double> x;  // best estimate of the bias, one per daily period
    std::vector<double> k;  // kalman gain
    std::vector<double> P;  // error covariance, [n][n] row by row
    std::vector<double> W;  // process noise, [n][n] row by row
    int size() const { return int(x.size()); }
    state() = default;
    state(int n_daily_observations, double covariance_init, double hourly_correlation, double process_noise_init) {
        if (n_daily_observations < 0) throw std::runtime_error("kalman: n_daily_observations must not be negative");
        const size_t n = size_t(n_daily_observations);
        x.assign(n, 0.0);
        k.assign(n, 0.0);
        P.assign(n * n, 0.0);
        W.assign(n * n, 0.0);
        kalman_check(shyft_hip_kalman_initial_state(n_daily_observations, covariance_init, hourly_correlation,
                                                    process_noise_init, P.data(), W.data()));
    }
    // the distinct values of W by folded distance (the batched entry's w table)
    std::vector<double> w_table() const {
        const size_t n = x.size();
        return std::vector<double>(W.begin(), W.begin() + (n ? n / 2 + 1 : 0));
    }
};

// kalman.h:56-84; ratio_std_w_over_v is 0.15 from the constructor (:72-77)
struct parameter {
    int n_daily_observations = 8;
    double hourly_correlation = 0.93;
    double covariance_init = 0.5;
    double std_error_bias_measurements = 2.0;
    double ratio_std_w_over_v = 0.15;
    parameter(int n_daily_observations = 8, double hourly_correlation = 0.93, double covariance_init = 0.5,
              double std_error_bias_measurements = 2.0, double ratio_std_w_over_v = 0.15)
        : n_daily_observations(n_daily_observations), hourly_correlation(hourly_correlation),
          covariance_init(covariance_init), std_error_bias_measurements(std_error_bias_measurements),
          ratio_std_w_over_v(ratio_std_w_over_v) {}
};

// the running-bias tables of one time axis (compute_running_bias, kalman.h:203-225)
struct running_tables {
    int save_every = 1;
    std::vector<int32_t> piece_begin, piece_ix;
    std::vector<double> piece_seconds;
};

// kalman.h:103-146
struct filter {
    parameter p;
    filter() = default;
    explicit filter(const parameter& p_) : p(p_) {}

    state create_initial_state() const {
        return state(p.n_daily_observations, p.covariance_init, p.hourly_correlation,
                     p.std_error_bias_measurements != 0.0 ? p.ratio_std_w_over_v * p.std_error_bias_measurements : 100.0);
    }
    // kalman.h:114-116, its integer arithmetic: whole seconds, whole hours (both truncating), + 200 years
    int fold_to_daily_observation(utctime t) const {
        const int64_t seconds = t / US;
        return int(((seconds / 3600 + 200L * 24 * 365) % 24) * p.n_daily_observations / 24);
    }
    double v2() const { return p.std_error_bias_measurements * p.std_error_bias_measurements; }
    std::vector<int32_t> fold_table(const fixed_dt& ta) const {
        std::vector<int32_t> f(ta.size());
        for (size_t i = 0; i < ta.size(); ++i) f[i] = fold_to_daily_observation(ta.time(i));
        return f;
    }
    // The pieces of the day-periodic staircase (period 24 h, bin 24h/n, anchored at the start of the UTC day of
    // ta.time(0); profile_description / profile_accessor, core/time_series.h:590-692) inside every step of ta.
    running_tables running(const fixed_dt& ta) const {
        const utctimespan day = 86400 * US;
        const int n = p.n_daily_observations;
        if (n < 1) throw std::runtime_error("kalman: n_daily_observations must be at least 1");
        if (ta.dt <= 0 || ta.dt > day || day % ta.dt != 0)
            throw std::runtime_error("kalman: compute_running_bias needs a time-axis delta-t that divides 24 hours");
        running_tables r;
        r.save_every = int(std::min<int64_t>(day / ta.dt, std::numeric_limits<int>::max()));
        r.piece_begin.assign(ta.size() + 1, 0);
        if (ta.size() == 0) return r;
        const utctimespan bin = day / n, period = bin * n;
        if (bin <= 0) throw std::runtime_error("kalman: n_daily_observations is too large for the profile");
        utctime t0 = ta.t / day * day;
        if (t0 > ta.t) t0 -= day;           // calendar::trim(t, DAY) rounds down
        t0 -= (t0 - ta.t) / period * period;  // profile_description::reset_start
        for (size_t i = 0; i < ta.size(); ++i) {
            const utcperiod s = ta.period(i);
            for (utctime t = s.start; t < s.end;) {
                const int64_t b = (t - t0) / bin;
                const utctime e = std::min(t0 + (b + 1) * bin, s.end);
                r.piece_ix.push_back(int32_t(b % n));
                r.piece_seconds.push_back(to_seconds(e - t));
                t = e;
            }
            r.piece_begin[i + 1] = int32_t(r.piece_ix.size());
        }
        return r;
    }
    // T steps of one filter on the host path; mode 0 filter, 1 predictor
    void run(const std::vector<double>& bias, const std::vector<int32_t>& fold, int mode, state& s,
             double* out = nullptr, const running_tables* rt = nullptr) const {
        if (s.size() != p.n_daily_observations)
            throw std::runtime_error("kalman: the state's size differs from the filter's n_daily_observations");
        const auto w = s.w_table();
        kalman_check(shyft_hip_kalman_run_host(s.size(), 1, bias.size(), bias.data(), fold.data(), w.data(), v2(), mode,
                                               s.x.data(), s.k.data(), s.P.data(), out, rt ? rt->save_every : 1,
                                               rt ? rt->piece_begin.data() : nullptr, rt ? rt->piece_ix.data() : nullptr,
                                               rt ? rt->piece_seconds.data() : nullptr));
    }
    // kalman.h:127-145
    void update(double observed_bias, utctime t, state& s) const {
        run({observed_bias}, {int32_t(fold_to_daily_observation(t))}, 0, s);
    }
};

// fc - obs on the steps of ta, both through the average restatement; NaN where the forecast's total_period does
// not contain the start of the step (kalman.h:178-180, 226-227)
inline std::vector<double> observed_bias(const point_ts& fc, const std::vector<double>& obs_avg, const fixed_dt& ta) {
    std::vector<double> b = average_values(fc, ta);
    const utcperiod tp = fc.total_period();
    for (size_t i = 0; i < ta.size(); ++i)
        b[i] = tp.contains(ta.time(i)) ? b[i] - obs_avg[i] : std::numeric_limits<double>::quiet_NaN();
    return b;
}

// kalman.h:154-238
struct bias_predictor {
    filter f;
    state s;
    bias_predictor() = default;
    explicit bias_predictor(const filter& f_) : f(f_), s(f_.create_initial_state()) {}
    bias_predictor(const filter& f_, const state& s_) : f(f_), s(s_) {}

    // kalman.h:172-185: forecasts outer (oldest first), steps inner, non-finite bias skipped
    void update_with_forecast(const std::vector<point_ts>& fc_set, const point_ts& obs, const fixed_dt& ta) {
        const auto obs_avg = average_values(obs, ta);
        const auto fold = f.fold_table(ta);
        for (const auto& fc : fc_set) f.run(observed_bias(fc, obs_avg, ta), fold, 1, s);
    }
    // kalman.h:202-236
    std::vector<double> compute_running_bias(const point_ts& fc, const point_ts& obs, const fixed_dt& ta) {
        const auto rt = f.running(ta);
        std::vector<double> out(ta.size());
        if (ta.size() == 0) return out;
        f.run(observed_bias(fc, average_values(obs, ta), ta), f.fold_table(ta), 1, s, out.data(), &rt);
        return out;
    }
};

}  // namespace shyft_hip::host::kalman
