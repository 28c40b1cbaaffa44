// accumulate_value on the device: the area of one point series over one period, statement by statement as
// host/time_series.hpp accumulate_value (core/time_series.h:202-288). Shared by kernels/resample.hip (one period per
// target interval), kernels/tsprep.hip (one window per ice-packing query) and kernels/ts_percentiles.hip (one period
// per interval of a shifted view); there is one copy.
//
// Every operation is evaluated as written: int64 tick arithmetic, to_seconds(x) = double(x) / 1e6 as a division,
// no FMA (-ffp-contract=off), isfinite by the exponent bits (rs_nan and rs_finite: device/workgroup.h).
//
// Index safety. The caller passes the n > 0 points of one series, whose times increase strictly and whose t_end lies
// after the last (checked on the host before the launch). rs_area reads point k only with k < n: the start index is
// at most n - 1, every read is followed by the test `k == n` which ends the walk, and the one place where the
// reference reads without that test (a one-point series whose point lies inside a period that starts before it,
// where the reference throws from point_dt::time) is refused by the host check and, should it reach the device, ends
// the walk with NaN.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "workgroup.h"

__device__ inline double rs_seconds(int64_t dt) { return double(dt) / 1e6; }
__device__ inline int64_t rs_max(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ inline int64_t rs_min(int64_t a, int64_t b) { return a < b ? a : b; }

// accumulate_value(source, [ps, pe), ., tsum, linear, strict_linear_between = true) over the n > 0 points t, v of
// one series (host/time_series.hpp accumulate_value, statement by statement); tsum == 0 gives NaN
//
// shift is added to every point time as it is read: the series seen `shift` later (time_shift_ts,
// core/time_series_dd.h:707-751), t_end already moved by the caller. The linear branch takes to_seconds of absolute
// times (rt, px_start + px_end), so moving the period instead would round differently; the stair-case branch uses
// differences only. The default 0 is the series as stored.
__device__ inline double rs_area(const int64_t* __restrict__ t_stored, const double* __restrict__ v, int64_t n,
                                 int64_t t_end, int64_t ps, int64_t pe, bool linear, int64_t& tsum, int64_t shift = 0) {
    const bool extrapolate_flat = !linear;
    const struct {
        const int64_t* __restrict__ p;
        int64_t d;
        __device__ int64_t operator[](int64_t k) const { return p[k] + d; }
    } t{t_stored, shift};
    tsum = 0;
    // open_range_index_of(ps): -1 before the first point, n - 1 from the last point on
    int64_t i;
    if (ps >= t_end) {
        i = n - 1;
    } else if (ps < t[0]) {
        i = -1;
    } else if (ps >= t[n - 1]) {
        i = n - 1;
    } else {  // upper_bound - 1; t[0] <= ps < t[n-1]
        i = first_false(int64_t(0), n, [&](int64_t m) { return t[m] <= ps; }) - 1;
    }
    int64_t lt = 0;
    double lv = rs_nan();
    bool l_finite = false;
    if (i < 0) {
        i = 0;
        lt = t[i];
        lv = v[i];
        ++i;
        l_finite = rs_finite(lv);
        if (!(lt >= ps && lt < pe)) return rs_nan();
        if (i == n) return rs_nan();  // the reference throws here; the host check refuses it before the launch
    }
    double area = 0.0;
    while (true) {
        if (!l_finite) {
            lt = t[i];
            lv = v[i];
            ++i;
            l_finite = rs_finite(lv);
            if (i == n) {
                if (l_finite && lt < pe) {
                    if (extrapolate_flat) {
                        const int64_t dt = pe - rs_max(ps, lt);
                        tsum += dt;
                        area += rs_seconds(dt) * lv;
                    }
                }
                break;
            }
            if (lt >= pe) break;
        } else {
            const int64_t rt = t[i];
            const double rv = v[i];
            ++i;
            const bool r_finite = rs_finite(rv);
            const int64_t px_start = rs_max(lt, ps), px_end = rs_min(rt, pe);
            int64_t dt = px_end - px_start;
            if (linear && r_finite) {
                const double a = (rv - lv) / rs_seconds(rt - lt);
                const double b = rv - a * rs_seconds(rt);
                area += rs_seconds(dt) * (0.5 * a * rs_seconds(px_start + px_end) + b);
                tsum += dt;
            } else {
                if (extrapolate_flat) {
                    area += lv * rs_seconds(dt);
                    tsum += dt;
                }
            }
            if (i == n) {
                if (r_finite && rt < pe) {
                    if (extrapolate_flat) {
                        dt = pe - rt;
                        tsum += dt;
                        area += rs_seconds(dt) * rv;
                    }
                }
                break;
            }
            if (rt >= pe) break;
            l_finite = r_finite;
            lt = rt;
            lv = rv;
        }
    }
    return tsum ? area : rs_nan();
}
