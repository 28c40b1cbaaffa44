// Host restatements of the point-wise filter series of the reference on host::point_ts (C++17, no device code). They
// are the definition of correct for kernels/tsfilter.hip, whose device entries are bit-identical to them; the _host
// entries of the C ABI run these on one thread.
//
//  convolve_policy, convolve_w_ts::value              core/time_series.h:895-980 (value: 966-975)
//  derivative_method, derivative_ts::values,          core/time_series_dd.h:170-175, 583-607;
//  derivative_fx                                      core/time_series_dd.cpp:311-463
//  inside_parameter::inside_value                     core/time_series_dd.h:1538-1554
//  bitmask, bit_decoder::decode                       core/time_series_dd.h:1609-1658; argument texts of
//                                                     apoint_ts::decode core/time_series_dd.cpp:942-948
// Every operation is evaluated as written: int64 ticks, to_seconds as a division, no FMA (-ffp-contract=off).
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "time_series.hpp"

namespace shyft_hip::host {

// ---- convolve_w (time_series.h:895-980) -------------------------------------------------------------------------------
enum convolve_policy : int { USE_FIRST = 0, USE_ZERO = 1, USE_NAN = 2 };  // :900-904

// convolve_w_ts::value(i) (:966-975): one accumulator, the taps in ascending j, a multiply and then an add
inline double convolve_w_value(const point_ts& ts, const double* w, size_t K, convolve_policy policy, size_t i) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double v = 0.0;
    for (size_t j = 0; j < K; ++j)
        v += j <= i ? w[j] * ts.v[i - j]
                    : (policy == USE_FIRST ? w[j] * ts.v[0] : (policy == USE_ZERO ? 0.0 : nan));
    return v;
}

// ---- derivative (time_series_dd.h:170-175, 583-607; time_series_dd.cpp:311-463) -----------------------------------------
enum derivative_method : int { DEFAULT_DIFF = 0, FORWARD_DIFF = 1, BACKWARD_DIFF = 2, CENTER_DIFF = 3 };

// the end of period i of the series' axis: the next point, t_end for the last one (point_dt::period, time_axis.h)
inline utctime period_end(const point_ts& ts, size_t i) { return i + 1 < ts.size() ? ts.t[i + 1] : ts.t_end; }

// derivative_fx (time_series_dd.cpp:311-448) for point i of a stair-case series. dt > 0 takes the fixed-step branch
// (:317-359), dt == 0 the variable one (:360-446).
//
// The reference works in place over the whole vector. Written per point this is the same, because no statement there
// reads a value it has already overwritten: the center loops carry the original v[i-1] along in v0 (`v0 = v1` with v1
// read before v[i] is stored), and read v[i+1] before the loop reaches it; the forward loop runs upwards and reads
// v[i] and v[i+1], neither stored yet; the fixed backward loop runs from the far end and reads v[i] and v[i-1], and
// the variable backward loop carries the original v[i-1] in v0. So every output is a function of the original
// v[i-1], v[i], v[i+1] and the periods around i, which is what this states.
inline double derivative_fx_value(const point_ts& ts, utctimespan dt, derivative_method dm, size_t i) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t n = ts.size();
    const std::vector<double>& v = ts.v;
    const std::vector<utctime>& t = ts.t;
    if (n < 2) return std::isfinite(v[0]) ? 0.0 : nan;  // :312-314, flat or nan
    const double v1 = v[i];
    if (dt > utctimespan{0}) {
        switch (dm) {
        case DEFAULT_DIFF:
        case CENTER_DIFF:
            if (i == 0)  // :322
                return std::isfinite(v1) ? (std::isfinite(v[1]) ? (v[1] - v1) / to_seconds(2 * dt) : 0.0) : nan;
            if (i + 1 == n)  // :344
                return std::isfinite(v1) ? (std::isfinite(v[i - 1]) ? (v1 - v[i - 1]) / to_seconds(2 * dt) : 0.0) : nan;
            if (std::isfinite(v1)) {  // :325-341
                const double v0 = v[i - 1];
                if (std::isfinite(v0)) {
                    if (std::isfinite(v[i + 1])) return (v[i + 1] - v0) / to_seconds(2 * dt);
                    return (v1 - v0) / to_seconds(2 * dt);
                }
                if (std::isfinite(v[i + 1])) return (v[i + 1] - v1) / to_seconds(2 * dt);
                return 0.0;
            }
            return nan;
        case FORWARD_DIFF:  // :348-351
            if (i + 1 == n) return std::isfinite(v1) ? 0.0 : nan;
            return std::isfinite(v1) ? (std::isfinite(v[i + 1]) ? (v[i + 1] - v1) / to_seconds(dt) : 0.0) : nan;
        case BACKWARD_DIFF:  // :354-357
            if (i == 0) return std::isfinite(v1) ? 0.0 : nan;
            return std::isfinite(v1) ? (std::isfinite(v[i - 1]) ? (v1 - v[i - 1]) / to_seconds(dt) : 0.0) : nan;
        }
        return nan;
    }
    // variable intervals: period k is [t[k], period_end(k))
    switch (dm) {
    case DEFAULT_DIFF:
    case CENTER_DIFF:
        if (i == 0)  // :367, p1.end - p0.start
            return std::isfinite(v1) ? (std::isfinite(v[1]) ? (v[1] - v[0]) / to_seconds(period_end(ts, 1) - t[0]) : 0.0) : nan;
        if (i + 1 == n) {  // :392-402, p1.end - p0.start
            if (std::isfinite(v1)) {
                if (std::isfinite(v[i - 1])) return (v1 - v[i - 1]) / to_seconds(ts.t_end - t[i - 1]);
                return 0.0;
            }
            return nan;
        }
        if (std::isfinite(v1)) {  // :373-387
            const double v0 = v[i - 1], v2 = v[i + 1];
            if (std::isfinite(v0)) {
                if (std::isfinite(v2))
                    return 2 * (v2 - v0) / to_seconds((t[i + 1] - t[i - 1]) + (period_end(ts, i + 1) - period_end(ts, i - 1)));
                return (v1 - v0) / to_seconds(period_end(ts, i) - t[i - 1]);
            } else if (std::isfinite(v2)) {
                return (v2 - v1) / to_seconds(period_end(ts, i + 1) - t[i]);
            }
            return 0.0;
        }
        return nan;
    case FORWARD_DIFF:  // :406-423
        if (i + 1 == n) return std::isfinite(v1) ? 0.0 : nan;
        if (std::isfinite(v1)) {
            if (std::isfinite(v[i + 1]))
                return 2 * (v[i + 1] - v1) / to_seconds((t[i + 1] - t[i]) + (period_end(ts, i + 1) - period_end(ts, i)));
            return 0.0;
        }
        return nan;
    case BACKWARD_DIFF:  // :426-443
        if (i == 0) return std::isfinite(v1) ? 0.0 : nan;
        if (std::isfinite(v1)) {
            if (std::isfinite(v[i - 1]))
                return 2 * (v1 - v[i - 1]) / to_seconds((t[i] - t[i - 1]) + (period_end(ts, i) - period_end(ts, i - 1)));
            return 0.0;
        }
        return nan;
    }
    return nan;
}

// derivative_ts::values() (time_series_dd.cpp:450-463), point i; the result is POINT_AVERAGE_VALUE (:594)
inline double derivative_value(const point_ts& ts, utctimespan dt, derivative_method dm, size_t i) {
    if (ts.fx == POINT_INSTANT_VALUE) {
        if (i + 1 < ts.size()) return (ts.v[i + 1] - ts.v[i]) / to_seconds(ts.t[i + 1] - ts.t[i]);
        return std::numeric_limits<double>::quiet_NaN();
    }
    return derivative_fx_value(ts, dt, dm, i);
}

// ---- inside (time_series_dd.h:1538-1554) ------------------------------------------------------------------------------
struct inside_parameter {
    double min_x = std::numeric_limits<double>::quiet_NaN();
    double max_x = std::numeric_limits<double>::quiet_NaN();
    double nan_x = std::numeric_limits<double>::quiet_NaN();
    double x_inside = 1.0;
    double x_outside = 0.0;
    double inside_value(const double& x) const noexcept {  // :1546-1554, the range is [min_x, max_x)
        if (!std::isfinite(x)) return nan_x;
        if (std::isfinite(min_x) && x < min_x) return x_outside;
        if (std::isfinite(max_x) && x >= max_x) return x_outside;
        return x_inside;
    }
};

// ---- decode (time_series_dd.h:1609-1658) ------------------------------------------------------------------------------
template <typename R>
constexpr R bitmask(unsigned int const onecount) {  // :1610-1613
    return static_cast<R>(-(onecount != 0)) & (static_cast<R>(-1) >> ((sizeof(R) * CHAR_BIT) - onecount));
}

struct bit_decoder {
    uint64_t start_bit{0};
    uint64_t bit_mask{0};
    bit_decoder() = default;
    bit_decoder(unsigned int start_bit_, unsigned int n_bits) : start_bit{start_bit_}, bit_mask{bitmask<uint64_t>(n_bits)} {}
    double decode(double x) const {  // :1650-1655
        const double nan = std::numeric_limits<double>::quiet_NaN();
        if (!std::isfinite(x)) return nan;
        if (x < 0) return nan;
        if (x > double(uint64_t(1) << 52)) return nan;
        return double((uint64_t(x) >> start_bit) & bit_mask);
    }
};

// the argument checks of apoint_ts::decode (time_series_dd.cpp:943-946), with its texts
inline void check_decode_arguments(int start_bit, int n_bits) {
    if (start_bit < 0 || start_bit > 51)
        throw std::runtime_error("start_bit must be in range [0..51], was " + std::to_string(start_bit));
    if (n_bits < 1 || n_bits > 51 - start_bit)  // start_bit + n_bits > 51, written so that the sum cannot overflow
        throw std::runtime_error("n_bits must be > 0 and start_bit+n_bits <= 51: n_bits =" + std::to_string(n_bits) +
                                 ", start_bit=" + std::to_string(start_bit));
}

}  // namespace shyft_hip::host
