// Internal, host-only: the argument checks of S point series in CSR form (row [S+1], t and v [row[S]], t_end [S],
// fx [S]) that shyft_hip_resample and the shyft_hip_ts_* entries share between their device and host twins, with the
// texts of host/time_series.hpp point_ts (core/time_axis.h:271-293). `prefix` names the entry family in the texts.
#pragma once
#include <stdint.h>

#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../host/time_series.hpp"

namespace shyft_hip_impl {

inline void check_csr_rows(const char* prefix, size_t S, const int64_t* row) {
    if (row[0] != 0) throw std::runtime_error(std::string(prefix) + ": row[0] must be 0");
    for (size_t s = 0; s < S; ++s)
        if (row[s + 1] < row[s]) throw std::runtime_error(std::string(prefix) + ": row must not decrease");
}

// the pointers and the CSR rows; after it every series s < S can be given to check_point_series_at
inline void check_point_series_rows(const char* who, const char* prefix, size_t S, const int64_t* row, const int64_t* t,
                                    const double* v, const int64_t* t_end, const int32_t* fx) {
    if (!row || !t_end || !fx) throw std::runtime_error(std::string(who) + ": null argument");
    check_csr_rows(prefix, S, row);
    if (row[S] > 0 && (!t || !v)) throw std::runtime_error(std::string(who) + ": null argument");
}

// series s: its fx, strictly increasing times, t_end after the last, and times inside a quarter of the 64-bit range
// (differences and sums of two times stay inside int64)
inline void check_point_series_at(const char* prefix, size_t s, const int64_t* row, const int64_t* t, const int64_t* t_end,
                                  const int32_t* fx) {
    namespace h = shyft_hip::host;
    if (fx[s] != int32_t(h::POINT_INSTANT_VALUE) && fx[s] != int32_t(h::POINT_AVERAGE_VALUE))
        throw std::runtime_error(std::string(prefix) + ": fx must be POINT_INSTANT_VALUE or POINT_AVERAGE_VALUE");
    const int64_t b = row[s], e = row[s + 1];
    if (b == e) return;
    for (int64_t k = b + 1; k < e; ++k)
        if (!(t[k - 1] < t[k])) throw std::runtime_error("time_axis::point_dt() needs time-points in increasing order");
    if (!(t_end[s] > t[e - 1])) throw std::runtime_error("time_axis::point_dt() illegal end-of-axis");
    if (t[b] < std::numeric_limits<int64_t>::min() / 4 || t_end[s] > std::numeric_limits<int64_t>::max() / 4)
        throw std::runtime_error(std::string(prefix) + ": times beyond a quarter of the 64-bit range are not supported");
}

// Both of the above, series by series. An entry with per-series rules of its own that must keep their place between
// the series (shyft_hip_resample) calls the two parts itself.
inline void check_point_series(const char* who, const char* prefix, size_t S, const int64_t* row, const int64_t* t,
                               const double* v, const int64_t* t_end, const int32_t* fx) {
    check_point_series_rows(who, prefix, S, row, t, v, t_end, fx);
    for (size_t s = 0; s < S; ++s) check_point_series_at(prefix, s, row, t, t_end, fx);
}

inline shyft_hip::host::point_ts point_series(size_t s, const int64_t* row, const int64_t* t, const double* v,
                                              const int64_t* t_end, const int32_t* fx) {
    namespace h = shyft_hip::host;
    return h::point_ts(std::vector<h::utctime>(t + row[s], t + row[s + 1]), t_end[s],
                       std::vector<double>(v + row[s], v + row[s + 1]), h::ts_point_fx(fx[s]));
}

}  // namespace shyft_hip_impl
