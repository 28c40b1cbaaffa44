// Internal, host only (no HIP): the index tables the region layer builds before a launch. A CSR segment table by
// counting sort (catchment, routing-group and ensemble segments), and the tables of a river network (routing.hip,
// routing_members.hip), and the UTC calendar with the per-step day-of-year / time-in-year tables of pt_gs_k.
// tools/host_tables_check.cpp runs all three under the address and undefined-behaviour sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace shyft_hip_impl {

// Counting sort of (key, item) pairs into off[n_keys + 1] / items: the items of key k are items[off[k] .. off[k + 1]),
// in the order they were enumerated (the segment sums add in that order). `pairs(emit)` calls emit(key, item) for
// every pair and runs twice, to count and to place, so it must enumerate the same pairs both times; a pair it does
// not emit is left out. Keys lie in [0, n_keys): the enumeration checks (and may throw) before it emits. Returns
// whether items is the identity 0, 1, 2, ... of its own length.
template <class Off, class Pairs>
bool build_csr(size_t n_keys, std::vector<Off>& off, std::vector<int32_t>& items, Pairs&& pairs) {
    off.assign(n_keys + 1, 0);
    pairs([&](size_t key, int32_t) { off[key + 1]++; });
    for (size_t k = 0; k < n_keys; ++k) off[k + 1] += off[k];
    items.resize(size_t(off[n_keys]));
    std::vector<Off> pos(off.begin(), off.end() - 1);
    pairs([&](size_t key, int32_t item) { items[size_t(pos[key]++)] = item; });
    for (size_t i = 0; i < items.size(); ++i)
        if (items[i] != int32_t(i)) return false;
    return true;
}

// routing::river_network as tables (core/routing.h:239-421) for P members that share the rivers: member m owns the
// group rows [group_row[m], group_row[m + 1]).
template <class Off>
struct river_tables {
    std::vector<Off> pair_off;         // [P*R + 1] CSR of the group rows of (member, river), ascending row
    std::vector<int32_t> pair_groups;  // [G]
    std::vector<int32_t> up_off, ups;  // [R + 1] CSR of the upstream rivers, ascending index (= ascending id)
    std::vector<int32_t> lvl_off, lvl_rivers;  // rivers by network level, upstream levels first, ascending index
    int n_levels() const { return int(lvl_off.size()) - 1; }
};

// The caller has checked group_river[g] in [0, R) and river_downstream[r] < R; a negative downstream is an outlet.
// Returns false when the network has a cycle (lvl_off / lvl_rivers are then not built): the caller raises its text.
template <class Off>
bool build_river_tables(size_t P, const int64_t* group_row, const int32_t* group_river, size_t R,
                        const int32_t* river_downstream, river_tables<Off>& tb) {
    build_csr(P * R, tb.pair_off, tb.pair_groups, [&](auto&& emit) {
        for (size_t m = 0; m < P; ++m)
            for (int64_t g = group_row[m]; g < group_row[m + 1]; ++g) emit(m * R + size_t(group_river[g]), int32_t(g));
    });
    build_csr(R, tb.up_off, tb.ups, [&](auto&& emit) {
        for (size_t u = 0; u < R; ++u)
            if (river_downstream[u] >= 0) emit(size_t(river_downstream[u]), int32_t(u));
    });
    // network levels: level(r) = 1 + max level of its upstream rivers (sources are level 0)
    std::vector<int32_t> level(R, -1);
    for (size_t pass = 0; pass <= R; ++pass) {
        bool changed = false;
        for (size_t r = 0; r < R; ++r) {
            int32_t lv = 0;
            bool ready = true;
            for (int32_t k = tb.up_off[r]; k < tb.up_off[r + 1]; ++k) {
                const int32_t ul = level[size_t(tb.ups[size_t(k)])];
                if (ul < 0) { ready = false; break; }
                lv = std::max(lv, ul + 1);
            }
            if (ready && level[r] != lv) { level[r] = lv; changed = true; }
        }
        if (!changed) break;
    }
    int32_t n_levels = 0;
    for (size_t r = 0; r < R; ++r) {
        if (level[r] < 0) return false;
        n_levels = std::max(n_levels, level[r] + 1);
    }
    build_csr(size_t(n_levels), tb.lvl_off, tb.lvl_rivers, [&](auto&& emit) {
        for (size_t r = 0; r < R; ++r) emit(size_t(level[r]), int32_t(r));
    });
    return true;
}

// UTC civil calendar (core/utctime_utilities.cpp:230-253): the proleptic Gregorian days <-> (year, month, day) maps
// in closed form, on days since 1970-01-01. Exact for every instant an int64 microsecond count can hold.
inline int64_t floor_div(int64_t a, int64_t b) {
    int64_t q = a / b;
    if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
    return q;
}
inline void civil_from_days(int64_t z, int64_t& y, int& m, int& d) {
    z += 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const int64_t doe = z - era * 146097;
    const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    y = yoe + era * 400;
    const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const int64_t mp = (5 * doy + 2) / 153;
    d = int(doy - (153 * mp + 2) / 5 + 1);
    m = int(mp < 10 ? mp + 3 : mp - 9);
    y += (m <= 2);
}
inline int64_t days_from_civil(int64_t y, int m, int d) {
    y -= m <= 2;
    const int64_t era = (y >= 0 ? y : y - 399) / 400;
    const int64_t yoe = y - era * 400;
    const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
    const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + doe - 719468;
}
constexpr int64_t DAY_US = 86400LL * 1000000LL;

// calendar::day_of_year (UTC, core/utctime_utilities.cpp:230-235)
inline int day_of_year(int64_t t_us) {
    const int64_t days = floor_div(t_us, DAY_US);
    int64_t y;
    int m, d;
    civil_from_days(days, y, m, d);
    return int(1 + days - days_from_civil(y, 1, 1));
}

// Whether every step time t0_us + i * dt_us, i <= n, lies within +-2^62 us of 1970-01-01 (about +-146 000 years):
// there neither the step times nor the products of the calendar arithmetic leave int64. dt_us > 0, n >= 1.
inline bool year_tables_cover(int64_t t0_us, int64_t dt_us, size_t n) {
    constexpr int64_t LIM = int64_t(1) << 62;
    int64_t span, end;
    if (t0_us < -LIM || t0_us > LIM) return false;
    if (__builtin_mul_overflow(int64_t(n), dt_us, &span) || __builtin_add_overflow(t0_us, span, &end)) return false;
    return end <= LIM;
}

// The per-step calendar tables of pt_gs_k (gamma_snow.h:89-96) for the steps t0_us + i * dt_us, i < n:
// doy[i] = calendar::day_of_year(t), trel[i] = t - calendar::trim(t, YEAR). The axis passes year_tables_cover.
inline void build_year_tables(int64_t t0_us, int64_t dt_us, size_t n, int32_t* doy, int64_t* trel) {
    for (size_t i = 0; i < n; ++i) {
        const int64_t t = t0_us + int64_t(i) * dt_us;
        const int64_t days = floor_div(t, DAY_US);
        int64_t y;
        int m, d;
        civil_from_days(days, y, m, d);
        const int64_t jan1 = days_from_civil(y, 1, 1);
        doy[i] = int32_t(1 + days - jan1);  // calendar::day_of_year
        trel[i] = t - jan1 * DAY_US;        // t - calendar::trim(t, YEAR)
    }
}

}  // namespace shyft_hip_impl
