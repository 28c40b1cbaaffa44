// Check of shyft_amd/csrc/include_internal/host_tables.h (the CSR builder, the river network tables and the calendar
// tables of pt_gs_k) on the CPU, under the address and undefined-behaviour sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o host_tables_check tools/host_tables_check.cpp && ./host_tables_check
//
// build_csr on a hand-made case with an empty key and a skipped item, on an identity and a non-identity input, with
// both offset types, with no keys, and with an enumeration that throws; build_river_tables on the 2-cycle, the 3-cycle
// and the 7-river network of tests/test_routing_edges.py, for one member and for two; build_year_tables (day of year
// and time since New Year of every step) against a day-by-day walk from 1970-01-01 that knows only the leap-year rule,
// on the axes of tests/time_axis_cases.py and on whole years around 1900, 1970, 2000, 2016, 2100 and 2400 at steps
// of 7 min + 1 us, 15 min, 1 h, 3 h and 24 h, with the range year_tables_cover accepts. It prints the number of checks
// and returns non-zero at the first that fails; the sanitizers abort on any finding. Host code only
// (tests/test_host_tables.py builds and runs it).
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "../shyft_amd/csrc/include_internal/host_tables.h"

using namespace shyft_hip_impl;

namespace {

int n_checks = 0;

template <class T>
void expect(const char* what, const std::vector<T>& got, std::vector<long long> want) {
    ++n_checks;
    bool ok = got.size() == want.size();
    for (size_t i = 0; ok && i < want.size(); ++i) ok = (long long)got[i] == want[i];
    if (ok) return;
    std::printf("FAILED %s: got", what);
    for (const T& v : got) std::printf(" %lld", (long long)v);
    std::printf("\n");
    std::exit(1);
}
void expect(const char* what, bool got, bool want) { expect(what, std::vector<int>{got}, {want}); }

template <class Off>
void csr_cases() {
    std::vector<Off> off;
    std::vector<int32_t> items;
    // keys of items 0..6; item 3 is skipped, key 1 stays empty; within a key the items keep their order
    const int key_of[7] = {2, 0, 2, -1, 3, 0, 2};
    bool id = build_csr(4, off, items, [&](auto&& emit) {
        for (int i = 0; i < 7; ++i)
            if (key_of[i] >= 0) emit(size_t(key_of[i]), int32_t(i));
    });
    expect("csr off", off, {0, 2, 2, 5, 6});
    expect("csr items", items, {1, 5, 0, 2, 6, 4});
    expect("csr identity", id, false);
    // contiguous keys in item order: the identity
    id = build_csr(3, off, items, [&](auto&& emit) {
        for (int i = 0; i < 6; ++i) emit(size_t(i / 2), int32_t(i));
    });
    expect("identity off", off, {0, 2, 4, 6});
    expect("identity items", items, {0, 1, 2, 3, 4, 5});
    expect("identity", id, true);
    // a skipped last item leaves a shorter identity: the caller compares the length
    id = build_csr(2, off, items, [&](auto&& emit) {
        emit(0, 0);
        emit(1, 1);
    });
    expect("short identity", id, true);
    expect("short identity items", items, {0, 1});
    // item i % 3: not the identity although every key has its items
    id = build_csr(3, off, items, [&](auto&& emit) {
        for (int i = 0; i < 6; ++i) emit(size_t(i % 3), int32_t(i));
    });
    expect("permuted items", items, {0, 3, 1, 4, 2, 5});
    expect("permuted identity", id, false);
    id = build_csr(0, off, items, [&](auto&&) {});
    expect("no keys off", off, {0});
    expect("no keys items", items, {});
    expect("no keys identity", id, true);
    bool thrown = false;
    try {
        build_csr(2, off, items, [&](auto&& emit) {
            emit(1, 0);
            throw std::runtime_error("refused");
        });
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    expect("enumeration throws", thrown, true);
}

template <class Off>
void network_cases() {
    river_tables<Off> tb;
    const int64_t one[2] = {0, 1};
    const int32_t on_river_0[1] = {0};
    const int32_t cycle2[3] = {1, 0, -1}, cycle3[4] = {1, 2, 0, 0};
    expect("2-cycle", build_river_tables(1, one, on_river_0, 3, cycle2, tb), false);
    expect("3-cycle", build_river_tables(1, one, on_river_0, 4, cycle3, tb), false);
    // 7 rivers on 4 levels: 0, 4, 6 -> 1 -> 5 -> 3, river 2 on its own
    const int32_t down[7] = {1, 5, -1, -1, 1, 3, 1};
    const int32_t group_river[12] = {0, 6, 1, 4, 0, 3, 2, 1, 3, 2, 1, 4};
    const int64_t all[2] = {0, 12};
    expect("tree", build_river_tables(1, all, group_river, 7, down, tb), true);
    expect("tree pair_off", tb.pair_off, {0, 2, 5, 7, 9, 11, 11, 12});
    expect("tree pair_groups", tb.pair_groups, {0, 4, 2, 7, 10, 6, 9, 5, 8, 3, 11, 1});
    expect("tree up_off", tb.up_off, {0, 0, 3, 3, 4, 4, 5, 5});
    expect("tree ups", tb.ups, {0, 4, 6, 5, 1});
    expect("tree lvl_off", tb.lvl_off, {0, 4, 5, 6, 7});
    expect("tree lvl_rivers", tb.lvl_rivers, {0, 2, 4, 6, 1, 5, 3});
    expect("tree levels", std::vector<int>{tb.n_levels()}, {4});
    // two members: rows [0, 5) and [5, 12); a (member, river) pair holds its member's rows only, ascending
    const int64_t two[3] = {0, 5, 12};
    expect("two members", build_river_tables(2, two, group_river, 7, down, tb), true);
    expect("two members pair_off", tb.pair_off, {0, 2, 3, 3, 3, 4, 4, 5, 5, 7, 9, 11, 12, 12, 12});
    expect("two members pair_groups", tb.pair_groups, {0, 4, 2, 3, 1, 7, 10, 6, 9, 5, 8, 11});
    expect("two members lvl_rivers", tb.lvl_rivers, {0, 2, 4, 6, 1, 5, 3});
    // a downstream below -1 is an outlet like -1 (shyft_hip_route takes it; route_members refuses it beforehand)
    const int32_t below[2] = {-5, 0};
    expect("downstream -5", build_river_tables(1, one, on_river_0, 2, below, tb), true);
    expect("downstream -5 ups", tb.ups, {1});
    expect("downstream -5 lvl_rivers", tb.lvl_rivers, {1, 0});
}

// ---- build_year_tables against a day-by-day walk ----
// The walk counts days forward and backward from 1970-01-01 (day 0 = day 1 of 1970) and knows only the leap-year
// rule; day k of the walk holds its year and its day of the year.
bool is_leap(int y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }

struct day_walk {
    static constexpr int Y0 = 1790, Y1 = 2510;  // years the walk covers: [Y0, Y1)
    std::vector<int32_t> year, doy;             // by day - first
    std::vector<int64_t> jan1_by_year;          // day number of Jan 1, by year - Y0 (Y1 included)
    int64_t first = 0;
    day_walk() {
        std::vector<int32_t> by, bd;  // the days before 1970, walking backward
        int64_t day = 0;
        jan1_by_year.assign(size_t(Y1 - Y0 + 1), 0);
        for (int y = 1969; y >= Y0; --y) {
            for (int d = is_leap(y) ? 366 : 365; d >= 1; --d) {
                by.push_back(y);
                bd.push_back(d);
                --day;
            }
            jan1_by_year[size_t(y - Y0)] = day;
        }
        first = day;
        year.assign(by.rbegin(), by.rend());
        doy.assign(bd.rbegin(), bd.rend());
        day = 0;
        for (int y = 1970; y < Y1; ++y) {
            jan1_by_year[size_t(y - Y0)] = day;
            for (int d = 1; d <= (is_leap(y) ? 366 : 365); ++d) {
                year.push_back(y);
                doy.push_back(d);
                ++day;
            }
        }
        jan1_by_year[size_t(Y1 - Y0)] = day;
    }
    int64_t jan1(int y) const { return jan1_by_year[size_t(y - Y0)]; }
};

constexpr int64_t US = 1000000LL, MIN_US = 60 * US, HOUR_US = 60 * MIN_US, D_US = 24 * HOUR_US;

void year_tables_axis(const day_walk& w, const char* what, int64_t t0, int64_t dt, size_t n) {
    ++n_checks;
    if (!year_tables_cover(t0, dt, n)) {
        std::printf("FAILED %s: year_tables_cover refuses the axis\n", what);
        std::exit(1);
    }
    std::vector<int32_t> doy(n);
    std::vector<int64_t> trel(n);
    build_year_tables(t0, dt, n, doy.data(), trel.data());
    for (size_t i = 0; i < n; ++i) {
        const int64_t t = t0 + int64_t(i) * dt;
        int64_t day = t / D_US;
        if (t % D_US < 0) --day;
        const size_t k = size_t(day - w.first);
        const int64_t want_trel = t - (day - (w.doy[k] - 1)) * D_US;
        if (doy[i] == w.doy[k] && trel[i] == want_trel) continue;
        std::printf("FAILED %s: step %zu (t = %lld us, year %d): doy %d, walk %d; trel %lld, walk %lld\n", what, i,
                    (long long)t, int(w.year[k]), int(doy[i]), int(w.doy[k]), (long long)trel[i], (long long)want_trel);
        std::exit(1);
    }
}

void year_table_cases() {
    const day_walk w;
    // the walk itself: 2015-01-01 is day 16436 (1420070400 s), 2000-03-01 is day 11017
    expect("walk 2015-01-01", std::vector<int64_t>{w.jan1(2015)}, {16436});
    expect("walk 2000-03-01", std::vector<int64_t>{w.jan1(2000) + 60}, {11017});
    expect("walk 1968 leap", std::vector<int64_t>{w.jan1(1969) - w.jan1(1968), w.jan1(2101) - w.jan1(2100)}, {366, 365});
    // the axes of tests/time_axis_cases.py
    const int64_t T0_2015 = w.jan1(2015) * D_US;
    year_tables_axis(w, "3h_leap", (w.jan1(2016) + 57) * D_US, 3 * HOUR_US, 32);
    year_tables_axis(w, "24h_year_end_leap", (w.jan1(2016) + 362) * D_US, D_US, 8);
    year_tables_axis(w, "1h_year_end_pre_epoch", (w.jan1(1967) + 364) * D_US + 12 * HOUR_US, HOUR_US, 24);
    year_tables_axis(w, "3h_pre_epoch_leap", (w.jan1(1968) + 58) * D_US, 3 * HOUR_US, 24);
    year_tables_axis(w, "15min_wed", T0_2015 + 98 * D_US + 22 * HOUR_US, 15 * MIN_US, 16);
    year_tables_axis(w, "odd_dt", T0_2015 + 12345678, 7 * MIN_US + 1, 60);
    year_tables_axis(w, "24h_2100", (w.jan1(2100) + 57) * D_US, D_US, 4);
    year_tables_axis(w, "24h_2000", (w.jan1(2000) + 57) * D_US, D_US, 4);
    // whole years around the century rule, the epoch and the leap years the tests use: every midnight and 1 us
    // before and after it (24 h steps from those three starts), and every finer step
    const int ranges[6][2] = {{1899, 1901}, {1967, 1972}, {1999, 2001}, {2015, 2017}, {2099, 2101}, {2399, 2401}};
    const int64_t dts[5] = {7 * MIN_US + 1, 15 * MIN_US, HOUR_US, 3 * HOUR_US, D_US};
    for (const auto& r : ranges)
        for (const int64_t dt : dts)
            for (const int64_t shift : {int64_t(0), int64_t(-1), int64_t(1)}) {
                const int64_t t0 = w.jan1(r[0]) * D_US + shift;
                const int64_t t1 = w.jan1(r[1] + 1) * D_US;
                char what[96];
                std::snprintf(what, sizeof what, "years %d-%d dt %lld us shift %lld", r[0], r[1], (long long)dt,
                              (long long)shift);
                year_tables_axis(w, what, t0, dt, size_t((t1 - t0) / dt) + 1);
            }
    // day_of_year is the same map (btk_prior_gradient uses it)
    expect("day_of_year", std::vector<int>{day_of_year(-1), day_of_year(0), day_of_year((w.jan1(2016) + 365) * D_US),
                                           day_of_year((w.jan1(2100) + 59) * D_US), day_of_year(w.jan1(1900) * D_US - 1)},
           {365, 1, 366, 60, 365});
    // the range the tables cover: step times within +-2^62 us, without overflow on the way
    const int64_t LIM = int64_t(1) << 62;
    expect("cover at the limit", year_tables_cover(LIM - 10, 1, 10), true);
    expect("cover past the limit", year_tables_cover(LIM - 10, 1, 11), false);
    expect("cover below the limit", year_tables_cover(-LIM - 1, 1, 1), false);
    expect("cover span overflow", year_tables_cover(0, INT64_MAX / 2, 5), false);
    expect("cover end overflow", year_tables_cover(LIM, LIM, 1), false);
    // at the ends of that range the closed form still agrees with itself: trel in [0, 366 days), doy from trel
    for (const int64_t t0 : {-LIM, LIM - 3 * D_US}) {
        int32_t doy[4];
        int64_t trel[4];
        build_year_tables(t0, D_US, 3, doy, trel);
        for (int i = 0; i < 3; ++i)
            expect("far instants", trel[i] >= 0 && trel[i] < 366 * D_US && doy[i] == 1 + trel[i] / D_US, true);
    }
}

}  // namespace

int main() {
    csr_cases<int32_t>();
    csr_cases<int64_t>();
    network_cases<int32_t>();
    network_cases<int64_t>();
    year_table_cases();
    std::printf("host_tables_check: %d checks passed\n", n_checks);
    return 0;
}
