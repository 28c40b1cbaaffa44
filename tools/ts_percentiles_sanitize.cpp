// Memory-safety run of host/ts_percentiles.hpp (the percentiles of a vector of shifted views) on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off
//       -o ts_percentiles_sanitize tools/ts_percentiles_sanitize.cpp && ./ts_percentiles_sanitize
//
// It builds stored series in the shape of tests/resample_cases.py (lengths 0, 1, 2, 3, 63, 64, 65, 257, 1000, evenly
// spaced and irregular times, both point types, NaN, infinities and zeros of both signs among the values) and runs
// ts_percentiles over views of them with positive, negative and zero shifts: S in 1, 2, 5, 64, 65 and 300 views, axes
// of 1, 2, 5 and 65 intervals that lie on, inside, before, across the end of and wholly outside the series, and the
// percentile lists of the tests (empty, single entries, the extremes alone, values out of range, 40 entries). These
// are the batches where the indexes can go wrong: index_of and the single ++is of extract_statistics at both ends of
// a series, series without points, intervals without a finite sample (the plan reads no rank), a single sample, and
// the clamped upper rank. check_views refuses the batches the entry would refuse; they are counted and skipped. It
// prints the number of values computed; the sanitizers abort on any finding. Host code only: it is never loaded into
// Python and never runs on a GPU machine.
#include <cstdio>

#include "../shyft_amd/csrc/host/ts_percentiles.hpp"

using namespace shyft_hip::host;

namespace {

constexpr utctime HOUR = 3600 * US;
const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();

unsigned next(unsigned& seed) { return seed = seed * 1664525u + 1013904223u; }

point_ts series(size_t n, bool even, ts_point_fx fx, unsigned seed, utctime t0) {
    std::vector<utctime> t;
    std::vector<double> v;
    const double hazards[] = {NaN, INF, -INF, -0.0, 0.0, 1e-310, -1.7e308, -3.5};
    for (size_t i = 0; i < n; ++i) {
        t.push_back(t0 + utctime(i) * HOUR + (even || i == 0 ? 0 : utctime(next(seed) % unsigned(HOUR / 2))));
        const unsigned r = next(seed);
        if (r % 5 == 0) v.push_back(hazards[(r >> 8) % 8]);
        else v.push_back(double(int(r >> 16) % 200) / 10.0 - 10.0);
    }
    const utctime end = even ? t0 + utctime(n) * HOUR : (n ? t.back() + 1 + utctime(next(seed) % unsigned(HOUR)) : 0);
    return point_ts(std::move(t), end, std::move(v), fx);
}

}  // namespace

int main() {
    const size_t lengths[] = {0, 1, 2, 3, 63, 64, 65, 257, 1000};
    const utctime t0 = utctime(1451606400) * US;
    std::vector<point_ts> rows;
    std::vector<int64_t> row{0}, t, t_end;
    unsigned seed = 11;
    for (size_t k = 0; k < 18; ++k) {
        rows.push_back(series(lengths[k % 9], k % 2 == 0, ts_point_fx((k / 2) % 2), ++seed, t0));
        t.insert(t.end(), rows.back().t.begin(), rows.back().t.end());
        row.push_back(int64_t(t.size()));
        t_end.push_back(rows.back().t_end);
    }
    std::vector<std::vector<int64_t>> lists = {{}, {50}, {0, 100}, {-1}, {-1000, 1000}, {0, 10, 25, -1, 50, 75, 90, 100},
                                               {101, -2, 999}, {}};
    for (int k = 0; k < 36; ++k) lists.back().push_back((7 * k) % 101);
    for (int64_t p : {-1, -1000, 1000, 555}) lists.back().push_back(p);
    struct axis { utctime t0; utctimespan dt; };
    const axis axes[] = {{t0, HOUR}, {t0, 24 * HOUR}, {t0, HOUR / 4}, {t0 + HOUR / 4, HOUR}, {t0 - 2 * HOUR - HOUR / 2, HOUR},
                         {t0 - 3 * HOUR, HOUR}, {t0 + 60 * HOUR, HOUR}, {t0 - 70 * HOUR, HOUR}, {t0 + 1100 * HOUR, HOUR}};
    size_t computed = 0, refused = 0;
    for (size_t S : {size_t(1), size_t(2), size_t(5), size_t(64), size_t(65), size_t(300)}) {
        std::vector<int32_t> src(S);
        std::vector<int64_t> shift(S);
        for (size_t s = 0; s < S; ++s) {
            src[s] = int32_t((s + S) % rows.size());
            const unsigned r = next(seed);
            shift[s] = r % 3 == 0 ? 0 : (int64_t(r >> 8) % 200 - 100) * (HOUR / 2) + (r % 3 == 1 ? int64_t(r % 7) : 0);
        }
        for (size_t T : {size_t(1), size_t(2), size_t(5), size_t(65)})
            for (const axis& a : axes) {
                const fixed_dt ta(a.t0, a.dt, T);
                try {
                    check_views(rows.size(), row.data(), t.data(), t_end.data(), S, src.data(), shift.data(), ta);
                } catch (const std::runtime_error&) {
                    // a one-point series strictly inside a period: the same views with those series taken out
                    ++refused;
                    for (size_t s = 0; s < S; ++s)
                        if (rows[size_t(src[s])].size() == 1) src[s] = 0;
                    check_views(rows.size(), row.data(), t.data(), t_end.data(), S, src.data(), shift.data(), ta);
                }
                for (const auto& pct : lists) {
                    std::vector<double> out(pct.size() * T, 0.0);
                    ts_percentiles(rows, S, src.data(), shift.data(), ta, pct.data(), pct.size(), out.data());
                    volatile double sink = 0.0;
                    for (double x : out) sink = x;
                    (void)sink;
                    computed += out.size();
                }
            }
    }
    // the refusals themselves: a view outside the stored series, and a one-point series moved inside a period
    const int32_t bad_src[] = {int32_t(rows.size())};
    const int64_t no_shift[] = {0}, some_shift[] = {HOUR / 3};
    const int32_t one_point[] = {1};
    for (int k = 0; k < 2; ++k) {
        try {
            check_views(rows.size(), row.data(), t.data(), t_end.data(), 1, k ? one_point : bad_src, k ? some_shift : no_shift,
                        fixed_dt(t0 - HOUR, HOUR, 5));
            std::printf("ts_percentiles_sanitize: refusal %d did not happen\n", k);
            return 1;
        } catch (const std::runtime_error&) {
            ++refused;
        }
    }
    std::printf("ts_percentiles_sanitize: %zu values, %zu batches refused, no finding\n", computed, refused);
    return 0;
}
