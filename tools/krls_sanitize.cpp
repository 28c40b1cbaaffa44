// Memory-safety run of host/krls.hpp (the KRLS predictor) on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off
//       -o krls_sanitize tools/krls_sanitize.cpp && ./krls_sanitize
//
// It trains predictors over series of 0, 1, 2, 9, 65, 130 and 300 points with NaN holes in the grow-only and the mixed
// setting, so that the matrices are reallocated several times and both branches run; with max_dict_size 1, 2 and 8, so
// that entries are removed from dictionaries of every small size; with offset, count and stride around the ends of the
// series (krls_dim's saturation); over several iterations; from a state exported by get_state and taken back by
// set_state; and it evaluates predict_vec, the scalar predict, predictor_mse and mse_ts with windows of 0, 3 and more
// points than the series has. It prints the number of values computed; the sanitizers abort on any finding. Host code
// only: it is never loaded into Python and never runs on a GPU machine.
#include <cstdio>

#include "../shyft_amd/csrc/host/krls.hpp"

using namespace shyft_hip::host;

namespace {

constexpr utctime HOUR = 3600 * US;
unsigned next(unsigned& seed) { return seed = seed * 1664525u + 1013904223u; }

point_ts series(size_t n, unsigned seed) {
    std::vector<utctime> t;
    std::vector<double> v;
    for (size_t i = 0; i < n; ++i) {
        t.push_back(utctime(i) * HOUR);
        const unsigned r = next(seed);
        v.push_back(r % 7 == 0 ? std::numeric_limits<double>::quiet_NaN() : double(int(r >> 16) % 200) / 100.0 - 1.0);
    }
    return point_ts(std::move(t), utctime(n) * HOUR, std::move(v), POINT_INSTANT_VALUE);
}

size_t use(const krls_rbf_predictor& p, const point_ts& ts) {
    size_t count = 0;
    double sink = 0.0;
    for (double x : p.predict(ts).v) sink += x, ++count;
    if (ts.size()) sink += p.predict(ts.t[ts.size() / 2]), ++count;
    for (size_t points : {size_t(0), size_t(3), ts.size() + 5, size_t(-1)})
        for (double x : p.mse_ts(ts, points).v) sink += x == x ? x : 0.0, ++count;
    for (size_t offset : {size_t(0), size_t(1), ts.size(), ts.size() + 3})
        for (int64_t c : {int64_t(-1), int64_t(0), int64_t(2), std::numeric_limits<int64_t>::max()})
            for (size_t stride : {size_t(1), size_t(3), size_t(1) << 62}) sink += p.predictor_mse(ts, offset, c, stride), ++count;
    if (sink != sink) std::printf("(a NaN among the sums)\n");
    return count;
}

}  // namespace

int main() {
    size_t count = 0;
    unsigned seed = 1;
    for (size_t n : {0, 1, 2, 9, 65, 130, 300}) {
        const point_ts ts = series(n, next(seed));
        for (int setting = 0; setting < 2; ++setting) {
            const utctimespan dt = setting ? 3 * HOUR : HOUR;
            const double gamma = setting ? 1e-3 : 0.5, tol = setting ? 0.01 : 0.001;
            for (size_t size : {size_t(1000000), size_t(1), size_t(2), size_t(8)}) {
                krls_rbf_predictor p(dt, gamma, tol, size);
                p.train(ts);
                count += use(p, ts);
                p.train(ts, 0, -1, 1, 3, 0.0);  // a trained predictor, several passes
                for (size_t offset : {size_t(0), size_t(2), n, n + 1})
                    for (int64_t c : {int64_t(-1), int64_t(0), int64_t(3), std::numeric_limits<int64_t>::max()})
                        for (size_t stride : {size_t(1), size_t(4), size_t(1) << 61}) p.train(ts, offset, c, stride);
                count += use(p, ts);
                const size_t m = p.dictionary_size();
                std::vector<double> d(m), alpha(m), Kinv(m * m), P(m * m);
                p.get_state(d.data(), alpha.data(), Kinv.data(), P.data());
                krls_rbf_predictor q(dt, gamma, tol, size);
                q.set_state(m, d.data(), alpha.data(), Kinv.data(), P.data());
                q.train(ts);
                count += use(q, ts);
                q.clear();
                count += use(q, ts);
            }
        }
    }
    std::printf("krls_sanitize: %zu values, no finding\n", count);
    return 0;
}
