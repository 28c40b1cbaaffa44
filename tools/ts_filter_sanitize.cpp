// Memory-safety run of host/ts_filter.hpp (convolve_w, derivative, inside, decode) on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off
//       -o ts_filter_sanitize tools/ts_filter_sanitize.cpp && ./ts_filter_sanitize
//
// It builds a batch in the shape of tests/resample_cases.py (lengths 0, 1, 2, 3, 63, 64, 65, 257, 1000, evenly spaced
// and irregular times, both point types, NaN and infinities among the values) and runs the four computations of the
// _host entries on every point of it: convolve_w for 0, 1, 5, 65 and 1500 weights (more than any series has points)
// under the three policies, because of its i - j indexing; derivative for the four methods on both branches; inside;
// and decode for every legal (start_bit, n_bits) pair on values up to and beyond 2^52, because of its shifts, with the
// argument check on the pairs around the limits. It prints the number of values computed; the sanitizers abort on any
// finding. Host code only: it is never loaded into Python and never runs on a GPU machine.
#include <cstdio>

#include "../shyft_amd/csrc/host/ts_filter.hpp"

using namespace shyft_hip::host;

namespace {

constexpr utctime HOUR = 3600 * US;
const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();

unsigned next(unsigned& seed) { return seed = seed * 1664525u + 1013904223u; }

point_ts series(size_t n, bool even, ts_point_fx fx, unsigned seed, bool for_decode) {
    std::vector<utctime> t;
    std::vector<double> v;
    const double hazards[] = {NaN, INF, -INF, -0.0, 0.0, 4503599627370496.0, 4503599627370498.0, -3.5};
    for (size_t i = 0; i < n; ++i) {
        t.push_back(utctime(i) * HOUR + (even || i == 0 ? 0 : utctime(next(seed) % unsigned(HOUR / 2))));
        const unsigned r = next(seed);
        if (r % 7 == 0) v.push_back(hazards[(r >> 8) % 8]);
        else if (for_decode) v.push_back(double((uint64_t(r) << (r % 21)) | next(seed)) + (r % 3 ? 0.0 : 0.25));
        else v.push_back(double(int(r >> 16) % 200) / 10.0 - 10.0);
    }
    const utctime end = even ? utctime(n) * HOUR : (n ? t.back() + 1 + utctime(next(seed) % unsigned(HOUR)) : 0);
    point_ts ts(std::move(t), end, std::move(v), fx);
    ts.fixed_step = even ? HOUR : 0;
    return ts;
}

}  // namespace

int main() {
    const size_t lengths[] = {0, 1, 2, 3, 63, 64, 65, 257, 1000};
    size_t computed = 0, refused = 0;
    unsigned seed = 7;
    for (size_t k = 0; k < 18; ++k) {
        const point_ts ts = series(lengths[k % 9], k % 2 == 0, ts_point_fx((k / 2) % 2), ++seed, false);
        for (size_t K : {size_t(0), size_t(1), size_t(5), size_t(65), size_t(1500)}) {
            std::vector<double> w(K);
            for (size_t j = 0; j < K; ++j) w[j] = next(seed) % 5 == 0 ? 0.0 : double(int(next(seed) >> 20) % 100) / 50.0 - 1.0;
            if (K > 2) w[K / 2] = NaN;
            for (int policy = 0; policy < 3; ++policy)
                for (size_t i = 0; i < ts.size(); ++i) {
                    volatile double r = convolve_w_value(ts, w.data(), K, convolve_policy(policy), i);
                    (void)r;
                    ++computed;
                }
        }
        for (int fx = 0; fx < 2; ++fx) {
            point_ts d = ts;
            d.fx = ts_point_fx(fx);
            for (int method = 0; method < 4; ++method)
                for (utctimespan dt : {d.fixed_step, utctimespan(0)})
                    for (size_t i = 0; i < d.size(); ++i) {
                        volatile double r = derivative_value(d, dt, derivative_method(method), i);
                        (void)r;
                        ++computed;
                    }
        }
        inside_parameter p;
        p.min_x = k % 3 ? -2.0 : NaN;
        p.max_x = k % 2 ? 5.0 : NaN;
        for (size_t i = 0; i < ts.size(); ++i) {
            volatile double r = p.inside_value(ts.v[i]);
            (void)r;
            ++computed;
        }
        const point_ts codes = series(lengths[k % 9], true, POINT_AVERAGE_VALUE, ++seed, true);
        for (int start_bit = -1; start_bit <= 52; ++start_bit)
            for (int n_bits : {-1, 0, 1, 2, 25, 50, 51, 52, std::numeric_limits<int>::max()}) {
                try {
                    check_decode_arguments(start_bit, n_bits);
                } catch (const std::runtime_error&) {
                    ++refused;
                    continue;
                }
                const bit_decoder dec{unsigned(start_bit), unsigned(n_bits)};
                for (size_t i = 0; i < codes.size(); ++i) {
                    volatile double r = dec.decode(codes.v[i]);
                    (void)r;
                    ++computed;
                }
            }
    }
    std::printf("ts_filter_sanitize: %zu values, %zu argument pairs refused, no finding\n", computed, refused);
    return 0;
}
