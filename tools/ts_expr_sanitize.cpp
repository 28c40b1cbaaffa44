// Memory-safety run of host/ts_expr.hpp (the planner, the program check and the interpreter) on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off
//       -o ts_expr_sanitize tools/ts_expr_sanitize.cpp && ./ts_expr_sanitize
//
// It builds the expression shapes and axis pairs of tests/ts_expr_cases.py (each operation in its three forms, abs,
// unary minus, a + b*3.0 - a/2.0, (a*b) + c on a foreign axis, right-deep chains of depth 8 and 9, a shifted operand;
// identical, other t_end, disjoint, touching, nested, interleaved, one point differs, one point, empty), with NaN,
// infinities and -0.0 among the values, plans every tree, checks every program and interprets it at every point.
// It prints the number of values computed; the sanitizers abort on any finding. Host code only: it is never loaded
// into Python and never runs on a GPU machine.
#include <cstdio>
#include <functional>

#include "../shyft_amd/csrc/host/ts_expr.hpp"

using namespace shyft_hip::host;
namespace hx = shyft_hip::host::expr;

namespace {

constexpr utctime HOUR = 3600 * US;
const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();

point_ts series(std::vector<double> hours, double end, ts_point_fx fx, unsigned seed) {
    std::vector<utctime> t;
    std::vector<double> v;
    const double hazards[] = {NaN, INF, -INF, -0.0, 0.0};
    for (size_t i = 0; i < hours.size(); ++i) {
        t.push_back(utctime(hours[i] * double(HOUR)));
        seed = seed * 1664525u + 1013904223u;
        v.push_back(seed % 7 == 0 ? hazards[(seed >> 8) % 5] : double(int(seed >> 16) % 200) / 10.0 - 10.0);
    }
    return point_ts(std::move(t), utctime(end * double(HOUR)), std::move(v), fx);
}

// a tree under construction: nodes in child-before-parent order
struct builder {
    hx::tree tr;
    int32_t term(int32_t k) { return add({hx::TERMINAL, 0, k, 0, 0.0}); }
    int32_t bin(int32_t op, int32_t a, int32_t b) { return add({hx::TS_TS, op, a, b, 0.0}); }
    int32_t ts_s(int32_t op, int32_t a, double s) { return add({hx::TS_S, op, a, 0, s}); }
    int32_t s_ts(int32_t op, double s, int32_t a) { return add({hx::S_TS, op, a, 0, s}); }
    int32_t abs(int32_t a) { return add({hx::ABS_TS, 0, a, 0, 0.0}); }
    int32_t add(hx::node n) {
        tr.nodes.push_back(n);
        return int32_t(tr.nodes.size() - 1);
    }
};

// the shapes over the terminals a = 0, b = 1, c = 2, a2 = 3 (a's axis), b shifted = 4
std::vector<hx::tree> shapes() {
    std::vector<hx::tree> out;
    auto make = [&](const std::function<void(builder&)>& f) {
        builder b;
        f(b);
        out.push_back(b.tr);
    };
    for (int32_t op = 0; op < hx::N_OPS; ++op) {
        make([&](builder& x) { x.bin(op, x.term(0), x.term(1)); });
        make([&](builder& x) { x.bin(op, x.term(0), x.term(3)); });
        make([&](builder& x) { x.ts_s(op, x.term(0), 2.5); });
        make([&](builder& x) { x.s_ts(op, 2.5, x.term(0)); });
        make([&](builder& x) { x.bin(hx::OP_ADD, x.s_ts(op, 2.5, x.term(0)), x.term(1)); });
    }
    make([](builder& x) { x.abs(x.term(0)); });
    make([](builder& x) { x.abs(x.bin(hx::OP_SUB, x.term(0), x.term(1))); });
    make([](builder& x) { x.s_ts(hx::OP_MUL, -1.0, x.term(0)); });
    make([](builder& x) {
        x.bin(hx::OP_SUB, x.bin(hx::OP_ADD, x.term(0), x.ts_s(hx::OP_MUL, x.term(1), 3.0)), x.ts_s(hx::OP_DIV, x.term(0), 2.0));
    });
    make([](builder& x) { x.bin(hx::OP_ADD, x.bin(hx::OP_MUL, x.term(0), x.term(1)), x.term(2)); });
    make([](builder& x) { x.bin(hx::OP_ADD, x.bin(hx::OP_MUL, x.term(0), x.term(3)), x.term(2)); });
    make([](builder& x) { x.bin(hx::OP_MUL, x.term(0), x.term(4)); });
    for (int depth : {8, 9})
        for (int values = 0; values < 2; ++values)
            make([&](builder& x) {
                const int32_t order[] = {0, 1, 2, 3};
                std::vector<int32_t> leaves;
                for (int i = 0; i < depth; ++i) leaves.push_back(x.term(values ? (i % 2 ? 3 : 0) : order[i % 4]));
                int32_t r = leaves.back();
                for (int i = depth - 2; i >= 0; --i) r = x.bin(hx::OP_ADD, leaves[size_t(i)], r);
            });
    return out;
}

}  // namespace

int main() {
    const std::vector<double> p{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    struct pair_t { const char* name; std::vector<double> a; double ea; std::vector<double> b; double eb; };
    const std::vector<pair_t> pairs{
        {"identical", p, 12, p, 12}, {"other_t_end", p, 12, p, 13}, {"disjoint", p, 12, {20, 21, 22}, 23},
        {"touching", p, 12, {12, 13, 14}, 15}, {"nested", p, 12, {3, 4, 5, 6}, 7},
        {"nested_between_points", {0, 4, 8}, 12, {5, 6, 7}, 10}, {"interleaved", {0, 2, 4, 6, 8}, 10, {1, 3, 5, 7, 9}, 11},
        {"one_differs", p, 12, {0, 1, 2, 3, 4, 5.5, 6, 7, 8, 9, 10, 11}, 12}, {"ends_on_a_point", p, 12, {2, 3, 4}, 6},
        {"one_point", p, 12, {4}, 5}, {"one_point_both", {4}, 6, {4}, 6}, {"empty", p, 12, {}, 0}, {"empty_both", {}, 0, {}, 0}};
    const std::vector<hx::tree> trees = shapes();
    size_t computed = 0, programs = 0;
    unsigned seed = 1;
    for (const pair_t& pr : pairs)
        for (int fxs = 0; fxs < 4; ++fxs) {
            const ts_point_fx fa = ts_point_fx(fxs & 1), fb = ts_point_fx(fxs >> 1);
            std::vector<point_ts> ts{series(pr.a, pr.ea, fa, ++seed), series(pr.b, pr.eb, fb, ++seed),
                                     series({1.5, 2.5, 6.25, 9}, 30, POINT_INSTANT_VALUE, ++seed),
                                     series(pr.a, pr.ea, fa, ++seed), series(pr.b, pr.eb, fb, ++seed)};
            for (auto& x : ts[4].t) x += HOUR / 2;  // b, half an hour later
            ts[4].t_end += HOUR / 2;
            // the CSR form of the terminals
            std::vector<int64_t> row{0}, t, t_end;
            std::vector<double> v;
            std::vector<int32_t> fx;
            std::vector<hx::terminal> terminals;
            for (const point_ts& s : ts) {
                t.insert(t.end(), s.t.begin(), s.t.end());
                v.insert(v.end(), s.v.begin(), s.v.end());
                row.push_back(int64_t(t.size()));
                t_end.push_back(s.t_end);
                fx.push_back(int32_t(s.fx));
                terminals.push_back({hx::axis{s.t, s.t_end}, s.fx});
            }
            hx::tables tb;
            std::vector<hx::plan> plans;
            for (const hx::tree& tr : trees) plans.push_back(hx::make_plan(tr, terminals, tb));
            const hx::batch b{ts.size(), row.data(), t.data(), v.data(), t_end.data(), fx.data(), tb.consts.size(),
                              tb.consts.data(), tb.periods.size() / 2, tb.periods.data()};
            std::vector<double> stack;
            for (const hx::plan& pl : plans) {
                const int depth = hx::check_program(b, pl.prog.data(), pl.prog.size(), pl.ta.size());
                if (depth != pl.depth) {
                    std::fprintf(stderr, "%s: the planner reports depth %d, the check %d\n", pr.name, pl.depth, depth);
                    return 1;
                }
                ++programs;
                for (size_t i = 0; i < pl.ta.size(); ++i) {
                    volatile double r = hx::run_program(b, pl.prog.data(), pl.prog.size(), i, pl.ta.t[i], stack);
                    (void)r;
                    ++computed;
                }
            }
        }
    std::printf("ts_expr_sanitize: %zu programs, %zu values, no finding\n", programs, computed);
    return 0;
}
