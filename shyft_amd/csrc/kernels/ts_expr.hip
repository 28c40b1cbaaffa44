// Time-series arithmetic for gfx950: E expressions over S terminal point series, every point of every expression in one
// launch. host/ts_expr.hpp states the semantics (the reference's lazy apoint_ts expressions), plans an expression tree
// into a postfix program and interprets such programs on one thread; that interpreter is the definition of correct and
// is what shyft_hip_ts_expr_host runs. This file evaluates the same programs on the device, bit for bit.
//
// The terminals come in the CSR form of shyft_hip_resample: row [S+1], t and v [row[S]] (int64 microseconds, values),
// t_end [S], fx [S]. Expression e has the program prog[prog_row[e] .. prog_row[e+1]) and the output points
// orow[e] .. orow[e+1) with times ot; consts and periods are the tables the programs index.
//
// te_kernel: one lane per output point, one wavefront per 64 consecutive points of one expression (wrow [E+1] counts
// the wavefronts of the expressions before e; a wavefront finds its expression by a search over it). The expression
// index goes through readfirstlane, so the program words, the program counter and the stack pointer live in scalar
// registers and every lane of the wavefront executes the same word. LOAD_RAW is a coalesced load of 64 neighbouring
// values; LOAD_AT is an upper_bound over the terminal's points per lane, then f(t). The top of the evaluation stack is
// a register, the rest a per-lane column of LDS, stk[depth][lane of the workgroup]: 8 x 256 doubles = 16 KB per
// workgroup, indexed by the wave-uniform stack pointer, never a private array. A lane touches only its own column, so
// there is no barrier, no atomic and no cross-lane operation, and no wavefront waits for another.
//
// Every operation is evaluated as written: int64 tick arithmetic, to_seconds(x) = double(x) / 1e6 as a division, no
// FMA (-ffp-contract=off), isfinite by the exponent bits, MAX / MIN as the comparisons of std::max / std::min, pow
// from detmath.
//
// Index safety. Before any launch the host checks (host/ts_expr.hpp check_program, series_args.h): row, prog_row and
// orow start at 0 and do not decrease, so row[S] points, prog_row[E] words and orow[E] output points were uploaded;
// times increase strictly in a terminal and t_end lies after the last; every program consists of known words that end
// at prog_row[e+1], with operation, terminal, constant and period indexes inside their tables; the stack never
// underflows, ends at depth 1 and is at most TE_DEPTH deep, so LDS rows 0 .. TE_DEPTH - 2 are the only ones touched;
// a LOAD_RAW names a terminal with exactly as many points as the expression, so v[row[term] + i] with i below the
// expression's point count is the terminal's own. A wavefront w < W = wrow[E] finds the e < E with wrow[e] <= w <
// wrow[e+1], and a lane works only when its point orow[e] + i lies below orow[e+1]. te_at reads points 0 .. n - 1 of
// its terminal only: point i + 1 after the test i + 1 < n; its search (first_false, device/workgroup.h) asks about
// points below n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../detmath/detmath.h"
#include "../device/csr_series.h"
#include "../device/ts_area.h"
#include "../host/ts_expr.hpp"
#include "../include_internal/device_call.h"
#include "../include_internal/series_args.h"

using namespace shyft_hip_impl;
namespace hx = shyft_hip::host::expr;

namespace {

constexpr int TE_BLOCK = 256;  // 4 wavefronts
constexpr int TE_WAVES = TE_BLOCK / 64;
constexpr int TE_DEPTH = hx::DEVICE_STACK_DEPTH;
constexpr int TE_WORDS = hx::DEVICE_PROGRAM_WORDS;

struct te_args {
    int64_t W;  // wavefronts of work
    int32_t E;
    const int64_t* row;
    const int64_t* t;
    const double* v;
    const int64_t* t_end;
    const int32_t* fx;
    const int64_t* prog_row;
    const int32_t* prog;
    const double* consts;
    const int64_t* periods;
    const int64_t* orow;
    const int64_t* ot;
    const int64_t* wrow;
    double* out;
};

// do_op of host/ts_expr.hpp
__device__ inline double te_op(double a, int32_t op, double b) {
    switch (op) {
    case hx::OP_ADD: return a + b;
    case hx::OP_SUB: return a - b;
    case hx::OP_MUL: return a * b;
    case hx::OP_DIV: return a / b;
    case hx::OP_MAX: return a < b ? b : a;
    case hx::OP_MIN: return b < a ? b : a;
    default: return detmath::pow(a, b);  // OP_POW; the host refused any other
    }
}

// value_at of host/ts_expr.hpp over the n points t, v of one terminal
__device__ inline double te_at(const int64_t* __restrict__ t, const double* __restrict__ v, int64_t n, int64_t t_end,
                               int32_t fx, int64_t tx) {
    if (n == 0 || tx < t[0] || tx >= t_end) return rs_nan();
    int64_t i = n - 1;
    if (tx < t[n - 1]) {  // upper_bound - 1; t[0] <= tx < t[n-1]
        i = first_false(int64_t(0), n, [&](int64_t m) { return t[m] <= tx; }) - 1;
    }
    const double vi = v[i];
    if (fx == int32_t(shyft_hip::host::POINT_INSTANT_VALUE) && i + 1 < n) {
        const double v2 = v[i + 1];
        if (rs_finite(v2)) {
            const int64_t t1 = t[i], t2 = t[i + 1];
            const double f = rs_seconds(t2 - tx) / rs_seconds(t2 - t1);
            return vi * f + (1.0 - f) * v2;
        }
    }
    return vi;
}

__global__ __launch_bounds__(TE_BLOCK) void te_kernel(te_args a) {
    __shared__ double stk[TE_DEPTH][TE_BLOCK];
    const int tid = int(threadIdx.x), lane = tid & 63;
    const int64_t stride = int64_t(gridDim.x) * TE_WAVES;
    for (int64_t w = int64_t(blockIdx.x) * TE_WAVES + (tid >> 6); w < a.W; w += stride) {
        const int32_t e = __builtin_amdgcn_readfirstlane(csr_series_of(a.wrow, a.E, w));
        const int64_t o0 = a.orow[e], o1 = a.orow[e + 1];
        const int64_t i = (w - a.wrow[e]) * 64 + lane;  // the point of the expression
        if (o0 + i >= o1) continue;
        const int64_t tx = a.ot[o0 + i];
        const int64_t p1 = a.prog_row[e + 1];
        double top = rs_nan();
        int sp = 0;  // values on the stack: stk[0 .. sp - 2] and top
        for (int64_t p = a.prog_row[e]; p < p1;) {
            const int32_t code = a.prog[p];
            if (code == hx::LOAD_RAW || code == hx::LOAD_AT) {
                const int32_t s = a.prog[p + 1];
                const int64_t r0 = a.row[s];
                if (sp > 0) stk[sp - 1][tid] = top;
                ++sp;
                if (code == hx::LOAD_RAW) top = a.v[r0 + i];
                else top = te_at(a.t + r0, a.v + r0, a.row[s + 1] - r0, a.t_end[s], a.fx[s], tx);
                p += 2;
            } else if (code == hx::ABS) {
                top = __builtin_fabs(top);
                p += 1;
            } else if (code == hx::BIN || code == hx::BIN_PERIOD) {
                --sp;
                top = te_op(stk[sp - 1][tid], a.prog[p + 1], top);
                if (code == hx::BIN_PERIOD) {
                    const int64_t* q = a.periods + 2 * int64_t(a.prog[p + 2]);
                    if (!(tx >= q[0] && tx < q[1])) top = rs_nan();
                    p += 3;
                } else {
                    p += 2;
                }
            } else if (code == hx::TS_SCALAR) {
                top = te_op(top, a.prog[p + 1], a.consts[a.prog[p + 2]]);
                p += 3;
            } else {  // SCALAR_TS
                top = te_op(a.consts[a.prog[p + 2]], a.prog[p + 1], top);
                p += 3;
            }
        }
        a.out[o0 + i] = top;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct te_checked {
    bool nothing = true;  // no expression or no output point
    int depth = 0;        // the deepest stack of the batch
    int64_t words = 0;    // the longest program of the batch
    hx::batch b;
};

// The argument checks that the device entry and its host twin share.
te_checked te_prepare(const char* who, size_t S, const int64_t* row, const int64_t* t, const double* v,
                      const int64_t* t_end, const int32_t* fx, size_t E, const int64_t* prog_row, const int32_t* prog,
                      size_t n_const, const double* consts, size_t n_period, const int64_t* periods, const int64_t* orow,
                      const int64_t* ot, double* out) {
    te_checked c;
    if (E == 0) return c;
    const std::string null_text = std::string(who) + ": null argument";
    if (S > 0) check_point_series(who, "ts_expr", S, row, t, v, t_end, fx);
    if (!prog_row || !orow) throw std::runtime_error(null_text);
    check_csr_rows("ts_expr", E, prog_row);
    check_csr_rows("ts_expr", E, orow);
    if ((prog_row[E] > 0 && !prog) || (n_const > 0 && !consts) || (n_period > 0 && !periods) ||
        (orow[E] > 0 && (!ot || !out)))
        throw std::runtime_error(null_text);
    if (S > size_t(std::numeric_limits<int32_t>::max()) || E > size_t(std::numeric_limits<int32_t>::max()))
        throw std::runtime_error("ts_expr: more than 2^31 - 1 terminals or expressions are not supported");
    const int64_t quarter_min = std::numeric_limits<int64_t>::min() / 4, quarter_max = std::numeric_limits<int64_t>::max() / 4;
    for (int64_t k = 0; k < orow[E]; ++k)
        if (ot[k] < quarter_min || ot[k] > quarter_max)
            throw std::runtime_error("ts_expr: times beyond a quarter of the 64-bit range are not supported");
    c.b = hx::batch{S, row, t, v, t_end, fx, n_const, consts, n_period, periods};
    for (size_t e = 0; e < E; ++e) {
        const int64_t words = prog_row[e + 1] - prog_row[e];
        c.depth = std::max(c.depth, hx::check_program(c.b, prog + prog_row[e], size_t(words), size_t(orow[e + 1] - orow[e])));
        c.words = std::max(c.words, words);
    }
    c.nothing = orow[E] == 0;
    return c;
}

call_record g_te;
constexpr const char* TE_UPLOAD = "ts_expr upload";

}  // namespace

extern "C" {

int shyft_hip_ts_expr(int device, size_t S, const int64_t* row, const int64_t* t, const double* v, const int64_t* t_end,
                      const int32_t* fx, size_t E, const int64_t* prog_row, const int32_t* prog, size_t n_const,
                      const double* consts, size_t n_period, const int64_t* periods, const int64_t* orow,
                      const int64_t* ot, double* out) {
    try {
        const te_checked ck = te_prepare("shyft_hip_ts_expr", S, row, t, v, t_end, fx, E, prog_row, prog, n_const, consts,
                                         n_period, periods, orow, ot, out);
        if (ck.depth > TE_DEPTH)
            throw std::runtime_error("ts_expr: an evaluation stack of " + std::to_string(ck.depth) +
                                     " values is deeper than the device's " + std::to_string(TE_DEPTH) +
                                     "; shyft_hip_ts_expr_host evaluates it");
        if (ck.words > TE_WORDS)
            throw std::runtime_error("ts_expr: a program of " + std::to_string(ck.words) +
                                     " words is longer than the device's " + std::to_string(TE_WORDS) +
                                     "; shyft_hip_ts_expr_host evaluates it");
        if (ck.nothing) return 0;
        std::vector<int64_t> wrow(E + 1, 0);
        for (size_t e = 0; e < E; ++e) wrow[e + 1] = wrow[e] + (orow[e + 1] - orow[e] + 63) / 64;
        const int64_t W = wrow[E];
        device_call c(device);
        const size_t np = S ? size_t(row[S]) : 0, no = size_t(orow[E]);
        dbuf<int64_t> d_row, d_t, d_tend, d_prog_row, d_periods, d_orow, d_ot, d_wrow;
        dbuf<double> d_v, d_consts, d_out;
        dbuf<int32_t> d_fx, d_prog;
        c.upload(d_row, row, S ? S + 1 : 0, TE_UPLOAD);
        c.upload(d_t, t, np, TE_UPLOAD);
        c.upload(d_v, v, np, TE_UPLOAD);
        c.upload(d_tend, t_end, S, TE_UPLOAD);
        c.upload(d_fx, fx, S, TE_UPLOAD);
        c.upload(d_prog_row, prog_row, E + 1, TE_UPLOAD);
        c.upload(d_prog, prog, size_t(prog_row[E]), TE_UPLOAD);
        c.upload(d_consts, consts, n_const, TE_UPLOAD);
        c.upload(d_periods, periods, 2 * n_period, TE_UPLOAD);
        c.upload(d_orow, orow, E + 1, TE_UPLOAD);
        c.upload(d_ot, ot, no, TE_UPLOAD);
        c.upload(d_wrow, wrow.data(), E + 1, TE_UPLOAD);
        d_out.alloc(no);
        te_args a{W, int32_t(E), d_row.p, d_t.p, d_v.p, d_tend.p, d_fx.p, d_prog_row.p, d_prog.p, d_consts.p,
                  d_periods.p, d_orow.p, d_ot.p, d_wrow.p, d_out.p};
        c.begin();
        hipLaunchKernelGGL(te_kernel, dim3(launch_blocks(size_t(W + TE_WAVES - 1) / TE_WAVES)), dim3(TE_BLOCK), 0, c.s, a);
        hip_check(hipGetLastError(), "ts_expr");
        g_te.finish(c, "ts_expr", out, d_out.p, no);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ts_expr_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                           const int64_t* t_end, const int32_t* fx, size_t E, const int64_t* prog_row,
                           const int32_t* prog, size_t n_const, const double* consts, size_t n_period,
                           const int64_t* periods, const int64_t* orow, const int64_t* ot, double* out) {
    (void)device;
    try {
        const te_checked ck = te_prepare("shyft_hip_ts_expr_host", S, row, t, v, t_end, fx, E, prog_row, prog, n_const,
                                         consts, n_period, periods, orow, ot, out);
        if (ck.nothing) return 0;
        std::vector<double> stack;
        for (size_t e = 0; e < E; ++e)
            for (int64_t k = orow[e]; k < orow[e + 1]; ++k)
                out[k] = hx::run_program(ck.b, prog + prog_row[e], size_t(prog_row[e + 1] - prog_row[e]),
                                         size_t(k - orow[e]), ot[k], stack);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

double shyft_hip_ts_expr_last_ms(int device) { return g_te.last_ms.load(device, 0.0); }

uint64_t shyft_hip_ts_expr_calls(int device) { return g_te.calls.load(device, 0); }

}  // extern "C"
