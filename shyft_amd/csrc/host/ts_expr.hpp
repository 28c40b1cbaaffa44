// Time-series arithmetic on one host thread (C++17, no device code): the reference's lazy expressions over apoint_ts
// (core/time_series_dd.h:275-291, 825-872, 1705-1890; core/time_series_dd.cpp:70-82, 94-129, 197-224, 835-920),
// restated as a planner that turns an expression tree into a postfix program, and an interpreter of such programs.
// kernels/ts_expr.hip evaluates the same programs on the device; the interpreter here is the definition of correct
// and is what shyft_hip_ts_expr_host runs.
//
// Nodes. A terminal is a point series (gpoint_ts; fixed axes are stored as points). ts op ts is abin_op_ts, ts op
// scalar abin_op_ts_scalar, scalar op ts abin_op_scalar_ts, abs abs_ts. Unary minus is scalar op ts with -1.0 and MUL
// (time_series_dd.cpp:101). time_shift(dt) is not a node: the caller shifts the times and t_end of the terminals,
// which gives time_shift_ts (time_series_dd.h:707-751) its axis, its values() and its value_at, since every time
// difference taken below is unchanged by a common shift.
//
// Axis of a node. ts op ts: time_axis::combine of the children's axes, continuous case (core/time_axis.h:1255-1310),
// see combine() below. The other nodes: the series operand's axis (time_series_dd.h:1825-1831, 1867-1873, 848-852).
// Point interpretation. ts op ts: result_policy (core/time_series.h:59-61). The other nodes: the operand's.
//
// Two modes, as in the reference.
//  values mode V, what values() returns (time_series_dd.cpp:197-224, 849-920; time_series_dd.h:863-867): a terminal
//   gives its raw v[i]. A ts op ts node whose children's axes are equal combines V(lhs)[i] and V(rhs)[i]; with unequal
//   axes it evaluates every point i as A(node, time(i)) (abin_op_ts::value, :835-839). The scalar forms and abs pass V
//   through; scalar op ts takes the series value as the first argument of std::max / std::min here (:861-862,
//   :874-875).
//  at mode A, value_at(t): a terminal gives f(t) (point_ts::operator(), core/time_series.h:368-378). ts op ts gives NaN
//   when t is outside the node's total period, else do_op(A(lhs, t), A(rhs, t)) (:125-129). ts op scalar is
//   do_op(A(lhs, t), s), scalar op ts do_op(s, A(rhs, t)), the scalar first also for MAX / MIN (:840-843, :882-885).
//   Once in A, everything below is A.
//  In V every axis between the root and the node equals the root's axis, so point i of the node is point i of the
//  root; in A the time is time(i) of the root. A program therefore needs only the root's point index and time.
//
// do_op (time_series_dd.cpp:70-82). MAX and MIN are std::max / std::min written as their comparison, so the first
// argument is returned when either is NaN. POW is detmath::pow where the reference calls std::pow; the two differ by
// at most detmath's stated 2 ulp. Nothing is fused (-ffp-contract=off) and to_seconds is a division.
//
// Program. int32 words in postfix order over an evaluation stack of doubles:
//   LOAD_RAW term          push v[i] of terminal `term` (V of a terminal; the terminal's axis is the root's)
//   LOAD_AT term           push f(t) of terminal `term`
//   ABS                    top = abs(top)
//   BIN op                 b = pop, a = pop, push do_op(a, b)
//   BIN_PERIOD op k        the same, NaN when t is outside periods[k] = [start, end) (ts op ts in A)
//   TS_SCALAR op k         top = do_op(top, consts[k])
//   SCALAR_TS op k         top = do_op(consts[k], top)
// A scalar is always the operand of a scalar form, so no word pushes a constant on its own. V of scalar op ts with
// MAX / MIN is emitted as TS_SCALAR: that is the series-first argument order.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../detmath/detmath.h"
#include "time_series.hpp"

namespace shyft_hip::host::expr {

enum op_t : int32_t { OP_ADD = 0, OP_SUB = 1, OP_MUL = 2, OP_DIV = 3, OP_MAX = 4, OP_MIN = 5, OP_POW = 6, N_OPS = 7 };
enum word_t : int32_t { LOAD_RAW = 0, LOAD_AT = 1, ABS = 2, BIN = 3, BIN_PERIOD = 4, TS_SCALAR = 5, SCALAR_TS = 6, N_WORDS = 7 };
enum kind_t : int32_t { TERMINAL = 0, TS_TS = 1, TS_S = 2, S_TS = 3, ABS_TS = 4 };

// the limits of the device evaluation (kernels/ts_expr.hip); the interpreter here has none
constexpr int DEVICE_STACK_DEPTH = 8;
constexpr int DEVICE_PROGRAM_WORDS = 64;

// the number of words of the instruction that starts with `code`, 0 for an unknown code
inline int word_count(int32_t code) {
    switch (code) {
    case LOAD_RAW: case LOAD_AT: case BIN: return 2;
    case ABS: return 1;
    case BIN_PERIOD: case TS_SCALAR: case SCALAR_TS: return 3;
    default: return 0;
    }
}

// do_op (time_series_dd.cpp:70-82)
inline double do_op(double a, int32_t op, double b) {
    switch (op) {
    case OP_ADD: return a + b;
    case OP_SUB: return a - b;
    case OP_MUL: return a * b;
    case OP_DIV: return a / b;
    case OP_MAX: return a < b ? b : a;  // std::max(a, b)
    case OP_MIN: return b < a ? b : a;  // std::min(a, b)
    case OP_POW: return detmath::pow(a, b);
    default: throw std::runtime_error("unsupported shyft::api::iop_t");
    }
}

// f(t) of a terminal: point_ts::operator() (core/time_series.h:368-378) over point_dt::index_of (time_axis.h:329-358).
// Not host::point_ts::operator(), which is a slope form without the finiteness rule and serves other entries.
inline double value_at(const utctime* t, const double* v, size_t n, utctime t_end, int32_t fx, utctime tx) {
    if (n == 0 || tx < t[0] || tx >= t_end) return std::numeric_limits<double>::quiet_NaN();
    size_t i = n - 1;
    if (tx < t[n - 1]) i = size_t(std::upper_bound(t, t + n, tx) - t) - 1;
    if (fx == int32_t(POINT_INSTANT_VALUE) && i + 1 < n && std::isfinite(v[i + 1])) {
        const utctime t1 = t[i], t2 = t[i + 1];
        const double f = to_seconds(t2 - tx) / to_seconds(t2 - t1);
        return v[i] * f + (1.0 - f) * v[i + 1];
    }
    return v[i];
}

// A point axis; no points is the empty axis (point_dt::null_range, whose total period holds no time).
struct axis {
    std::vector<utctime> t;
    utctime t_end = 0;
    size_t size() const { return t.size(); }
    utcperiod total_period() const { return t.empty() ? utcperiod() : utcperiod(t.front(), t_end); }
    bool operator==(const axis& o) const { return t == o.t && (t.empty() || t_end == o.t_end); }
    // point_dt::open_range_index_of (time_axis.h:374) for a tx at or after t[0]
    size_t open_range_index_of(utctime tx) const {
        if (tx >= t_end || tx >= t.back()) return t.size() - 1;
        return size_t(std::upper_bound(t.begin(), t.end(), tx) - t.begin()) - 1;
    }
};

// time_axis::combine(a, b), continuous case (core/time_axis.h:1255-1310), statement by statement. The empty axis when
// the periods do not overlap or a side is empty; a when both have the same period, size and periods; otherwise the
// merge of the points of both from the interval that holds the intersection's start t0 up to its end te, common
// points once, t_end = te. As written there, the side that starts earlier contributes the start of its interval that
// holds t0, a point before t0, when t0 is not one of its points; the other side's value is NaN there.
inline axis combine(const axis& a, const axis& b) {
    if (a.size() == 0 || b.size() == 0) return axis();
    const utcperiod pa = a.total_period(), pb = b.total_period();
    if (pb.start >= pa.end || pb.end <= pa.start) return axis();  // !pa.overlaps(pb)
    if (a == b) return a;  // equal period, size and periods
    const utctime t0 = std::max(pa.start, pb.start), te = std::min(pa.end, pb.end);
    size_t ia = a.open_range_index_of(t0), ib = b.open_range_index_of(t0);
    const size_t ea = 1 + a.open_range_index_of(te), eb = 1 + b.open_range_index_of(te);
    axis r;
    r.t.reserve((ea - ia) + (eb - ib));
    r.t_end = te;
    while (ia < ea && ib < eb) {
        const utctime ta = a.t[ia], tb = b.t[ib];
        if (ta == tb) {
            r.t.push_back(ta);
            ++ia;
            ++ib;
        } else if (ta < tb) {
            r.t.push_back(ta);
            ++ia;
        } else {
            r.t.push_back(tb);
            ++ib;
        }
    }
    if (ia < ea) {
        while (ia < ea) {
            const utctime ti = a.t[ia++];
            if (ti < te) r.t.push_back(ti);
        }
    } else {
        while (ib < eb) {
            const utctime ti = b.t[ib++];
            if (ti < te) r.t.push_back(ti);
        }
    }
    if (r.t.back() == r.t_end) r.t.pop_back();
    return r;
}

// result_policy (core/time_series.h:59-61)
inline ts_point_fx result_policy(ts_point_fx a, ts_point_fx b) {
    return a == POINT_INSTANT_VALUE || b == POINT_INSTANT_VALUE ? POINT_INSTANT_VALUE : POINT_AVERAGE_VALUE;
}

// One node of an expression tree. Children come before their parents in tree::nodes and the root is the last node.
// TERMINAL: a = the terminal's index. TS_TS: a, b = the child nodes. TS_S and S_TS: a = the series child, s the scalar.
// ABS_TS: a = the child.
struct node {
    int32_t kind = TERMINAL;
    int32_t op = OP_ADD;
    int32_t a = 0, b = 0;
    double s = 0.0;
};
struct tree {
    std::vector<node> nodes;
};

// The terminals of a batch: their axes and point types (the values are not needed to plan).
struct terminal {
    axis ta;
    ts_point_fx fx = POINT_AVERAGE_VALUE;
};

// The tables that the programs of a batch share, and what the planner reports of one tree.
struct tables {
    std::vector<double> consts;
    std::vector<utctime> periods;  // [n][2] = start, end
};
struct plan {
    axis ta;  // the root's axis
    ts_point_fx fx = POINT_AVERAGE_VALUE;
    std::vector<int32_t> prog;
    int depth = 0;  // the deepest the evaluation stack gets
};

namespace detail {

struct bound {  // what binding a node gives (local_do_bind of each node type)
    axis ta;
    ts_point_fx fx;
};

inline void check_tree(const tree& tr, size_t n_terminals) {
    if (tr.nodes.empty()) throw std::runtime_error("ts_expr: an expression needs at least one node");
    for (size_t k = 0; k < tr.nodes.size(); ++k) {
        const node& x = tr.nodes[k];
        if (x.kind < TERMINAL || x.kind > ABS_TS) throw std::runtime_error("ts_expr: unknown node kind");
        if (x.kind == TERMINAL) {
            if (x.a < 0 || size_t(x.a) >= n_terminals) throw std::runtime_error("ts_expr: terminal index out of range");
            continue;
        }
        if (x.a < 0 || size_t(x.a) >= k || (x.kind == TS_TS && (x.b < 0 || size_t(x.b) >= k)))
            throw std::runtime_error("ts_expr: a node's children must come before it");
        if (x.kind != ABS_TS && (x.op < 0 || x.op >= N_OPS)) throw std::runtime_error("unsupported shyft::api::iop_t");
    }
}

struct emitter {
    const tree& tr;
    const std::vector<bound>& b;
    tables& tb;
    std::vector<int32_t>& prog;
    int sp = 0, depth = 0;

    void push() { depth = std::max(depth, ++sp); }
    int32_t constant(double s) {
        tb.consts.push_back(s);
        return int32_t(tb.consts.size() - 1);
    }
    // k: the node; at: A mode (else V)
    void emit(int32_t k, bool at) {
        const node& x = tr.nodes[size_t(k)];
        switch (x.kind) {
        case TERMINAL:
            prog.insert(prog.end(), {at ? LOAD_AT : LOAD_RAW, x.a});
            push();
            break;
        case TS_TS: {
            const bool below_at = at || !(b[size_t(x.a)].ta == b[size_t(x.b)].ta);
            emit(x.a, below_at);
            emit(x.b, below_at);
            if (below_at) {
                const utcperiod p = b[size_t(k)].ta.total_period();
                tb.periods.push_back(p.start);
                tb.periods.push_back(p.end);
                prog.insert(prog.end(), {BIN_PERIOD, x.op, int32_t(tb.periods.size() / 2 - 1)});
            } else {
                prog.insert(prog.end(), {BIN, x.op});
            }
            --sp;
            break;
        }
        case TS_S:
            emit(x.a, at);
            prog.insert(prog.end(), {TS_SCALAR, x.op, constant(x.s)});
            break;
        case S_TS: {
            emit(x.a, at);
            const bool series_first = !at && (x.op == OP_MAX || x.op == OP_MIN);  // time_series_dd.cpp:861-862, 874-875
            prog.insert(prog.end(), {series_first ? TS_SCALAR : SCALAR_TS, x.op, constant(x.s)});
            break;
        }
        default:  // ABS_TS
            emit(x.a, at);
            prog.push_back(ABS);
            break;
        }
    }
};

}  // namespace detail

// The plan of one tree over the terminals of its batch; the constants and periods it uses are appended to tb.
inline plan make_plan(const tree& tr, const std::vector<terminal>& terminals, tables& tb) {
    detail::check_tree(tr, terminals.size());
    std::vector<detail::bound> b(tr.nodes.size());
    for (size_t k = 0; k < tr.nodes.size(); ++k) {
        const node& x = tr.nodes[k];
        if (x.kind == TERMINAL) b[k] = {terminals[size_t(x.a)].ta, terminals[size_t(x.a)].fx};
        else if (x.kind == TS_TS)
            b[k] = {combine(b[size_t(x.a)].ta, b[size_t(x.b)].ta), result_policy(b[size_t(x.a)].fx, b[size_t(x.b)].fx)};
        else b[k] = b[size_t(x.a)];
    }
    plan p;
    p.ta = b.back().ta;
    p.fx = b.back().fx;
    detail::emitter e{tr, b, tb, p.prog};
    e.emit(int32_t(tr.nodes.size() - 1), false);
    p.depth = e.depth;
    return p;
}

// The terminals of a batch in the CSR form of shyft_hip_resample, and the tables of its programs.
struct batch {
    size_t S = 0;
    const int64_t* row = nullptr;
    const utctime* t = nullptr;
    const double* v = nullptr;
    const utctime* t_end = nullptr;
    const int32_t* fx = nullptr;
    size_t n_const = 0;
    const double* consts = nullptr;
    size_t n_period = 0;
    const utctime* periods = nullptr;
};

// The deepest the stack of a program gets. Throws on an unknown word, an operation, terminal, constant or period
// index out of range, a stack that underflows or does not end at depth 1, and a LOAD_RAW of a terminal that does not
// have n_points points (it is read at the root's point index).
inline int check_program(const batch& b, const int32_t* prog, size_t n_words, size_t n_points) {
    int sp = 0, depth = 0;
    size_t p = 0;
    while (p < n_words) {
        const int32_t code = prog[p];
        const int w = word_count(code);
        if (w == 0) throw std::runtime_error("ts_expr: unknown program word " + std::to_string(code));
        if (p + size_t(w) > n_words) throw std::runtime_error("ts_expr: the program ends inside an instruction");
        if (code == LOAD_RAW || code == LOAD_AT) {
            const int32_t term = prog[p + 1];
            if (term < 0 || size_t(term) >= b.S) throw std::runtime_error("ts_expr: terminal index out of range");
            if (code == LOAD_RAW && size_t(b.row[term + 1] - b.row[term]) != n_points)
                throw std::runtime_error("ts_expr: LOAD_RAW needs a terminal with as many points as the expression");
            depth = std::max(depth, ++sp);
        } else if (code == ABS) {
            if (sp < 1) throw std::runtime_error("ts_expr: the evaluation stack underflows");
        } else {
            if (prog[p + 1] < 0 || prog[p + 1] >= N_OPS) throw std::runtime_error("unsupported shyft::api::iop_t");
            if (code == BIN || code == BIN_PERIOD) {
                if (sp < 2) throw std::runtime_error("ts_expr: the evaluation stack underflows");
                --sp;
                if (code == BIN_PERIOD && (prog[p + 2] < 0 || size_t(prog[p + 2]) >= b.n_period))
                    throw std::runtime_error("ts_expr: period index out of range");
            } else {
                if (sp < 1) throw std::runtime_error("ts_expr: the evaluation stack underflows");
                if (prog[p + 2] < 0 || size_t(prog[p + 2]) >= b.n_const)
                    throw std::runtime_error("ts_expr: constant index out of range");
            }
        }
        p += size_t(w);
    }
    if (sp != 1) throw std::runtime_error("ts_expr: a program must leave exactly one value on the evaluation stack");
    return depth;
}

// A checked program at point i of the root axis, whose time is tx.
inline double run_program(const batch& b, const int32_t* prog, size_t n_words, size_t i, utctime tx,
                          std::vector<double>& stack) {
    stack.clear();
    for (size_t p = 0; p < n_words; p += size_t(word_count(prog[p]))) {
        switch (prog[p]) {
        case LOAD_RAW:
            stack.push_back(b.v[b.row[prog[p + 1]] + int64_t(i)]);
            break;
        case LOAD_AT: {
            const int32_t s = prog[p + 1];
            const int64_t r0 = b.row[s];
            stack.push_back(value_at(b.t + r0, b.v + r0, size_t(b.row[s + 1] - r0), b.t_end[s], b.fx[s], tx));
            break;
        }
        case ABS:
            stack.back() = std::abs(stack.back());
            break;
        case BIN:
        case BIN_PERIOD: {
            const double y = stack.back();
            stack.pop_back();
            double r = do_op(stack.back(), prog[p + 1], y);
            if (prog[p] == BIN_PERIOD) {
                const utctime* q = b.periods + 2 * size_t(prog[p + 2]);
                if (!(tx >= q[0] && tx < q[1])) r = std::numeric_limits<double>::quiet_NaN();
            }
            stack.back() = r;
            break;
        }
        case TS_SCALAR:
            stack.back() = do_op(stack.back(), prog[p + 1], b.consts[prog[p + 2]]);
            break;
        default:  // SCALAR_TS
            stack.back() = do_op(b.consts[prog[p + 2]], prog[p + 1], stack.back());
            break;
        }
    }
    return stack.back();
}

}  // namespace shyft_hip::host::expr
