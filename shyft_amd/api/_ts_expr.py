"""TimeSeries arithmetic: lazy expression trees and their evaluation (api_time_series.cpp; core/time_series_dd.cpp:94-122,
1007-1118). An operator builds a tree and computes nothing; `evaluate` plans a whole vector of trees
(csrc/host/ts_expr.hpp) and runs them in one device call (region.ts_expr_csr), or with host=True on the host,
bit-identical. The tree node forms are those of `_api._ts_expr_plan`: a `_PointTs`, or (kind, op, a, b)."""
from __future__ import annotations

import numbers

import numpy as np

from . import _api
from ._api import POINT_INSTANT_VALUE, POINT_AVERAGE_VALUE

# kind_t, op_t and the limits of the device evaluation, of csrc/host/ts_expr.hpp
TS_TS, TS_S, S_TS, ABS_TS = 1, 2, 3, 4
ADD, SUB, MUL, DIV, MAX, MIN, POW = range(7)
DEVICE_STACK_DEPTH, DEVICE_PROGRAM_WORDS = 8, 64


def _series_class():
    from . import TimeSeries
    return TimeSeries


def _vector_class():
    from . import TsVector
    return TsVector


def node_of(ts):
    """the tree of a TimeSeries: its expression, or its concrete series as a terminal"""
    return ts._expr if ts._expr is not None else ts._ts


def lazy(tree, fx):
    """a TimeSeries that holds a tree and its point interpretation, not yet evaluated"""
    cls = _series_class()
    ts = cls.__new__(cls)
    ts._expr, ts._fx = tree, fx
    return ts


def _is_scalar(x):
    return isinstance(x, numbers.Real) and not isinstance(x, bool)


def binary(op, lhs, rhs):
    """lhs op rhs in the reference's three forms (time_series_dd.cpp:94-122); NotImplemented for other operands"""
    cls = _series_class()
    if isinstance(lhs, cls) and isinstance(rhs, cls):
        a, b = lhs.point_interpretation(), rhs.point_interpretation()  # result_policy, time_series.h:59-61
        fx = POINT_INSTANT_VALUE if POINT_INSTANT_VALUE in (a, b) else POINT_AVERAGE_VALUE
        return lazy((TS_TS, op, node_of(lhs), node_of(rhs)), fx)
    if isinstance(lhs, cls) and _is_scalar(rhs):
        return lazy((TS_S, op, node_of(lhs), float(rhs)), lhs.point_interpretation())
    if _is_scalar(lhs) and isinstance(rhs, cls):
        return lazy((S_TS, op, node_of(rhs), float(lhs)), rhs.point_interpretation())
    return NotImplemented


def absolute(ts):
    return lazy((ABS_TS, 0, node_of(ts), None), ts.point_interpretation())


def shifted(ts, dt):
    """time_shift(ts, dt) (time_series_dd.h:707-751): the tree over terminals whose times and t_end are moved by dt"""
    moved = {}

    def walk(n):
        if not isinstance(n, tuple):
            if id(n) not in moved:
                moved[id(n)] = n._shifted(dt)
            return moved[id(n)]
        kind, op, a, b = n
        return (kind, op, walk(a), walk(b) if kind == TS_TS else b)

    n = walk(node_of(ts))
    cls = _series_class()
    return lazy(n, ts.point_interpretation()) if isinstance(n, tuple) else cls(_impl=n)


def evaluate(tsv, host=False):
    """The concrete `_PointTs` of every TimeSeries of tsv. The unevaluated expressions among them are planned together
    and run in one device call; with host=True, and for an expression beyond the device's stack depth or program
    length, on the host, bit-identical. Each result is cached in its TimeSeries."""
    from ..region import ts_expr_csr
    for ts in tsv:
        if ts._impl is None and ts._expr is None:
            ts._ts  # a shifted view (TimeSeries.partition_by) becomes its concrete series
    todo = [ts for ts in tsv if ts._impl is None]
    if todo:
        terminals, prog_row, prog, consts, periods, orow, ot, fx, t_end, depth = _api._ts_expr_plan([ts._expr for ts in todo])
        csr = _api._series_csr(terminals)
        words = np.diff(prog_row)
        on_host = np.full(len(todo), True) if host else (depth > DEVICE_STACK_DEPTH) | (words > DEVICE_PROGRAM_WORDS)
        values = np.empty(ot.shape[0])
        for where, h in ((on_host, True), (~on_host, False)):
            pick = np.flatnonzero(where)
            if not len(pick):
                continue
            if len(pick) == len(todo):  # the usual case: the whole batch goes one way
                values = ts_expr_csr(*csr, prog_row, prog, consts, periods, orow, ot, host=h)
                break
            p_row = np.concatenate([[0], np.cumsum(words[pick])])
            o_row = np.concatenate([[0], np.cumsum(np.diff(orow)[pick])])
            p = np.concatenate([prog[prog_row[e]:prog_row[e + 1]] for e in pick])
            o = np.concatenate([ot[orow[e]:orow[e + 1]] for e in pick])
            got = ts_expr_csr(*csr, p_row, p, consts, periods, o_row, o, host=h)
            for j, e in enumerate(pick):
                values[orow[e]:orow[e + 1]] = got[o_row[j]:o_row[j + 1]]
        for e, ts in enumerate(todo):
            ts._impl = _api._PointTs._from_us(ot[orow[e]:orow[e + 1]], int(t_end[e]), values[orow[e]:orow[e + 1]],
                                              POINT_INSTANT_VALUE if fx[e] == 0 else POINT_AVERAGE_VALUE)
    return [ts._impl for ts in tsv]


# ---- TsVector: element by element (ats_vector, time_series_dd.cpp:1007-1118) ------------------------------------------
_OP_NAMES = {ADD: "add", SUB: "sub", MUL: "multiply", DIV: "divide", MAX: "max", MIN: "min", POW: "pow"}


def _broadcast(op, lhs, rhs):
    """the element pairs of lhs op rhs where at least one side is a TsVector; None for an operand of another type"""
    vec, cls = _vector_class(), _series_class()
    one = lambda x: isinstance(x, cls) or _is_scalar(x)  # noqa: E731
    if isinstance(lhs, vec) and isinstance(rhs, vec):
        if len(lhs) != len(rhs):
            raise RuntimeError(f"ts-vector {_OP_NAMES[op]} require same sizes: lhs.size={len(lhs)},rhs.size={len(rhs)}")
        return list(zip(lhs, rhs))
    if isinstance(lhs, vec) and one(rhs):
        return [(x, rhs) for x in lhs]
    if one(lhs) and isinstance(rhs, vec):
        return [(lhs, x) for x in rhs]
    return None


def vector_binary(op, lhs, rhs):
    vec = _vector_class()
    if op in (ADD, SUB) and isinstance(lhs, vec) and isinstance(rhs, vec) and (len(lhs) == 0) != (len(rhs) == 0):
        # an empty side is the neutral element of add and sub (time_series_dd.cpp:1035-1040, 1054-1059)
        if len(rhs) == 0:
            return vec(lhs)
        return vec(rhs) if op == ADD else vec(-x for x in rhs)
    if isinstance(lhs, vec) and _is_scalar(rhs) and op == DIV:  # a / b is a * (1.0 / b) (:1021)
        with np.errstate(divide="ignore"):
            op, rhs = MUL, float(np.float64(1.0) / np.float64(rhs))
    if isinstance(rhs, vec) and not isinstance(lhs, vec) and (op in (MIN, MAX) or (_is_scalar(lhs) and op in (ADD, MUL))):
        lhs, rhs = rhs, lhs  # b + a, b * a, a.min(b), a.max(b): the vector's element comes first (:1010, 1033, 1090-1099)
    pairs = _broadcast(op, lhs, rhs)
    if pairs is None:
        return NotImplemented
    return vec(binary(op, a, b) for a, b in pairs)


def function(op, a, b):
    """api.min / api.max / api.pow in the reference's three forms, on TimeSeries or TsVector"""
    vec = _vector_class()
    r = vector_binary(op, a, b) if isinstance(a, vec) or isinstance(b, vec) else binary(op, a, b)
    if r is NotImplemented:
        raise TypeError(f"{_OP_NAMES[op]}: the arguments must be TimeSeries, TsVector or numbers, at least one a series")
    return r


def min(a, b):  # noqa: A001  (the reference's name)
    return function(MIN, a, b)


def max(a, b):  # noqa: A001
    return function(MAX, a, b)


def pow(a, b):  # noqa: A001
    return function(POW, a, b)


def time_shift(ts, dt):
    """api.time_shift(ts, dt): ts moved dt seconds later; a TsVector element by element"""
    vec = _vector_class()
    if isinstance(ts, vec):
        return vec(shifted(x, dt) for x in ts)
    return shifted(ts, dt)
