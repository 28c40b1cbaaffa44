"""Expression trees over the batches of tests/resample_cases.py, for the time-series arithmetic (host/ts_expr.hpp,
kernels/ts_expr.hip).

A terminal is a `Term`: the numpy arrays of one point series (times in int64 microseconds) and its `_PointTs`. A tree
is a Term or a tuple (kind, op, a, b) in the form of `_api._ts_expr_plan`, with Terms where that takes `_PointTs`:
a and b trees for TS_TS, a tree and a number for TS_S and S_TS (the series first in both), a tree and None for ABS_TS.

SHAPES are the expression shapes, each a function of four terminals a, b, c and a2, where a2 has a's axis and other
values (so `a op a2` is evaluated in values mode). AXIS_PAIRS are hand-made pairs of axes for `a op b`, HAZARDS value
hazards at a point and at the next point of a linear series. `plan` turns trees into the arguments of
region.ts_expr_csr.
"""
import numpy as np

from tests import resample_cases as rc

TS_TS, TS_S, S_TS, ABS_TS = 1, 2, 3, 4
ADD, SUB, MUL, DIV, MAX, MIN, POW = range(7)
OPS = (ADD, SUB, MUL, DIV, MAX, MIN, POW)
LOAD_RAW, LOAD_AT, ABS, BIN, BIN_PERIOD, TS_SCALAR, SCALAR_TS = range(7)  # word_t of host/ts_expr.hpp
HOUR = rc.HOUR


class Term:
    def __init__(self, t, v, t_end, fx):
        from shyft_amd.api import _api
        self.t = np.asarray(t, np.int64)
        self.v = np.asarray(v, np.float64)
        self.t_end, self.fx = int(t_end), int(fx)
        policy = _api.POINT_INSTANT_VALUE if self.fx == 0 else _api.POINT_AVERAGE_VALUE
        self.pts = _api._PointTs._from_us(self.t.tolist(), self.t_end, self.v.tolist(), policy)

    def twin(self, seed=0):
        """the same axis and point type, other values (NaN and infinities stay where they are)"""
        rng = np.random.default_rng(1000 + seed)
        return Term(self.t, np.where(np.isfinite(self.v), rng.normal(1.0, 3.0, len(self.v)), self.v[::-1]), self.t_end,
                    self.fx)

    def shifted(self, dt):
        return Term(self.t + dt, self.v, self.t_end + dt, self.fx)


def terms_of(batch):
    row, t, v, t_end, fx = batch
    return [Term(t[row[k]:row[k + 1]], v[row[k]:row[k + 1]], t_end[k], fx[k]) for k in range(len(t_end))]


def chain(terms):
    """right-deep: t0 + (t1 + (t2 + ...)); its evaluation stack gets len(terms) deep"""
    tree = terms[-1]
    for x in reversed(terms[:-1]):
        tree = (TS_TS, ADD, x, tree)
    return tree


def _forms(op):
    return {f"ts_{op}_ts": lambda a, b, c, a2, op=op: (TS_TS, op, a, b),
            f"ts_{op}_ts_values": lambda a, b, c, a2, op=op: (TS_TS, op, a, a2),
            f"ts_{op}_scalar": lambda a, b, c, a2, op=op: (TS_S, op, a, 2.5),
            f"scalar_{op}_ts": lambda a, b, c, a2, op=op: (S_TS, op, a, 2.5)}


SHAPES = {}
for _op in OPS:
    SHAPES.update(_forms(_op))
SHAPES.update({
    "abs": lambda a, b, c, a2: (ABS_TS, 0, a, None),
    "abs_at": lambda a, b, c, a2: (ABS_TS, 0, (TS_TS, SUB, a, b), None),
    "neg": lambda a, b, c, a2: (S_TS, MUL, a, -1.0),
    # a + b*3.0 - a/2.0
    "mixed": lambda a, b, c, a2: (TS_TS, SUB, (TS_TS, ADD, a, (TS_S, MUL, b, 3.0)), (TS_S, DIV, a, 2.0)),
    "mixed_values": lambda a, b, c, a2: (TS_TS, SUB, (TS_TS, ADD, a, (TS_S, MUL, a2, 3.0)), (TS_S, DIV, a, 2.0)),
    # (a*b) + c with c on a foreign axis, and the same with a values-mode product
    "product_plus_foreign": lambda a, b, c, a2: (TS_TS, ADD, (TS_TS, MUL, a, b), c),
    "values_product_plus_foreign": lambda a, b, c, a2: (TS_TS, ADD, (TS_TS, MUL, a, a2), c),
    # the two scalar-first MAX / MIN orders: values mode at the root, at mode under a ts op ts on unequal axes
    "scalar_max_under_at": lambda a, b, c, a2: (TS_TS, ADD, (S_TS, MAX, a, 2.5), b),
    "scalar_min_under_values": lambda a, b, c, a2: (TS_TS, ADD, (S_TS, MIN, a, 2.5), a2),
    "depth_8": lambda a, b, c, a2: chain([a, b, c, a2, a, b, c, a2]),
    "depth_8_values": lambda a, b, c, a2: chain([a, a2] * 4),
    "depth_9": lambda a, b, c, a2: chain([a, b, c, a2, a, b, c, a2, a]),
    "shifted_operand": lambda a, b, c, a2: (TS_TS, MUL, a, b.shifted(HOUR // 2)),
    "shifted_same_axis": lambda a, b, c, a2: (TS_S, MUL, (TS_TS, ADD, a.shifted(3 * HOUR), a2.shifted(3 * HOUR)), 2.0),
})
DEVICE_SHAPES = [s for s in SHAPES if s != "depth_9"]  # depth_9 is beyond the device's stack


def _axis(points, end, fx, seed):
    rng = np.random.default_rng(seed)
    points = list(points)
    return Term((np.asarray(points, np.float64) * HOUR).astype(np.int64) + rc.T_2016, rng.normal(2.0, 5.0, len(points)),
                end * HOUR + rc.T_2016, fx)


def axis_pairs(fx_a=0, fx_b=1):
    """name -> (a, b): the axis relations of `a op b`"""
    p = list(range(0, 12))
    return {
        "identical": (_axis(p, 12, fx_a, 1), _axis(p, 12, fx_b, 2)),
        "other_t_end": (_axis(p, 12, fx_a, 3), _axis(p, 13, fx_b, 4)),
        "disjoint": (_axis(p, 12, fx_a, 5), _axis([20, 21, 22], 23, fx_b, 6)),
        "touching": (_axis(p, 12, fx_a, 7), _axis([12, 13, 14], 15, fx_b, 8)),
        "nested": (_axis(p, 12, fx_a, 9), _axis([3, 4, 5, 6], 7, fx_b, 10)),
        "nested_between_points": (_axis([0, 4, 8], 12, fx_a, 11), _axis([5, 6, 7], 10, fx_b, 12)),
        "interleaved": (_axis([0, 2, 4, 6, 8], 10, fx_a, 13), _axis([1, 3, 5, 7, 9], 11, fx_b, 14)),
        "one_differs": (_axis(p, 12, fx_a, 15), _axis(p[:5] + [5.5] + p[6:], 12, fx_b, 16)),
        "ends_on_a_point": (_axis(p, 12, fx_a, 17), _axis([2, 3, 4], 6, fx_b, 18)),
        "one_point": (_axis(p, 12, fx_a, 19), _axis([4], 5, fx_b, 20)),
        "one_point_both": (_axis([4], 6, fx_a, 21), _axis([4], 6, fx_b, 22)),
        "empty": (_axis(p, 12, fx_a, 23), _axis([], 0, fx_b, 24)),
        "empty_both": (_axis([], 0, fx_a, 25), _axis([], 0, fx_b, 26)),
    }


HAZARDS = (np.nan, np.inf, -np.inf, -0.0, 0.0)


def hazard_pairs():
    """(a, b) with one hazard value at point 3 of a (so it is v[i] for times in [3, 4) and v[i+1] for [2, 3)), against
    a b whose points fall between a's; every combination of the two point types"""
    out = {}
    for h, x in enumerate(HAZARDS):
        for fx_a in (0, 1):
            for fx_b in (0, 1):
                a = _axis(range(0, 8), 8, fx_a, 40 + h)
                a.v[3] = x
                a = Term(a.t, a.v, a.t_end, a.fx)
                b = Term(a.t[:-1] + HOUR // 4, np.where(np.arange(7) % 2, -1.5, 2.0), a.t_end, fx_b)
                out[f"{x}_{fx_a}{fx_b}"] = (a, b)
    return out


def to_plan_tree(tree):
    if isinstance(tree, Term):
        return tree.pts
    kind, op, a, b = tree
    return (kind, op, to_plan_tree(a), to_plan_tree(b) if kind == TS_TS else b)


class Plan:
    """the arguments of region.ts_expr_csr for a list of trees, and what the planner reports"""

    def __init__(self, trees):
        from shyft_amd.api import _api
        (terminals, self.prog_row, self.prog, self.consts, self.periods, self.orow, self.ot, self.fx, self.t_end,
         self.depth) = _api._ts_expr_plan([to_plan_tree(x) for x in trees])
        self.csr = _api._series_csr(terminals)
        self.n_terminals = len(terminals)

    def args(self):
        return (*self.csr, self.prog_row, self.prog, self.consts, self.periods, self.orow, self.ot)

    def program(self, e):
        return self.prog[self.prog_row[e]:self.prog_row[e + 1]].tolist()

    def axis(self, e):
        return self.ot[self.orow[e]:self.orow[e + 1]], int(self.t_end[e])


def batch_trees(E, k, shapes=DEVICE_SHAPES, long_points=0):
    """E trees over a resample_cases batch of E terminals (lengths rotating, three epochs by k): tree e is shape
    e % len(shapes) of the terminals e, e + 1, e + 2 and a twin of e. With long_points, terminal 8 (where E allows) has
    that many points and tree 8 is an at-mode sum whose root axis is that terminal's."""
    t0, dt = rc.EPOCHS[k % len(rc.EPOCHS)]
    terms = terms_of(rc.make_batch(E, t0, dt, 7300 + E, first=k))
    if long_points and E > 8:
        rng = np.random.default_rng(5)
        terms[8] = Term(t0 + dt * np.arange(long_points, dtype=np.int64), rng.normal(0.0, 4.0, long_points),
                        t0 + dt * long_points, 0)
    names = list(shapes)
    trees = []
    for e in range(E):
        a, b, c = terms[e], terms[(e + 1) % E], terms[(e + 2) % E]
        trees.append(SHAPES[names[e % len(names)]](a, b, c, a.twin(e)))
    if long_points and E > 8:
        a = terms[8]  # every second point of a, linear, over a's period: the merged axis is a's, and the sum is at mode
        coarse = Term(a.t[::2], np.cos(np.arange(len(a.t[::2]))), a.t_end, 0)
        trees[8] = (TS_TS, ADD, (TS_TS, MUL, a, a.twin(8)), (S_TS, SUB, coarse, 1.0))
    return trees
