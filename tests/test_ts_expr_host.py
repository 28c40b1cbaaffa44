"""Time-series arithmetic on the host (csrc/host/ts_expr.hpp through region.ts_expr_csr(host=True)): the reference's
known answers, an independent numpy statement of combine, f(t) and the two evaluation modes over every case of
tests/ts_expr_cases.py, hand-derived small cases, the planner's programs, and the refusals."""
import numpy as np
import pytest

from shyft_amd import region
from shyft_amd._native import ShyftHipError
from tests import oracle_lib
from tests import resample_cases as rc
from tests import ts_expr_cases as xc
from tests.ts_expr_cases import (ABS, ABS_TS, ADD, BIN, BIN_PERIOD, DIV, LOAD_AT, LOAD_RAW, MAX, MIN, MUL, POW, S_TS,
                                 SCALAR_TS, SUB, TS_S, TS_SCALAR, TS_TS, Plan, Term)

NAN = float("nan")
HOUR = rc.HOUR


def host_values(trees):
    """[values of tree e], and the plan"""
    plan = Plan(trees)
    out = region.ts_expr_csr(*plan.args(), host=True)
    return [out[plan.orow[e]:plan.orow[e + 1]] for e in range(len(trees))], plan


# ---- the independent statement ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def det_pow():
    f = oracle_lib.load("detmath").oracle_pow  # detmath::pow on the host, element by element
    return lambda a, b: np.array([f(float(x), float(y)) for x, y in zip(*np.broadcast_arrays(a, b))])


class Model:
    """values() and value_at() of an expression as the issue states them, on numpy arrays"""

    def __init__(self, det_pow):
        self.pow = det_pow

    def op(self, op, a, b):
        a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
        with np.errstate(all="ignore"):
            if op == MAX:
                return np.where(a < b, b, a)  # std::max(a, b): a unless a < b
            if op == MIN:
                return np.where(b < a, b, a)  # std::min(a, b): a unless b < a
            if op == POW:
                return self.pow(a, b)
            return {ADD: np.add, SUB: np.subtract, MUL: np.multiply, DIV: np.divide}[op](a, b)

    @staticmethod
    def f(x, tx):
        """f(t) of a terminal at the times tx"""
        tx = np.asarray(tx, np.int64)
        r = np.full(len(tx), NAN)
        n = len(x.t)
        if n == 0:
            return r
        inside = (tx >= x.t[0]) & (tx < x.t_end)
        i = np.clip(np.searchsorted(x.t, tx, side="right") - 1, 0, n - 1)
        nxt = np.minimum(i + 1, n - 1)
        linear = (x.fx == 0) & (i + 1 < n) & np.isfinite(x.v[nxt])
        with np.errstate(all="ignore"):
            f = ((x.t[nxt] - tx).astype(np.float64) / 1e6) / ((x.t[nxt] - x.t[i]).astype(np.float64) / 1e6)
            line = x.v[i] * f + (1.0 - f) * x.v[nxt]
        return np.where(inside, np.where(linear, line, x.v[i]), NAN)

    @staticmethod
    def combine(a, b):
        """(times, t_end) of two axes, as sets: the points of each side from the one at or before the start of the
        intersection, below its end"""
        (ta, ea), (tb, eb) = a, b
        empty = (np.empty(0, np.int64), 0)
        if len(ta) == 0 or len(tb) == 0 or tb[0] >= ea or eb <= ta[0]:
            return empty
        if len(ta) == len(tb) and np.array_equal(ta, tb) and ea == eb:
            return a
        t0, te = max(ta[0], tb[0]), min(ea, eb)
        part = lambda t: t[(t >= t[t <= t0].max()) & (t < te)]  # noqa: E731
        return np.union1d(part(ta), part(tb)), te

    def axis(self, tree):
        if isinstance(tree, Term):
            return tree.t, tree.t_end
        kind, _, a, b = tree
        return self.combine(self.axis(a), self.axis(b)) if kind == TS_TS else self.axis(a)

    def fx(self, tree):
        if isinstance(tree, Term):
            return tree.fx
        kind, _, a, b = tree
        return min(self.fx(a), self.fx(b)) if kind == TS_TS else self.fx(a)  # instant (0) wins

    @staticmethod
    def same_axis(p, q):
        return len(p[0]) == len(q[0]) and np.array_equal(p[0], q[0]) and (len(p[0]) == 0 or p[1] == q[1])

    def values(self, tree):
        if isinstance(tree, Term):
            return tree.v
        kind, op, a, b = tree
        if kind == ABS_TS:
            return np.abs(self.values(a))
        if kind == TS_S:
            return self.op(op, self.values(a), b)
        if kind == S_TS:
            return self.op(op, self.values(a), b) if op in (MAX, MIN) else self.op(op, b, self.values(a))
        if self.same_axis(self.axis(a), self.axis(b)):
            return self.op(op, self.values(a), self.values(b))
        return self.at(tree, self.axis(tree)[0])

    def at(self, tree, tx):
        if isinstance(tree, Term):
            return self.f(tree, tx)
        kind, op, a, b = tree
        if kind == ABS_TS:
            return np.abs(self.at(a, tx))
        if kind == TS_S:
            return self.op(op, self.at(a, tx), b)
        if kind == S_TS:
            return self.op(op, b, self.at(a, tx))
        t, t_end = self.axis(tree)
        inside = (tx >= t[0]) & (tx < t_end) if len(t) else np.zeros(len(tx), bool)
        return np.where(inside, self.op(op, self.at(a, tx), self.at(b, tx)), NAN)


def _check(model, trees, what):
    got, plan = host_values(trees)
    for e, tree in enumerate(trees):
        t, t_end = model.axis(tree)
        pt, pe = plan.axis(e)
        assert np.array_equal(pt, t), (what, e, "axis")
        if len(t):
            assert pe == t_end, (what, e, "t_end")
        assert plan.fx[e] == model.fx(tree), (what, e, "point type")
        want = model.values(tree)
        assert rc.same_bits(got[e], np.asarray(want, np.float64)), (what, e, got[e][:6], want[:6])


@pytest.mark.parametrize("shape", list(xc.SHAPES))
def test_every_shape_on_every_axis_pair_equals_the_numpy_statement(det_pow, shape):
    model = Model(det_pow)
    for fx_a, fx_b in ((0, 1), (1, 0), (0, 0), (1, 1)):
        pairs = xc.axis_pairs(fx_a, fx_b)
        c = xc._axis([1.5, 2.5, 6.25, 9], 30, 0, 99)
        _check(model, [xc.SHAPES[shape](a, b, c, a.twin(k)) for k, (a, b) in enumerate(pairs.values())],
               (shape, fx_a, fx_b))


@pytest.mark.parametrize("shape", ["ts_0_ts", "ts_3_ts", "ts_4_ts", "ts_5_ts", "ts_6_ts", "scalar_3_ts", "scalar_4_ts",
                                   "scalar_5_ts", "ts_4_scalar", "abs", "abs_at", "neg", "mixed",
                                   "scalar_max_under_at", "scalar_min_under_values", "product_plus_foreign"])
def test_value_hazards_equal_the_numpy_statement(det_pow, shape):
    model = Model(det_pow)
    pairs = xc.hazard_pairs()
    c = xc._axis([1.5, 2.5, 6.25], 30, 0, 98)
    trees = [xc.SHAPES[shape](a, b, c, a.twin(k)) for k, (a, b) in enumerate(pairs.values())]
    trees += [xc.SHAPES[shape](b, a, c, b.twin(k)) for k, (a, b) in enumerate(pairs.values())]
    _check(model, trees, shape)


@pytest.mark.parametrize("k,E", [(0, 9), (1, 65)])
def test_batches_of_the_gpu_test_equal_the_numpy_statement(det_pow, k, E):
    """the batches tests/test_ts_expr_gpu.py compares device against host on, here host against the statement"""
    _check(Model(det_pow), xc.batch_trees(E, k, shapes=list(xc.SHAPES), long_points=300), (k, E))


# ---- the reference's known answers -----------------------------------------------------------------------------------
def _fixed(values, fx, t0=0, dt=HOUR):
    n = len(values)
    return Term(t0 + dt * np.arange(n, dtype=np.int64), values, t0 + dt * n, fx)


def test_pow_known_answers():
    """shyft/tests/api/test_pow.py:11-17: a = [1, 2, 3], b = [2, 2, 2] stair-case on one axis"""
    a, b = _fixed([1.0, 2.0, 3.0], 1), _fixed([2.0, 2.0, 2.0], 1)
    got, _ = host_values([(TS_S, POW, a, 2.0), (S_TS, POW, a, 2.0), (TS_TS, POW, b, a)])
    assert got[0].tolist() == [1.0, 4.0, 9.0]
    assert got[1].tolist() == [2.0, 4.0, 8.0]
    assert got[2].tolist() == [2.0, 4.0, 8.0]


def test_basic_math_known_answers():
    """shyft/tests/api/test_time_series.py:206-232: a = 3.0 stair-case, b = 2.0 linear on 240 hours"""
    a, b = _fixed([3.0] * 240, 1), _fixed([2.0] * 240, 0)
    c = xc.SHAPES["mixed"](a, b, None, None)  # a + b*3.0 - a/2.0
    got, plan = host_values([c, (S_TS, MUL, a, -1.0), (S_TS, SUB, b, 1.0), (TS_S, SUB, b, 1.0), (TS_S, MAX, c, 300.0),
                             (TS_S, MIN, c, -300.0)])
    assert all(len(g) == 240 for g in got)
    assert np.all(got[0] == 7.5)                 # :224-226
    assert np.all(got[1] == -3.0)                # :227, d = -a
    assert got[2].max() == -1.0                  # :210, (1.0 - b)
    assert got[3].max() == 1.0                   # :211, (b - 1.0)
    assert np.all(got[4] == 300.0) and np.all(got[5] == -300.0)  # :229-232
    assert plan.fx.tolist() == [0, 1, 0, 0, 0, 0]  # result_policy: linear wins in c; the scalar forms keep the operand's


def test_time_shift_known_answer():
    """shyft/tests/api/test_time_series.py:366-372: 2.0 * ts1.time_shift(t0 - t1) has ts0's times and twice its values"""
    ts0 = _fixed(np.arange(24.0), 0, t0=rc.T_2016)
    shift = 3600 * 10**6 * 24 * 7
    ts1 = ts0.shifted(shift)
    got, plan = host_values([(S_TS, MUL, ts1.shifted(-shift), 2.0)])
    assert np.array_equal(plan.axis(0)[0], ts0.t) and plan.axis(0)[1] == ts0.t_end
    assert got[0].tolist() == (2.0 * ts0.v).tolist()


# ---- hand-derived small cases ----------------------------------------------------------------------------------------
def test_the_period_check_gives_nan_outside_an_inner_node():
    """(a + b) + c: a on [0, 4) h, b on [2, 6) h, c on [0, 8) h, all stair-case 1.0. The inner node's axis starts at
    a's point 2 h (the start of the intersection) and ends at 4 h; the outer axis is the merge of {2, 3} with c's points
    from 2 h on, up to 4 h. Shift c by half an hour and its point 1.5 h holds the start: there the inner node is
    outside its period, NaN, although a(1.5 h) + c(1.5 h) alone would be finite."""
    a, b = _fixed([1.0] * 4, 1), _fixed([1.0] * 4, 1, t0=2 * HOUR)
    c = _fixed([1.0] * 8, 1, t0=HOUR // 2)
    got, plan = host_values([(TS_TS, ADD, (TS_TS, ADD, a, b), c)])
    assert (plan.axis(0)[0] / HOUR).tolist() == [1.5, 2.0, 2.5, 3.0, 3.5] and plan.axis(0)[1] == 4 * HOUR
    assert rc.same_bits(got[0], np.array([NAN, 3.0, 3.0, 3.0, 3.0]))


def test_the_first_argument_wins_on_nan():
    a, b = _fixed([NAN, 1.0, NAN, 5.0], 1), _fixed([2.0, NAN, NAN, 3.0], 1)
    got, _ = host_values([(TS_TS, MAX, a, b), (TS_TS, MIN, a, b), (TS_TS, MAX, b, a), (TS_TS, MIN, b, a)])
    assert rc.same_bits(got[0], np.array([NAN, 1.0, NAN, 5.0]))  # a < b is false with a NaN on either side: a
    assert rc.same_bits(got[1], np.array([NAN, 1.0, NAN, 3.0]))
    assert rc.same_bits(got[2], np.array([2.0, NAN, NAN, 5.0]))
    assert rc.same_bits(got[3], np.array([2.0, NAN, NAN, 3.0]))


def test_both_scalar_max_orders():
    """max(2.5, ts): values mode takes the series first, so a NaN point stays NaN (time_series_dd.cpp:861); at mode,
    under a ts op ts on unequal axes, takes the scalar first, so the NaN point becomes 2.5 (:840-843)"""
    a = _fixed([NAN, 1.0, 4.0], 1)
    zero = _fixed([0.0, 0.0], 1, t0=0, dt=2 * HOUR)  # other points, the same period up to 3 h ... 4 h
    got, plan = host_values([(S_TS, MAX, a, 2.5), (TS_TS, ADD, (S_TS, MAX, a, 2.5), zero)])
    assert rc.same_bits(got[0], np.array([NAN, 2.5, 4.0]))
    assert (plan.axis(1)[0] / HOUR).tolist() == [0.0, 1.0, 2.0]
    assert rc.same_bits(got[1], np.array([2.5, 2.5, 4.0]))
    assert plan.program(0) == [LOAD_RAW, 0, TS_SCALAR, MAX, 0]
    assert plan.program(1)[:5] == [LOAD_AT, 0, SCALAR_TS, MAX, 1]


def test_negative_zero_in_each_mode():
    """values mode passes a stored -0.0 through: -0.0 + -0.0 = -0.0 and max(-0.0, 0.0) = -0.0 (not less: the first).
    At mode a linear terminal computes v[i]*f + (1-f)*v[i+1] with f = 1 at its own point: -0.0*1 + 0*1.0 = +0.0."""
    a, b = _fixed([-0.0, 1.0, -0.0], 0), _fixed([-0.0, 1.0, -0.0], 0)
    other = _fixed([-0.0, -0.0, -0.0, -0.0], 0, dt=HOUR * 3 // 4)
    got, _ = host_values([(TS_TS, ADD, a, b), (TS_S, MAX, a, 0.0), (TS_TS, ADD, a, other)])
    assert np.signbit(got[0][[0, 2]]).all() and got[0][1] == 2.0
    assert np.signbit(got[1][[0, 2]]).all()
    # a(0) = -0.0*1 + 0.0*1.0 = +0.0, other(0) = -0.0*1 + 0.0*-0.0 = -0.0 + -0.0 = -0.0; +0.0 + -0.0 = +0.0
    assert got[2][0] == 0.0 and not np.signbit(got[2][0])


def test_the_empty_combine_and_the_result_point_types():
    p = xc.axis_pairs(1, 1)
    inst = xc.axis_pairs(0, 1)
    trees = [(TS_TS, ADD, *p["disjoint"]), (TS_TS, ADD, *p["touching"]), (TS_TS, ADD, *p["empty"]),
             (TS_TS, ADD, (TS_TS, ADD, *p["disjoint"]), p["identical"][0]), (TS_TS, MUL, *p["identical"]),
             (TS_TS, MUL, *inst["identical"]), (ABS_TS, 0, inst["identical"][0], None),
             (S_TS, SUB, inst["identical"][1], 1.0)]
    got, plan = host_values(trees)
    assert [len(g) for g in got] == [0, 0, 0, 0, 12, 12, 12, 12]
    assert plan.fx.tolist() == [1, 1, 1, 1, 1, 0, 0, 1]


# ---- the planner's programs ------------------------------------------------------------------------------------------
def _words(program):
    sizes = {LOAD_RAW: 2, LOAD_AT: 2, ABS: 1, BIN: 2, BIN_PERIOD: 3, TS_SCALAR: 3, SCALAR_TS: 3}
    out, p = [], 0
    while p < len(program):
        out.append(tuple(program[p:p + sizes[program[p]]]))
        p += sizes[program[p]]
    return out


def test_plans_of_the_named_shapes():
    a, b = xc.axis_pairs()["interleaved"]
    c, a2 = xc._axis([1.5, 2.5], 30, 0, 97), a.twin()
    names = ["mixed", "mixed_values", "product_plus_foreign", "values_product_plus_foreign", "abs", "neg", "depth_8",
             "depth_8_values", "depth_9"]
    plan = Plan([xc.SHAPES[n](a, b, c, a2) for n in names])
    prog = {n: _words(plan.program(e)) for e, n in enumerate(names)}
    depth = dict(zip(names, plan.depth.tolist()))
    words = dict(zip(names, np.diff(plan.prog_row).tolist()))
    # terminals in order of first use: a 0, b 1, a2 2, c 3
    assert plan.n_terminals == 4
    assert prog["mixed"] == [(LOAD_AT, 0), (LOAD_AT, 1), (TS_SCALAR, MUL, 0), (BIN_PERIOD, ADD, 0), (LOAD_AT, 0),
                             (TS_SCALAR, DIV, 1), (BIN_PERIOD, SUB, 1)]
    assert prog["mixed_values"] == [(LOAD_RAW, 0), (LOAD_RAW, 2), (TS_SCALAR, MUL, 2), (BIN, ADD), (LOAD_RAW, 0),
                                    (TS_SCALAR, DIV, 3), (BIN, SUB)]
    assert [w[0] for w in prog["product_plus_foreign"]] == [LOAD_AT, LOAD_AT, BIN_PERIOD, LOAD_AT, BIN_PERIOD]
    assert [w[0] for w in prog["values_product_plus_foreign"]] == [LOAD_AT, LOAD_AT, BIN_PERIOD, LOAD_AT, BIN_PERIOD]
    assert prog["abs"] == [(LOAD_RAW, 0), (ABS,)]
    assert [w[:2] for w in prog["neg"]] == [(LOAD_RAW, 0), (SCALAR_TS, MUL)]
    assert plan.consts[prog["neg"][1][2]] == -1.0
    assert [w[0] for w in prog["depth_8"]] == [LOAD_AT] * 8 + [BIN_PERIOD] * 7
    assert [w[0] for w in prog["depth_8_values"]] == [LOAD_RAW] * 8 + [BIN] * 7
    assert depth == {"mixed": 2, "mixed_values": 2, "product_plus_foreign": 2, "values_product_plus_foreign": 2,
                     "abs": 1, "neg": 1, "depth_8": 8, "depth_8_values": 8, "depth_9": 9}
    assert words["depth_8"] == 8 * 2 + 7 * 3 and words["depth_8_values"] == 8 * 2 + 7 * 2 and words["mixed"] == 18
    # the periods of mixed: the merged axis of a and b, both nodes
    t, t_end = plan.axis(0)
    assert plan.periods[:2].tolist() == [[t[0], t_end]] * 2


# ---- refusals of malformed programs and limits -------------------------------------------------------------------------
def _good():
    a, b = xc.axis_pairs()["interleaved"]
    plan = Plan([(TS_TS, ADD, a, b), (TS_S, MUL, a, 2.0)])
    return dict(zip(("row", "t", "v", "t_end", "fx", "prog_row", "prog", "consts", "periods", "orow", "ot"),
                    [np.array(x) for x in plan.args()]))


def _refused(expected, **change):
    texts = []
    for host in (False, True):
        a = _good()
        a.update({k: np.asarray(v) for k, v in change.items()})
        with pytest.raises(ShyftHipError) as e:
            region.ts_expr_csr(*a.values(), host=host)
        texts.append(str(e.value))
    assert texts == [expected, expected]  # the device entry, refused before it touches the device, and its _host twin


def test_the_well_formed_batch_is_accepted_by_the_host_twin():
    a = _good()
    assert a["prog"].tolist() == [LOAD_AT, 0, LOAD_AT, 1, BIN_PERIOD, ADD, 0, LOAD_RAW, 0, TS_SCALAR, MUL, 0]
    assert region.ts_expr_csr(*a.values(), host=True).shape == (a["orow"][-1],)


def test_an_unknown_word_is_refused():
    prog = _good()["prog"]
    prog[7] = 9
    _refused("ts_expr: unknown program word 9", prog=prog)


def test_an_operation_out_of_range_is_refused():
    prog = _good()["prog"]
    prog[5] = 7
    _refused("unsupported shyft::api::iop_t", prog=prog)


def test_a_terminal_index_out_of_range_is_refused():
    prog = _good()["prog"]
    prog[3] = 2
    _refused("ts_expr: terminal index out of range", prog=prog)


def test_a_constant_index_out_of_range_is_refused():
    prog = _good()["prog"]
    prog[11] = 1
    _refused("ts_expr: constant index out of range", prog=prog)


def test_a_period_index_out_of_range_is_refused():
    prog = _good()["prog"]
    prog[6] = -1
    _refused("ts_expr: period index out of range", prog=prog)


def test_a_stack_underflow_is_refused():
    prog = _good()["prog"]
    prog[0:2] = [LOAD_AT, 0]
    prog[2:4] = [BIN, ADD]
    _refused("ts_expr: the evaluation stack underflows", prog=prog)


def test_a_program_that_leaves_two_values_is_refused():
    a = _good()
    _refused("ts_expr: a program must leave exactly one value on the evaluation stack",
             prog=np.concatenate([a["prog"][:4], a["prog"][7:]]), prog_row=[0, 4, 9])


def test_a_program_that_ends_inside_an_instruction_is_refused():
    a = _good()
    _refused("ts_expr: the program ends inside an instruction", prog=a["prog"][:-1], prog_row=[0, 7, 11])


def test_a_raw_load_of_a_terminal_of_another_size_is_refused():
    a = _good()  # the second expression, a * 2.0, with one output point less than a has points
    _refused("ts_expr: LOAD_RAW needs a terminal with as many points as the expression",
             orow=[0, a["orow"][1], a["orow"][2] - 1], ot=a["ot"][:-1])


def test_a_decreasing_orow_is_refused():
    a = _good()
    _refused("ts_expr: row must not decrease", orow=[0, a["orow"][2] + 1, a["orow"][2]])


def test_a_malformed_terminal_is_refused():
    t = _good()["t"]
    t[1] = t[0]
    _refused("time_axis::point_dt() needs time-points in increasing order", t=t)


def test_the_device_limits_are_refused_by_the_device_entry_only():
    a, b = xc.axis_pairs()["interleaved"]
    c, a2 = xc._axis([1.5, 2.5], 30, 0, 97), a.twin()
    deep = Plan([xc.SHAPES["depth_9"](a, b, c, a2)])
    with pytest.raises(ShyftHipError) as e:
        region.ts_expr_csr(*deep.args())
    assert str(e.value) == ("ts_expr: an evaluation stack of 9 values is deeper than the device's 8; "
                            "shyft_hip_ts_expr_host evaluates it")
    assert len(region.ts_expr_csr(*deep.args(), host=True)) == deep.orow[-1]
    tree = a
    for _ in range(21):  # 2 + 21 * 3 = 65 words, stack depth 1
        tree = (TS_S, ADD, tree, 1.0)
    long = Plan([tree])
    assert long.depth.tolist() == [1] and len(long.prog) == 65
    with pytest.raises(ShyftHipError) as e:
        region.ts_expr_csr(*long.args())
    assert str(e.value) == ("ts_expr: a program of 65 words is longer than the device's 64; "
                            "shyft_hip_ts_expr_host evaluates it")
    want = a.v.copy()
    for _ in range(21):
        want = want + 1.0
    assert region.ts_expr_csr(*long.args(), host=True).tolist() == want.tolist()


def test_no_expression_is_nothing_to_do():
    a = _good()
    for host in (False, True):  # neither touches the device
        out = region.ts_expr_csr(a["row"], a["t"], a["v"], a["t_end"], a["fx"], [0], [], [], np.empty((0, 2)), [0], [],
                                 host=host)
        assert out.shape == (0,)
