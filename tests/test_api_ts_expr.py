"""api.TimeSeries / api.TsVector arithmetic (shyft_amd/api/_ts_expr.py): the operators and functions of the
reference's apoint_ts and ats_vector, laziness, expressions as arguments of the existing entries, and concrete series
unchanged. Everything here evaluates through the host twin, so no GPU is needed."""
import copy

import numpy as np
import pytest

from shyft_amd import api, region

HOUR = 3600
AVG, INST = api.POINT_AVERAGE_VALUE, api.POINT_INSTANT_VALUE


def _ts(values, fx=AVG, t0=0, dt=HOUR):
    return api.TimeSeries(api.TimeAxis(t0, dt, len(values)), values, fx)


@pytest.fixture
def count(monkeypatch):
    """the number of evaluations (host or device) since the fixture was made"""
    calls = []
    real = region.ts_expr_csr
    monkeypatch.setattr(region, "ts_expr_csr", lambda *a, **kw: (calls.append(kw.get("host")), real(*a, **kw))[1])
    return calls


def test_operators_of_a_series():
    a, b = _ts([1.0, 2.0, 3.0]), _ts([2.0, 2.0, 4.0])
    assert list((a + b).values) == [3.0, 4.0, 7.0]
    assert list((a - b).values) == [-1.0, 0.0, -1.0]
    assert list((a * b).values) == [2.0, 4.0, 12.0]
    assert list((a / b).values) == [0.5, 1.0, 0.75]
    assert list((a + 1).values) == [2.0, 3.0, 4.0] and list((1 + a).values) == [2.0, 3.0, 4.0]
    assert list((a - 1.0).values) == [0.0, 1.0, 2.0] and list((1.0 - a).values) == [0.0, -1.0, -2.0]
    assert list((a * 3.6).values) == [1.0 * 3.6, 2.0 * 3.6, 3.0 * 3.6] and list((2.0 * a).values) == [2.0, 4.0, 6.0]
    assert list((a / 2.0).values) == [0.5, 1.0, 1.5] and list((6.0 / a).values) == [6.0, 3.0, 2.0]
    assert list((-a).values) == [-1.0, -2.0, -3.0]
    assert list((a - b).abs().values) == [1.0, 0.0, 1.0]
    assert list(a.min(b).values) == [1.0, 2.0, 3.0] and list(a.max(b).values) == [2.0, 2.0, 4.0]
    assert list(a.min(2.0).values) == [1.0, 2.0, 2.0] and list(a.max(2.0).values) == [2.0, 2.0, 3.0]
    assert list(a.pow(2.0).values) == [1.0, 4.0, 9.0] and list(b.pow(a).values) == [2.0, 4.0, 64.0]
    with pytest.raises(TypeError):
        a + "x"


def test_module_functions_in_the_three_forms():
    from shyft_amd.api import max as ts_max, min as ts_min, pow as ts_pow  # the reference's `from shyft.api import pow`
    a, b = _ts([1.0, 2.0, 3.0]), _ts([2.0, 2.0, 2.0])
    assert list(api.max(a, b).values) == [2.0, 2.0, 3.0] and list(ts_max(a, 2.5).values) == [2.5, 2.5, 3.0]
    assert list(api.max(2.5, a).values) == [2.5, 2.5, 3.0]
    assert list(api.min(a, b).values) == [1.0, 2.0, 2.0] and list(ts_min(1.5, a).values) == [1.0, 1.5, 1.5]
    assert list(api.pow(a, 2.0).values) == [1.0, 4.0, 9.0]      # test_pow.py:13-17
    assert list(ts_pow(2.0, a).values) == [2.0, 4.0, 8.0]
    assert list(api.pow(b, a).values) == [2.0, 4.0, 8.0]
    s = api.time_shift(a, 2 * HOUR)
    assert [s.time(i) for i in range(3)] == [2 * HOUR, 3 * HOUR, 4 * HOUR] and list(s.values) == [1.0, 2.0, 3.0]
    assert s.total_period().end == 5 * HOUR
    assert max(1, 2) == 2 and api.percentiles is not None  # the builtins are untouched for everyone else


def test_the_reference_s_first_expression():
    """shyft/tests/api/test_time_series.py:206-232"""
    ta = api.TimeAxis(1500000000, HOUR, 240)
    a = api.TimeSeries(ta=ta, fill_value=3.0, point_fx=AVG)
    b = api.TimeSeries(ta=ta, fill_value=2.0, point_fx=INST)
    assert (1.0 - b).values.to_numpy().max() == -1.0 and (b - 1.0).values.to_numpy().max() == 1.0
    c = a + b * 3.0 - a / 2.0
    d, f, g, h, k = -a, api.max(c, 300.0), api.min(c, -300.0), c.max(300.0), c.min(-300)
    assert a.size() == b.size() == c.size() == 240
    assert c.value(0) == 7.5
    for i in range(240):
        assert c.value(i) == a.value(i) + b.value(i) * 3.0 - a.value(i) / 2.0 and d.value(i) == -a.value(i)
        assert f.value(i) == h.value(i) == 300.0 and g.value(i) == k.value(i) == -300.0
    assert c.point_interpretation() == INST and d.point_interpretation() == AVG


def test_time_shift_in_an_expression():
    """shyft/tests/api/test_time_series.py:366-372"""
    t0, t1 = 1451606400, 1451606400 + 7 * 86400
    ts0 = _ts(np.arange(24.0).tolist(), INST, t0=t0)
    ts1 = api.time_shift(ts0, t1 - t0)
    ts2 = 2.0 * ts1.time_shift(t0 - t1)
    for i in range(ts0.size()):
        assert ts0.value(i) == ts1.value(i) and ts0.value(i) * 2.0 == ts2.value(i)
        assert ts0.time(i) + (t1 - t0) == ts1.time(i) and ts0.time(i) == ts2.time(i)
    shifted_sum = (ts0 + ts0).time_shift(HOUR)  # a shift of an expression moves its terminals
    assert shifted_sum.time(0) == t0 + HOUR and list(shifted_sum.values) == (2.0 * np.arange(24.0)).tolist()


def test_nothing_is_evaluated_until_it_is_read(count):
    a, b = _ts([1.0, 2.0, 3.0], AVG), _ts([1.0, 1.0], INST, t0=HOUR // 2)
    c = (a * b + 2.0).abs()
    d = api.max(c, 0.5).time_shift(HOUR)
    assert count == [] and c._impl is None and d._impl is None
    assert c.point_interpretation() == INST and (a * 2.0).point_interpretation() == AVG
    assert count == []
    assert c.size() == 5  # a's interval that holds b's start contributes its point, then the merge up to b's end
    assert count == [True]  # the host twin, once
    assert [c.time(i) for i in range(5)] == [0.0, 1800.0, 3600.0, 5400.0, 7200.0] and c.total_period().end == 2.5 * HOUR
    assert np.isnan(c.value(0)) and c(1800.0) == 3.0
    assert count == [True]  # cached
    assert d.value(1) == 3.0 and count == [True, True]


def test_a_nested_expression_is_evaluated_as_a_tree_not_from_its_cached_points():
    """(a*b)(t) between the points is a(t)*b(t), not the line through the product's points"""
    a, b = _ts([0.0, 2.0, 4.0], INST), _ts([0.0, 2.0, 4.0], INST)
    p = a * b
    assert list(p.values) == [0.0, 4.0, 16.0]  # now cached
    mid = _ts([0.0, 0.0], AVG, t0=HOUR // 2)
    assert list((p + mid).values)[1:3] == [1.0, 4.0]  # at 0.5 h: 1.0 * 1.0, not (0 + 4) / 2; at 1 h: 4.0


def test_set_after_evaluation_makes_the_series_concrete():
    """a cached result does not follow a later set() on a terminal (the reference's does, test_time_series.py:234-238)"""
    a, b = _ts([3.0, 3.0]), _ts([2.0, 2.0])
    c = a + b
    assert c.value(0) == 5.0
    b.set(0, 3.0)
    assert c.value(0) == 5.0 and (a + b).value(0) == 6.0
    c.set(1, 9.0)
    assert list((c * 1.0).values) == [5.0, 9.0]


def test_an_expression_is_accepted_where_a_series_is():
    ta = api.TimeAxis(0, 2 * HOUR, 2)
    a, b = _ts([1.0, 2.0, 3.0, 4.0], INST), _ts([4.0, 3.0, 2.0, 1.0], INST)
    lazy = api.TsVector([a + b * 2.0, api.max(a, b), (a - b).abs()])
    concrete = lazy.evaluate(host=True)
    assert all(x._impl is None for x in api.TsVector([a + b * 2.0, api.max(a, b)]))
    for got, want in zip(api.average(api.TsVector([a + b * 2.0, api.max(a, b), (a - b).abs()]), ta, host=True),
                         api.average(concrete, ta, host=True)):
        assert list(got.values) == list(want.values)
    got = api.percentiles(api.TsVector([a + b * 2.0, api.max(a, b), (a - b).abs()]), ta, [0, 50, 100])
    want = api.percentiles(concrete, ta, [0, 50, 100])
    assert [list(x.values) for x in got] == [list(x.values) for x in want]
    e = (a - b * 2.0).abs()  # 7, 4, 1, 2: the 1 is below the limit and filled from its neighbours
    assert list(e.min_max_check_linear_fill(1.5, 10.0).values) == [7.0, 4.0, 3.0, 2.0] == \
        list(e.evaluate(host=True).min_max_check_linear_fill(1.5, 10.0).values)
    assert list(copy.deepcopy(a + b).values) == [5.0, 5.0, 5.0, 5.0] and list(api.TimeSeries(a + b).values) == [5.0] * 4


def test_vector_operators_and_functions():
    a, b = _ts([1.0, 2.0]), _ts([4.0, 8.0])
    v, w = api.TsVector([a, b]), api.TsVector([b, a])
    vals = lambda tsv: [list(x.values) for x in tsv]  # noqa: E731
    assert isinstance(v + w, api.TsVector)
    assert vals(v + w) == [[5.0, 10.0]] * 2 and vals(v - w) == [[-3.0, -6.0], [3.0, 6.0]]
    assert vals(v * w) == [[4.0, 16.0]] * 2 and vals(v / w) == [[0.25, 0.25], [4.0, 4.0]]
    assert vals(v + 1.0) == vals(1.0 + v) == [[2.0, 3.0], [5.0, 9.0]]
    assert vals(v * 2.0) == vals(2.0 * v) == [[2.0, 4.0], [8.0, 16.0]]
    assert vals(v - 1.0) == [[0.0, 1.0], [3.0, 7.0]] and vals(1.0 - v) == [[0.0, -1.0], [-3.0, -7.0]]
    assert vals(v / 4.0) == [[0.25, 0.5], [1.0, 2.0]] and vals(8.0 / v) == [[8.0, 4.0], [2.0, 1.0]]
    assert vals(v + a) == vals(a + v) == [[2.0, 4.0], [5.0, 10.0]]
    assert vals(v - a) == [[0.0, 0.0], [3.0, 6.0]] and vals(a - v) == [[0.0, 0.0], [-3.0, -6.0]]
    assert vals(v / a) == [[1.0, 1.0], [4.0, 4.0]] and vals(b / v) == [[4.0, 4.0], [1.0, 1.0]]
    assert vals(-v) == [[-1.0, -2.0], [-4.0, -8.0]] and vals((-v).abs()) == vals(v)
    assert vals(v.min(w)) == [[1.0, 2.0]] * 2 and vals(v.max(3.0)) == [[3.0, 3.0], [4.0, 8.0]]
    assert vals(api.max(v, w)) == [[4.0, 8.0]] * 2 and vals(api.min(3.0, v)) == [[1.0, 2.0], [3.0, 3.0]]
    assert vals(api.max(a, v)) == [[1.0, 2.0], [4.0, 8.0]]
    assert vals(v.pow(2.0)) == [[1.0, 4.0], [16.0, 64.0]] and vals(api.pow(2.0, v)) == [[2.0, 4.0], [16.0, 256.0]]
    assert vals(api.pow(b, api.TsVector([a]))) == [[4.0, 64.0]]  # test_pow.py:30
    assert vals(api.TsVector([a]).pow(b)) == [[1.0, 256.0]]     # test_pow.py:31
    assert [x.time(0) for x in v.time_shift(HOUR)] == [HOUR, HOUR] == [x.time(0) for x in api.time_shift(v, HOUR)]
    # an empty side is neutral for + and - (time_series_dd.cpp:1035-1040, 1054-1059)
    assert vals(v + api.TsVector()) == vals(v) == vals(api.TsVector() + v) and vals(api.TsVector() - v) == vals(-v)
    assert [1] + api.TsVector([a]) == [1, a]  # a plain list still concatenates


def test_a_size_mismatch_raises_the_reference_s_text():
    a = _ts([1.0, 2.0])
    v, w = api.TsVector([a, a]), api.TsVector([a, a, a])
    texts = {"add": lambda: v + w, "sub": lambda: v - w, "multiply": lambda: v * w, "divide": lambda: v / w,
             "min": lambda: v.min(w), "max": lambda: api.max(v, w), "pow": lambda: v.pow(w)}
    for name, f in texts.items():
        with pytest.raises(RuntimeError) as e:
            f()
        assert str(e.value) == f"ts-vector {name} require same sizes: lhs.size=2,rhs.size=3"


def test_vector_evaluate_is_one_call(count):
    a, b = _ts([1.0, 2.0, 3.0]), _ts([2.0, 2.0], INST, t0=HOUR // 2)
    v = api.TsVector([a + b, a * 2.0, a, (a - b).abs()])
    r = v.evaluate(host=True)
    assert count == [True] and all(x._impl is not None for x in v)
    assert [x.size() for x in r] == [5, 3, 3, 5] and list(r[1].values) == [2.0, 4.0, 6.0]
    assert list(r[2].values) == [1.0, 2.0, 3.0]
    r[2].set(0, 7.0)
    assert a.value(0) == 1.0  # the results are copies
    assert v.evaluate(host=True)[0].size() == 5 and count == [True]  # nothing left to evaluate


def test_a_concrete_series_behaves_as_before():
    ta = api.TimeAxis(0, HOUR, 3)
    a = api.TimeSeries(ta, [1.0, 2.0, 4.0], INST)
    assert a._expr is None and a._impl is a._ts
    assert (a.size(), len(a), a.value(1), a.time(2), a(1800), a.point_interpretation()) == (3, 3, 2.0, 7200.0, 1.5, INST)
    a.set(1, 3.0)
    assert list(a.values) == [1.0, 3.0, 4.0] and list(a.v) == [1.0, 3.0, 4.0]
    assert (a.total_period().start, a.total_period().end) == (0.0, 3 * HOUR)
    b = api.TimeSeries(a)
    b.set(0, 9.0)
    assert a.value(0) == 1.0 and copy.deepcopy(a).value(2) == 4.0
    assert list(a.average(api.TimeAxis(0, 3 * HOUR, 1)).values) == list(api.average(a, api.TimeAxis(0, 3 * HOUR, 1)).values)
    f = api.TimeSeries(ta, fill_value=2.5, point_fx=AVG)
    assert list(f.values) == [2.5] * 3 and f.point_interpretation() == AVG
    p = api.TsFactory().create_time_point_ts(api.UtcPeriod(0, 10), [0, 3, 7], [1.0, 2.0, 3.0])
    assert p.size() == 3 and p.total_period().end == 10.0
