"""convolve_w, derivative, inside and decode on the host entries (shyft_hip_ts_*_host, host=True;
host/ts_filter.hpp) and through the api: the reference's own test numbers restated as data
(test/time_series_derivative_test.cpp, test/time_series_decode_test.cpp, shyft/tests/api/test_convolve_ts.py), the host
against ordered-loop restatements written here on the GPU test's batches at reduced size, and the refusals. No GPU."""
import math

import numpy as np
import pytest

from shyft_amd import api, region
from shyft_amd._native import ShyftHipError
from tests import resample_cases as rc
from tests import tsfilter_cases as fc

NAN = float("nan")
AVG, INST = api.POINT_AVERAGE_VALUE, api.POINT_INSTANT_VALUE
METHODS = (api.DEFAULT, api.FORWARD, api.BACKWARD, api.CENTER)


def _on_fixed(values, fx, dt=10):
    return api.TimeSeries(api.TimeAxis(0, dt, len(values)), values, fx)


def _on_points(values, fx, dt=10):
    n = len(values)
    return api.TsFactory().create_time_point_ts(api.UtcPeriod(0, dt * n), [dt * i for i in range(n)], values, fx)


def _equal(got, expected, what=""):
    """== where the expected value is finite, NaN where it is not"""
    got = list(got)
    assert len(got) == len(expected), what
    for i, (g, e) in enumerate(zip(got, expected)):
        if math.isnan(e):
            assert math.isnan(g), (what, i, g)
        else:
            assert g == e, (what, i, g, e)


# ---- derivative: test/time_series_derivative_test.cpp -----------------------------------------------------------------
def test_fixed_step_is_remembered():
    f, p = _on_fixed([1.0, 2.0], AVG), _on_points([1.0, 2.0], AVG)
    assert f._ts._fixed_dt_us == 10 * 10**6 and p._ts._fixed_dt_us == 0
    import copy
    assert copy.deepcopy(f)._ts._fixed_dt_us == 10 * 10**6
    assert f._ts._with_values([3.0, 4.0], INST)._fixed_dt_us == 10 * 10**6
    assert f.inside(0.0, 1.5)._ts._fixed_dt_us == 10 * 10**6 and p.inside(0.0, 1.5)._ts._fixed_dt_us == 0
    with pytest.raises(AttributeError):
        f._ts._fixed_dt_us = 5


@pytest.mark.parametrize("make", (_on_fixed, _on_points))
def test_linear_derivative(make):
    """tc_ts_linear_derivative (:26-47): the slope to the next point, NaN at the last; every method the same"""
    f = make([1.0, 1.0, 2.0, 3.0, -1.0, 5.0], INST)
    for m in METHODS:
        d = f.derivative(m)
        assert d.size() == f.size() and d.point_interpretation() == AVG
        _equal(d.values, [0.0 / 10.0, 1.0 / 10.0, 1.0 / 10.0, -4.0 / 10.0, 6.0 / 10.0, NAN], m)
    assert list(f.derivative().values)[:5] == pytest.approx([0.0, 0.1, 0.1, -0.4, 0.6])  # the reference's literals


STAIR = [1.0, 1.0, 2.0, NAN, -1.0, 5.0]
# the fixed-step branch divides by to_seconds(2 * dt) and to_seconds(dt) (time_series_dd.cpp:322-357); the variable
# branch doubles the difference over the sum of the start and the end distances (:367-443)
STAIR_EXPECTED = {
    (_on_fixed, api.DEFAULT): [0.0 / 20.0, 1.0 / 20.0, 1.0 / 20.0, NAN, 6.0 / 20.0, 6.0 / 20.0],
    (_on_points, api.DEFAULT): [0.0 / 20.0, 2 * 1.0 / 40.0, 1.0 / 20.0, NAN, 6.0 / 20.0, 6.0 / 20.0],
    (_on_fixed, api.FORWARD): [0.0 / 10.0, 1.0 / 10.0, 0.0, NAN, 6.0 / 10.0, 0.0],
    (_on_points, api.FORWARD): [2 * 0.0 / 20.0, 2 * 1.0 / 20.0, 0.0, NAN, 2 * 6.0 / 20.0, 0.0],
    (_on_fixed, api.BACKWARD): [0.0, 0.0 / 10.0, 1.0 / 10.0, NAN, 0.0, 6.0 / 10.0],
    (_on_points, api.BACKWARD): [0.0, 2 * 0.0 / 20.0, 2 * 1.0 / 20.0, NAN, 0.0, 2 * 6.0 / 20.0],
}


@pytest.mark.parametrize("make", (_on_fixed, _on_points))
@pytest.mark.parametrize("method", (api.DEFAULT, api.FORWARD, api.BACKWARD))
def test_stair_case_derivative(make, method):
    """tc_ts_stair_case_derivative, _fwd_, _bwd_ (:49-109)"""
    d = make(STAIR, AVG).derivative(method)
    assert d.point_interpretation() == AVG
    _equal(d.values, STAIR_EXPECTED[make, method], method)
    if method == api.DEFAULT:
        _equal(make(STAIR, AVG).derivative(api.CENTER).values, STAIR_EXPECTED[make, method], "center")
        _equal(make(STAIR, AVG).derivative().values, STAIR_EXPECTED[make, method], "no argument")
    # the reference's tables (doctest::Approx)
    table = {api.DEFAULT: [0.0, 1 / 20.0, 1 / 20.0, NAN, 6 / 20.0, 6 / 20.0],
             api.FORWARD: [0.0, 1 / 10.0, 0.0, NAN, 6 / 10.0, 0.0],
             api.BACKWARD: [0.0, 0.0, 1 / 10.0, NAN, 0.0, 6 / 10.0]}[method]
    assert list(d.values) == pytest.approx(table, nan_ok=True)


@pytest.mark.parametrize("make", (_on_fixed, _on_points))
@pytest.mark.parametrize("method", METHODS)
def test_stair_case_one_value_and_one_segment(make, method):
    """tc_ts_stair_case_one_value (:111-122) and tc_ts_linear_one_segment (:124-135), every method"""
    _equal(make([0.0], AVG).derivative(method).values, [0.0])
    _equal(make([NAN], AVG).derivative(method).values, [NAN])
    _equal(make([math.inf], AVG).derivative(method).values, [NAN])
    fixed = make is _on_fixed
    one = {api.DEFAULT: [1.0 / 2.0, 1.0 / 2.0], api.CENTER: [1.0 / 2.0, 1.0 / 2.0],
           api.FORWARD: [1.0 / 1.0 if fixed else 2 * 1.0 / 2.0, 0.0],
           api.BACKWARD: [0.0, 1.0 / 1.0 if fixed else 2 * 1.0 / 2.0]}[method]
    _equal(make([0.0, 1.0], AVG, dt=1).derivative(method).values, one, method)
    _equal(make([NAN, 1.0], AVG, dt=1).derivative(method).values, [NAN, 0.0], method)


def test_derivative_inside_issue():
    """derivative_inside_issue (:176-196): the derivative of a constant series is finite everywhere"""
    orig = api.TimeSeries(api.TimeAxis(0, 10, 6), fill_value=1.0, point_fx=AVG)
    d = orig.derivative()
    assert all(math.isfinite(x) for x in d.values)
    a = d.inside(NAN, NAN, NAN, 1.0, 0.0)
    assert list(a.values) == [1.0] * 6
    b = (orig + orig.derivative().inside(NAN, NAN, NAN, 1.0, 0.0)).inside(NAN, NAN, NAN, 1.0, 0.0)  # a lazy operand
    assert list(b.values) == [1.0] * 6 and b.size() == 6


# ---- convolve_w: shyft/tests/api/test_convolve_ts.py ------------------------------------------------------------------
W5 = [0.05, 0.15, 0.6, 0.15, 0.05]


def _ordered_sum(terms):
    v = 0.0
    for x in terms:
        v += x
    return v


def test_convolve_mass_balance_case():
    source = api.TimeSeries(api.TimeAxis(0, 3600, 24), fill_value=10.0, point_fx=AVG)
    first = source.convolve_w(W5, api.convolve_policy.USE_FIRST)
    assert first.size() == 24 and first.point_interpretation() == AVG
    assert list(first.values) == [10.0] * 24
    assert source.convolve_w(api.DoubleVector(W5), api.USE_FIRST).values == first.values
    zero = list(source.convolve_w(W5, api.USE_ZERO).values)
    nan = list(source.convolve_w(W5, api.USE_NAN).values)
    for i in range(4):  # the partial sums, then 0.0 for every tap before the first point
        assert zero[i] == _ordered_sum([w * 10.0 for w in W5[:i + 1]] + [0.0] * (4 - i)), i
        assert math.isnan(nan[i])
    assert zero[4:] == [10.0] * 20 and nan[4:] == [10.0] * 20
    assert zero[0] == 0.5 and zero[3] == pytest.approx(9.5)
    inst = api.TimeSeries(api.TimeAxis(0, 3600, 4), [1.0, 2.0, 3.0, 4.0], INST).convolve_w([1.0], api.USE_ZERO)
    assert inst.point_interpretation() == INST and list(inst.values) == [1.0, 2.0, 3.0, 4.0]


def test_convolve_edges():
    source = _on_fixed([1.0, 2.0, 4.0], AVG)
    for policy in (api.USE_FIRST, api.USE_ZERO, api.USE_NAN):
        assert list(source.convolve_w([], policy).values) == [0.0, 0.0, 0.0]  # K == 0
    w = [1.0, 10.0, 100.0, 1000.0, 10000.0]  # K > n
    assert list(source.convolve_w(w, api.USE_FIRST).values) == [11111.0, 11112.0, 11124.0]
    assert list(source.convolve_w(w, api.USE_ZERO).values) == [1.0, 12.0, 124.0]
    assert all(math.isnan(x) for x in source.convolve_w(w, api.USE_NAN).values)
    spike = _on_fixed([1.0, math.inf, 2.0, 3.0], AVG)  # an inf input against a zero weight is NaN
    _equal(spike.convolve_w([1.0, 0.0], api.USE_ZERO).values, [1.0, math.inf, NAN, 3.0])
    _equal(spike.convolve_w([0.0], api.USE_ZERO).values, [0.0, NAN, 0.0, 0.0])
    _equal(_on_fixed([math.inf, 1.0], AVG).convolve_w([1.0, 0.0], api.USE_FIRST).values, [NAN, NAN])
    assert [int(p) for p in api.convolve_policy] == [0, 1, 2] and api.USE_NAN is api.convolve_policy.USE_NAN
    assert [int(m) for m in api.derivative_method] == [0, 1, 2, 3] and api.CENTER is api.derivative_method.CENTER


# ---- inside -----------------------------------------------------------------------------------------------------------
def test_inside_table():
    """inside_parameter::inside_value (time_series_dd.h:1546-1554): [min, max), a NaN limit is no limit"""
    x = [-1.0, 0.0, 0.5, 1.0, 2.0, NAN, math.inf, -math.inf]
    for fx in (AVG, INST):
        ts = _on_points(x, fx)
        r = ts.inside(0.0, 1.0)
        assert r.point_interpretation() == fx
        _equal(r.values, [0.0, 1.0, 1.0, 0.0, 0.0, NAN, NAN, NAN])
        _equal(ts.inside(NAN, 1.0).values, [1.0, 1.0, 1.0, 0.0, 0.0, NAN, NAN, NAN])
        _equal(ts.inside(0.0, NAN).values, [0.0, 1.0, 1.0, 1.0, 1.0, NAN, NAN, NAN])
        _equal(ts.inside(NAN, NAN).values, [1.0, 1.0, 1.0, 1.0, 1.0, NAN, NAN, NAN])
        _equal(ts.inside(math.inf, -math.inf).values, [1.0, 1.0, 1.0, 1.0, 1.0, NAN, NAN, NAN])  # not finite: no limit
        _equal(ts.inside(0.0, 1.0, -9.0, 7.0, 3.0).values, [3.0, 7.0, 7.0, 3.0, 3.0, -9.0, -9.0, -9.0])
        _equal(ts.inside(0.0, 1.0, nan_v=5.0).values, [0.0, 1.0, 1.0, 0.0, 0.0, 5.0, 5.0, 5.0])


# ---- decode: test/time_series_decode_test.cpp -------------------------------------------------------------------------
def test_decode_loops_of_the_reference():
    low = _on_fixed([float(i) for i in range(1024)], INST).decode(0, 1)  # :44-48
    assert low.point_interpretation() == INST
    assert list(low.values) == [float(i & 1) for i in range(1024)]
    assert list(_on_fixed([float(2**51), float(2**51 + 1)], AVG).decode(0, 1).values) == [0.0, 1.0]  # :52-55
    for start_bit in range(10):  # :59-69
        for n_bits in range(1, 10):
            max_val = (1 << n_bits) - 1
            got = _on_fixed([float(max_val << start_bit), 0.0, float(1 << start_bit)], AVG).decode(start_bit, n_bits)
            assert list(got.values) == [float(max_val), 0.0, 1.0], (start_bit, n_bits)
    x = [float((1 << 9) + (2 << 1) + 1), float(7 << 1), float((1 << 9) + (5 << 1) + 1)]  # :74-90
    groups = _on_fixed(x, AVG)
    assert list(groups.decode(0, 1).values) == [1.0, 0.0, 1.0]
    assert list(groups.decode(1, 3).values) == [2.0, 7.0, 5.0]
    assert list(groups.decode(9, 1).values) == [1.0, 0.0, 1.0]
    bad = _on_fixed([NAN, -2.3, float(2**52) + 1.0, math.inf, -0.5, float(2**52), float(2**52) - 1.0, 6.9], AVG)
    _equal(bad.decode(0, 1).values, [NAN, NAN, NAN, NAN, NAN, 0.0, 1.0, 0.0])  # :95-97; 2^52 itself is decoded
    _equal(bad.decode(1, 50).values, [NAN, NAN, NAN, NAN, NAN, 0.0, float(2**50 - 1), 3.0])


def test_decode_refusals():
    ts = _on_fixed([1.0, 2.0], AVG)
    empty = api.TimeSeries(api.TimeAxis(0, 10, 0), [], AVG)
    for start in (-1, 52):
        for x in (ts, empty):
            with pytest.raises(RuntimeError, match=rf"start_bit must be in range \[0\.\.51\], was {start}$"):
                x.decode(start, 1)
    for start, bits in ((0, 0), (0, -3), (0, 52), (51, 1), (40, 12)):
        for x in (ts, empty):
            with pytest.raises(RuntimeError, match=rf"n_bits must be > 0 and start_bit\+n_bits <= 51: n_bits ={bits}, "
                                                   rf"start_bit={start}$"):
                x.decode(start, bits)
    assert list(ts.decode(50, 1).values) == [0.0, 0.0] and list(ts.decode(0, 51).values) == [1.0, 2.0]


# ---- the host against ordered loops written here ------------------------------------------------------------------------
def _to_seconds(dt):
    return float(dt) / 1e6


def _loop_convolve(b, w_row, w, w_of, policy):
    """convolve_w_ts::value for every point: one accumulator per point, the taps added in ascending j"""
    row, _, v, _, _ = b
    out = np.empty(len(v))
    with np.errstate(all="ignore"):
        for s in range(len(row) - 1):
            x = v[row[s]:row[s + 1]]
            n = len(x)
            ws = w[w_row[w_of[s]]:w_row[w_of[s] + 1]]
            acc = np.zeros(n)
            for j, wj in enumerate(ws):  # every point takes tap j before any takes tap j + 1
                term = np.empty(n)
                head = min(j, n)
                if n:
                    term[:head] = wj * x[0] if policy[s] == fc.USE_FIRST else (0.0 if policy[s] == fc.USE_ZERO else NAN)
                term[head:] = wj * x[:n - head]
                acc = acc + term
            out[row[s]:row[s + 1]] = acc
    return out


def _loop_derivative_fx(t, t_end, v, dt, dm):
    """derivative_fx (time_series_dd.cpp:311-448) in place over the whole vector, loop by loop as the reference"""
    fin = math.isfinite
    n = len(v)
    v = list(v)
    period = lambda i: (t[i], t[i + 1] if i + 1 < n else t_end)  # noqa: E731
    if n < 2:
        if n:
            v[0] = 0.0 if fin(v[0]) else NAN
        return v
    if dt > 0:
        if dm in (fc.DEFAULT, fc.CENTER):
            v0 = v[0]
            v[0] = ((v[1] - v0) / _to_seconds(2 * dt) if fin(v[1]) else 0.0) if fin(v0) else NAN
            for i in range(1, n - 1):
                v1 = v[i]
                if fin(v1):
                    if fin(v0):
                        v[i] = (v[i + 1] - v0) / _to_seconds(2 * dt) if fin(v[i + 1]) else (v1 - v0) / _to_seconds(2 * dt)
                    else:
                        v[i] = (v[i + 1] - v1) / _to_seconds(2 * dt) if fin(v[i + 1]) else 0.0
                else:
                    v[i] = NAN
                v0 = v1
            v[-1] = ((v[-1] - v0) / _to_seconds(2 * dt) if fin(v0) else 0.0) if fin(v[-1]) else NAN
        elif dm == fc.FORWARD:
            for i in range(n - 1):
                v[i] = ((v[i + 1] - v[i]) / _to_seconds(dt) if fin(v[i + 1]) else 0.0) if fin(v[i]) else NAN
            v[-1] = 0.0 if fin(v[-1]) else NAN
        else:
            for i in range(n - 1, 0, -1):
                v[i] = ((v[i] - v[i - 1]) / _to_seconds(dt) if fin(v[i - 1]) else 0.0) if fin(v[i]) else NAN
            v[0] = 0.0 if fin(v[0]) else NAN
        return v
    if dm in (fc.DEFAULT, fc.CENTER):
        v0 = v[0]
        p0, p1 = period(0), period(1)
        v[0] = ((v[1] - v[0]) / _to_seconds(p1[1] - p0[0]) if fin(v[1]) else 0.0) if fin(v0) else NAN
        for i in range(1, n - 1):
            p1, v1, p2, v2 = period(i), v[i], period(i + 1), v[i + 1]
            if fin(v1):
                if fin(v0):
                    if fin(v2):
                        v[i] = 2 * (v2 - v0) / _to_seconds((p2[0] - p0[0]) + (p2[1] - p0[1]))
                    else:
                        v[i] = (v1 - v0) / _to_seconds(p1[1] - p0[0])
                elif fin(v2):
                    v[i] = (v2 - v1) / _to_seconds(p2[1] - p1[0])
                else:
                    v[i] = 0.0
            else:
                v[i] = NAN
            v0, p0 = v1, p1
        p1, v1 = period(n - 1), v[-1]
        v[-1] = ((v1 - v0) / _to_seconds(p1[1] - p0[0]) if fin(v0) else 0.0) if fin(v1) else NAN
    elif dm == fc.FORWARD:
        p0, v0 = period(0), v[0]
        for i in range(n - 1):
            p1, v1 = period(i + 1), v[i + 1]
            if fin(v0):
                v[i] = 2 * (v1 - v0) / _to_seconds((p1[0] - p0[0]) + (p1[1] - p0[1])) if fin(v1) else 0.0
            else:
                v[i] = NAN
            p0, v0 = p1, v1
        v[-1] = 0.0 if fin(v[-1]) else NAN
    else:
        p0, v0 = period(0), v[0]
        v[0] = 0.0 if fin(v[0]) else NAN
        for i in range(1, n):
            p1, v1 = period(i), v[i]
            if fin(v1):
                v[i] = 2 * (v1 - v0) / _to_seconds((p1[0] - p0[0]) + (p1[1] - p0[1])) if fin(v0) else 0.0
            else:
                v[i] = NAN
            p0, v0 = p1, v1
    return v


def _loop_derivative(b, fixed_dt, method):
    """derivative_ts::values (time_series_dd.cpp:450-463)"""
    row, t, v, t_end, fx = b
    out = np.empty(len(v))
    for s in range(len(row) - 1):
        ts = [int(x) for x in t[row[s]:row[s + 1]]]
        vs = [float(x) for x in v[row[s]:row[s + 1]]]
        if fx[s] == 0:
            for i in range(len(vs) - 1):
                vs[i] = (vs[i + 1] - vs[i]) / _to_seconds(ts[i + 1] - ts[i])
            if vs:
                vs[-1] = NAN
        else:
            vs = _loop_derivative_fx(ts, int(t_end[s]), vs, int(fixed_dt[s]), int(method[s]))
        out[row[s]:row[s + 1]] = vs
    return out


def _loop_inside(b, min_x, max_x, nan_x, x_in, x_out):
    row, _, v, _, _ = b
    out = np.empty(len(v))
    for s in range(len(row) - 1):
        for k in range(row[s], row[s + 1]):
            x = v[k]
            if not math.isfinite(x):
                out[k] = nan_x[s]
            elif math.isfinite(min_x[s]) and x < min_x[s]:
                out[k] = x_out[s]
            elif math.isfinite(max_x[s]) and x >= max_x[s]:
                out[k] = x_out[s]
            else:
                out[k] = x_in[s]
    return out


def _loop_decode(b, start_bit, n_bits):
    row, _, v, _, _ = b
    out = np.empty(len(v))
    for s in range(len(row) - 1):
        for k in range(row[s], row[s + 1]):
            x = float(v[k])
            if not math.isfinite(x) or x < 0 or x > float(1 << 52):
                out[k] = NAN
            else:
                out[k] = float((int(x) >> int(start_bit[s])) & ((1 << int(n_bits[s])) - 1))
    return out


REDUCED = ((0, 1), (1, 9), (2, 20))  # (time base, S): the GPU test's batches at reduced size


@pytest.mark.parametrize("k,S", REDUCED)
def test_host_convolve_equals_the_ordered_loop(k, S):
    _, _, b, _ = fc.batch(S, k)
    Ks = (0, 1, 5, 65, 300)
    w_row, w = fc.profiles(Ks, 50 + S, nan_in=(3,))
    for shift in range(3):
        policy = np.array([(s + shift) % 3 for s in range(S)], np.int32)
        w_of = np.array([(s + shift) % len(Ks) for s in range(S)], np.int64)
        fc.same(region.ts_convolve_w_csr(*b, w_row, w, w_of, policy, host=True), _loop_convolve(b, w_row, w, w_of, policy),
                ("per series", shift))
    one = fc.weights(7, 3)
    shared = region.ts_convolve_w_csr(*b, [0, 7], one, 0, fc.USE_FIRST, host=True)
    fc.same(shared, _loop_convolve(b, [0, 7], one, [0] * S, [fc.USE_FIRST] * S), "shared")
    row = b[0]
    for s in range(S):  # the api's method on one series is the same call
        if row[s + 1] - row[s] in (3, 64):
            ts = api.TimeSeries(_impl=api._api._PointTs._from_us(b[1][row[s]:row[s + 1]], int(b[3][s]),
                                                                 b[2][row[s]:row[s + 1]],
                                                                 api.point_interpretation_policy(int(b[4][s]))))
            fc.same(np.asarray(ts.convolve_w(one, api.USE_FIRST).values), shared[row[s]:row[s + 1]], s)


@pytest.mark.parametrize("k,S", REDUCED)
def test_host_derivative_equals_the_in_place_loops(k, S):
    _, dt, b, fixed = fc.batch(S, k)
    hazards = fc.with_nan_runs(b)
    for bb in (b, hazards, (b[0], b[1], b[2], b[3], np.ones(S, np.int32))):  # the last: every series stair-case
        for m in range(4):
            for fdt in (fixed, np.zeros(S, np.int64)):
                got = region.ts_derivative_csr(*bb, fdt, m, host=True)
                fc.same(got, _loop_derivative(bb, fdt, [m] * S), (m, int(fdt.max())))
    per_series = np.arange(S, dtype=np.int32) % 4
    fc.same(region.ts_derivative_csr(*b, fixed, per_series, host=True), _loop_derivative(b, fixed, per_series), "methods")


def test_derivative_branches_differ_only_where_doubling_overflows():
    """on an evenly spaced axis 2 * (v2 - v0) / (2 * dt seconds) equals (v2 - v0) / (2 * dt seconds) unless the
    doubling overflows; which branch a series takes is therefore an input"""
    t0, dt = rc.EPOCHS[0]
    t = t0 + dt * np.arange(3)
    v = [-1.5e308, 0.0, 1.5e308]  # v2 - v0 overflows by itself in both branches, v1 - v0 only when doubled
    args = ([0, 3], t, v, [t0 + 3 * dt], [1])
    fixed = region.ts_derivative_csr(*args, dt, fc.FORWARD, host=True)
    variable = region.ts_derivative_csr(*args, 0, fc.FORWARD, host=True)
    assert fixed[0] == 1.5e308 / _to_seconds(dt) and variable[0] == math.inf
    rng = np.random.default_rng(2)
    vv = rng.normal(0, 5, 40)
    even = ([0, 40], t0 + dt * np.arange(40), vv, [t0 + 40 * dt], [1])
    for m in range(4):
        fc.same(region.ts_derivative_csr(*even, dt, m, host=True), region.ts_derivative_csr(*even, 0, m, host=True), m)


@pytest.mark.parametrize("k,S", REDUCED)
def test_host_inside_and_decode_equal_the_loops(k, S):
    _, _, b, _ = fc.batch(S, k)
    v = b[2].copy()
    v[::7] = 2.0   # exactly on min_x of some series
    v[3::7] = 9.0  # exactly on max_x
    b = (b[0], b[1], v, b[3], b[4])
    p = (np.where(np.arange(S) % 3, 2.0, NAN), np.where(np.arange(S) % 2, 9.0, NAN), np.where(np.arange(S) % 4, NAN, -1.0),
         1.0 + np.arange(S), -1.0 - np.arange(S))
    fc.same(region.ts_inside_csr(*b, *p, host=True), _loop_inside(b, *p), "inside")
    fc.same(region.ts_inside_csr(*b, 2.0, 9.0, host=True), _loop_inside(b, [2.0] * S, [9.0] * S, [NAN] * S, [1.0] * S, [0.0] * S),
            "defaults")
    d = fc.decode_values(b, 77 + S)
    start, bits = np.arange(S, dtype=np.int32) % 50, 1 + np.arange(S, dtype=np.int32) % 2
    bits[0], start[0] = 51, 0
    got = region.ts_decode_csr(*d, start, bits, host=True)
    fc.same(got, _loop_decode(d, start, bits), "decode")
    assert np.isnan(got).any() and np.isfinite(got).any()


# ---- refusals, with the same text from both twins (no device is needed to refuse) -----------------------------------------
H = rc.HOUR
GOOD = ([0, 3, 5], [0, H, 2 * H, 0, H], [1.0, 2.0, 3.0, 4.0, 5.0], [3 * H, 2 * H], [1, 0])
CALLS = {
    "convolve": lambda b, host, **kw: region.ts_convolve_w_csr(*b, **{"w_row": [0, 2], "w": [0.5, 0.5], "host": host, **kw}),
    "derivative": lambda b, host, **kw: region.ts_derivative_csr(*b, host=host, **kw),
    "inside": lambda b, host, **kw: region.ts_inside_csr(*b, 0.0, 1.0, host=host, **kw),
    "decode": lambda b, host, **kw: region.ts_decode_csr(*b, **{"start_bit": 0, "n_bits": 1, "host": host, **kw}),
}


def _refused(name, text, b=GOOD, **kw):
    for host in (True, False):
        with pytest.raises(ShyftHipError, match=text):
            CALLS[name](b, host, **kw)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_series_refusals(name):
    row, t, v, t_end, fx = GOOD
    _refused(name, "needs time-points in increasing order", (row, [0, 2 * H, H, 0, H], v, t_end, fx))
    _refused(name, "illegal end-of-axis", (row, t, v, [2 * H, 2 * H], fx))
    _refused(name, "ts_filter: fx must be POINT_INSTANT_VALUE or POINT_AVERAGE_VALUE", (row, t, v, t_end, [1, 2]))
    _refused(name, "ts_filter: row must not decrease", ([0, 4, 3, 5], t, v, [5 * H, 5 * H, 5 * H], [0, 0, 0]))
    _refused(name, "ts_filter: times beyond a quarter of the 64-bit range", (row, t, v, [3 * H, 2**62], fx))


def test_parameter_refusals():
    _refused("convolve", r"convolve_w: w_row\[0\] must be 0", w_row=[1, 2], w=[0.5, 0.5])
    _refused("convolve", "convolve_w: w_row must not decrease", w_row=[0, 2, 1], w=[0.5])
    for w_of in (-1, 1, [0, 7]):
        _refused("convolve", "convolve_w: w_of is out of range", w_of=w_of)
    for policy in (-1, 3, [0, 5]):
        _refused("convolve", "convolve_w: policy must be USE_FIRST, USE_ZERO or USE_NAN", policy=policy)
    for method in (-1, 4, [0, 9]):
        _refused("derivative", "derivative: method must be DEFAULT, FORWARD, BACKWARD or CENTER", method=method)
    _refused("derivative", "derivative: fixed_dt must not be negative", fixed_dt=[H, -1])
    _refused("derivative", "derivative: fixed_dt is not the spacing of the series", fixed_dt=[H + 1, 0])
    uneven = ([0, 3], [0, H, 2 * H + 1], [1.0, 2.0, 3.0], [3 * H + 1], [1])
    _refused("derivative", "derivative: fixed_dt is not the spacing of the series", uneven, fixed_dt=H)
    long_end = ([0, 3], [0, H, 2 * H], [1.0, 2.0, 3.0], [3 * H + 1], [1])
    _refused("derivative", "derivative: fixed_dt is not the spacing of the series", long_end, fixed_dt=H)
    region.ts_derivative_csr(*GOOD, [H, H], 0, host=True)  # both series evenly spaced
    for start in (-1, 52):
        _refused("decode", rf"start_bit must be in range \[0\.\.51\], was {start}$", start_bit=[0, start])
    for start, bits in ((0, 0), (51, 1), (3, 49), (0, 2**31 - 1)):
        _refused("decode", rf"n_bits must be > 0 and start_bit\+n_bits <= 51: n_bits ={bits}, start_bit={start}$",
                 start_bit=start, n_bits=bits)
    with pytest.raises(ShyftHipError, match="tsfilter: path must be AUTO, DIRECT or TILED"):
        region.tsfilter_set_path(3)


def test_the_cap_on_the_weights_is_the_device_entry_s():
    one = ([0, 1], [0], [2.0], [H], [1])
    w = np.full(65537, 0.5)
    with pytest.raises(ShyftHipError, match="convolve_w: more than 65536 weights in a profile are not supported on the device"):
        region.ts_convolve_w_csr(*one, [0, 65537], w)
    assert region.ts_convolve_w_csr(*one, [0, 65537], w, host=True)[0] == 65537.0  # USE_FIRST: 65537 times 0.5 * 2.0


def test_empties_need_no_device():
    none = (np.zeros(1, np.int64), [], [], [], [])   # S == 0
    no_points = ([0, 0, 0], [], [], [5, 5], [0, 1])  # two series without points
    for b in (none, no_points):
        for host in (True, False):
            for name in CALLS:
                assert CALLS[name](b, host).shape == (0,)
    empty = api.TsVector()
    assert len(empty.derivative()) == 0 and len(empty.inside(0.0, 1.0)) == 0
    assert len(empty.convolve_w([1.0], api.USE_ZERO)) == 0 and len(empty.decode(0, 1)) == 0
    no_values = api.TimeSeries(api.TimeAxis(0, 10, 0), [], AVG)
    assert no_values.derivative().size() == 0 and no_values.convolve_w([1.0], api.USE_NAN).size() == 0
