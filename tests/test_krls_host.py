"""KRLS interpolation on the host: api.KrlsRbfPredictor, TimeSeries.krls_interpolation / get_krls_predictor and
region.krls_train_csr / krls_predict with host=True (csrc/host/krls.hpp).

The reference's two tests (shyft/tests/api/test_time_series.py:1211-1261) are restated with their bounds. The algorithm
is then pinned against a statement of its own in this file, written with Python floats from the issue's steps (Engel,
Mannor, Meir 2004, as dlib implements them), with detmath's exp as tests/test_detmath.py reaches it and the same
summation orders: bitwise. Parity with dlib's last bit is not pinned anywhere."""
import numpy as np
import pytest

from shyft_amd import api, region
from tests import oracle_lib
from tests.krls_cases import GROW, HOUR, MIXED, T0, US, csr, grow_series, noisy_sine, same_bits, same_state


# ---- the reference's tests ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sine():
    ta = api.TimeAxis(T0 // US, api.deltahours(1), 30 * 24)
    data = np.sin(np.linspace(0, 2 * np.pi, ta.size()))
    return ta, data, api.TimeSeries(ta, data, api.POINT_INSTANT_VALUE)


def test_reference_krls_ts(sine):
    """test_krls_ts: assertAlmostEqual(places=1) is |difference| < 0.05"""
    ta, data, ts = sine
    k = ts.krls_interpolation(api.deltahours(3))
    assert len(k) == len(ts)
    assert k.point_interpretation() == api.POINT_INSTANT_VALUE
    assert [k.time(i) for i in (0, 1, 719)] == [ts.time(i) for i in (0, 1, 719)]
    assert np.abs(np.array(k.values) - data).max() < 0.05


def test_reference_get_krls_predictor(sine):
    """test_ts_get_krls_predictor: places=1 is 0.05, places=2 is 0.005"""
    ta, data, ts = sine
    pred = ts.get_krls_predictor(api.deltahours(3))
    ts_krls = pred.predict(ta)
    assert len(ts_krls) == len(ts)
    ts_mse = pred.mse_ts(ts)
    assert len(ts_mse) == len(ts)
    assert np.abs(np.array(ts_krls.values) - data).max() < 0.05
    assert np.abs(np.array(ts_mse.values)).max() < 0.005
    assert abs(pred.predictor_mse(ts)) < 0.005
    assert 0 < pred.dictionary_size < region.KRLS_LDS_CAPACITY
    assert (pred.dt, pred.gamma, pred.tolerance, pred.size) == (3 * 3600, 1e-3, 0.01, 1000000)
    assert ts_krls.point_interpretation() == api.POINT_AVERAGE_VALUE  # predicted_point_fx's default
    assert ts_mse.point_interpretation() == api.POINT_INSTANT_VALUE   # the source's


# ---- an independent statement ------------------------------------------------------------------------------------------
def _dot64(u, v):
    p = [0.0] * 64
    for i in range(len(u)):
        p[i & 63] = p[i & 63] + u[i] * v[i]
    o = 32
    while o >= 1:
        for l in range(o):
            p[l] = p[l] + p[l + o]
        o //= 2
    return p[0]


class Model:
    """the issue's steps with Python floats (IEEE doubles, no contraction); grows, updates, never removes"""

    def __init__(self, exp, dt_us, gamma, tolerance):
        self.exp, self.gamma, self.tolerance = exp, gamma, tolerance
        self.scaling = 1.0 / (dt_us / 1e6)
        self.d, self.alpha, self.Kinv, self.P = [], [], [], []
        self.grown = self.updated = 0

    def kern(self, a, b):
        return self.exp(-self.gamma * ((a - b) * (a - b)))

    def position(self, t_us):
        return (t_us / 1e6) * self.scaling

    def train_one(self, x, y):
        m = len(self.d)
        if m == 0:
            self.d, self.alpha, self.Kinv, self.P = [x], [y / 1.0], [[1.0 / 1.0]], [[1.0]]
            k = [self.kern(x, x)]
            return _dot64(self.alpha, k)
        k = [self.kern(x, di) for di in self.d]
        a = []
        for i in range(m):
            acc = 0.0
            for j in range(m):
                acc = acc + self.Kinv[i][j] * k[j]
            a.append(acc)
        delta = 1.0 - _dot64(k, a)
        e = y - _dot64(k, self.alpha)
        if delta > self.tolerance:
            self.grown += 1
            for i in range(m):
                for j in range(m):
                    self.Kinv[i][j] = self.Kinv[i][j] + (a[i] * a[j]) / delta
                self.Kinv[i].append(-a[i] / delta)
                self.P[i].append(0.0)
            self.Kinv.append([-a[j] / delta for j in range(m)] + [1.0 / delta])
            self.P.append([0.0] * m + [1.0])
            ka = e / delta
            self.alpha = [self.alpha[i] - a[i] * ka for i in range(m)] + [ka]
            self.d.append(x)
            k.append(self.kern(x, x))
        else:
            self.updated += 1
            Pa = []
            for i in range(m):
                acc = 0.0
                for j in range(m):
                    acc = acc + self.P[i][j] * a[j]
                Pa.append(acc)
            s = 1.0 + _dot64(a, Pa)
            q = [Pa[i] / s for i in range(m)]
            r = []
            for j in range(m):
                acc = 0.0
                for i in range(m):
                    acc = acc + a[i] * self.P[i][j]
                r.append(acc)
            for i in range(m):
                for j in range(m):
                    self.P[i][j] = self.P[i][j] - q[i] * r[j]
            for i in range(m):
                acc = 0.0
                for j in range(m):
                    acc = acc + self.Kinv[i][j] * q[j]
                self.alpha[i] = self.alpha[i] + acc * e
        return _dot64(self.alpha, k)

    def train(self, t, v, offset=0, count=None, stride=1, iterations=1, mse_tol=0.001):
        dim = len(v) if count is None else min(offset + count * stride, len(v))
        mse = 0.0
        for _ in range(iterations):
            mse, nan_count = 0.0, 0
            for i in range(offset, dim, stride):
                y = float(v[i])
                if y != y:
                    nan_count += 1
                    continue
                diff = y - self.train_one(self.position(int(t[i])), y)
                mse = mse + diff * diff
            mse = mse / max(float(dim - nan_count), 1.0)
            if mse < mse_tol:
                break
        return mse

    def f(self, t_us):
        x, acc = self.position(t_us), 0.0
        for i in range(len(self.d)):
            acc = acc + self.alpha[i] * self.kern(x, self.d[i])
        return acc


@pytest.fixture(scope="module")
def dm_exp():
    return oracle_lib.load("detmath").oracle_exp


def _host(t, v, dt, **kw):
    return region.krls_train_csr(*csr([(t, v)]), dt, host=True, **kw)


@pytest.mark.parametrize("iterations", [1, 3])
def test_host_equals_independent_statement_bitwise(dm_exp, iterations):
    t, v = noisy_sine(40, 3, holes=(0, 5, 6, 17, 39))
    model = Model(dm_exp, 3 * HOUR, **MIXED)
    mse = model.train(t, v, iterations=iterations, mse_tol=0.0)
    assert model.grown > 0 and model.updated > 0, "the series must take both branches"
    d_row, d, alpha, Kinv, P, h_mse, path = _host(t, v, 3 * HOUR, iterations=iterations, mse_tol=0.0, **MIXED)
    assert d_row.tolist() == [0, len(model.d)] and path.tolist() == [region.KRLS_PATH_HOST]
    assert same_bits(d, model.d) and same_bits(alpha, model.alpha)
    assert same_bits(Kinv[0], model.Kinv) and same_bits(P[0], model.P)
    assert same_bits(h_mse, [mse])
    assert np.abs(Kinv[0]).max() > 1e3  # an ill-conditioned case on purpose: equality is of the bits, not of a tolerance
    q_t = t[0] + (HOUR // 2) * np.arange(90, dtype=np.int64)
    got = region.krls_predict(d_row, d, alpha, 3 * HOUR, MIXED["gamma"], [0, 90], q_t, host=True)
    assert same_bits(got, [model.f(int(x)) for x in q_t])
    res = region.krls_predict(d_row, d, alpha, 3 * HOUR, MIXED["gamma"], [0, 40], t, q_v=v, host=True)
    assert same_bits(res, [float(y) - model.f(int(x)) if y == y else np.nan for x, y in zip(t, v)])


def test_grow_only_statement_bitwise(dm_exp):
    t, v = grow_series(70, 5)
    model = Model(dm_exp, HOUR, **GROW)
    mse = model.train(t, v)
    assert model.updated == 0 and len(model.d) == 70  # more than 64 entries: the strided sums wrap
    got = _host(t, v, HOUR, **GROW)
    assert same_bits(got[1], model.d) and same_bits(got[2], model.alpha) and same_bits(got[3][0], model.Kinv)
    assert same_bits(got[4][0], model.P) and same_bits(got[5], [mse])


# ---- grow-only exactness, removal ---------------------------------------------------------------------------------------
def _api_series(t, v, fx=api.POINT_INSTANT_VALUE):
    step = int(t[1] - t[0]) if len(t) > 1 else HOUR
    return api.TimeSeries(api.TimeAxis(int(t[0]) // US if len(t) else T0 // US, step // US, len(t)), v, fx)


@pytest.mark.parametrize("valid", [83, 257, 942])
def test_grow_only_every_valid_point_joins_and_is_reproduced(valid):
    t, v = grow_series(valid, valid)
    ts = _api_series(t, v)
    p = ts.get_krls_predictor(3600, **GROW)
    assert p.dictionary_size == valid == int((~np.isnan(v)).sum())
    pr = np.array(p.predict(api.TimeAxis(int(t[0]) // US, 3600, len(t))).values)
    ok = ~np.isnan(v)
    assert np.abs(pr[ok] - v[ok]).max() < 1e-10
    assert np.isfinite(pr).all()  # the gaps are filled


def test_removal_keeps_the_dictionary_at_size():
    t, v = grow_series(40, 11, nan_every=10**6)
    p = _api_series(t[1:], v[1:]).get_krls_predictor(3600, size=8, **GROW)
    assert p.dictionary_size == 8
    pr = np.array(p.predict(api.TimeAxis(int(t[1]) // US, 3600, 40)).values)
    assert np.isfinite(pr).all()
    assert same_bits(p._d, (t[-8:] / 1e6) * (1.0 / 3600.0))  # the oldest entries left: the last eight remain


# ---- other behaviour ----------------------------------------------------------------------------------------------------
def test_iterations_and_mse_tol():
    t, v = noisy_sine(120, 8)
    one = _host(t, v, 3 * HOUR, iterations=1, **MIXED)
    three = _host(t, v, 3 * HOUR, iterations=3, mse_tol=0.0, **MIXED)
    assert not same_bits(one[2], three[2])
    stopped = _host(t, v, 3 * HOUR, iterations=3, mse_tol=1e9, **MIXED)  # the first pass is below it: the loop ends
    assert same_state(one, stopped)
    none = _host(t, v, 3 * HOUR, iterations=0, **MIXED)
    assert none[0].tolist() == [0, 0] and none[5][0] == 0.0


def test_offset_count_stride_select_the_loops_points():
    t, v = noisy_sine(60, 9, holes=(7, 20))
    got = _host(t, v, 3 * HOUR, offset=3, count=5, stride=4, **MIXED)
    pick = list(range(3, min(3 + 5 * 4, 60), 4))
    assert pick == [3, 7, 11, 15, 19]
    want = _host(t[pick], v[pick], 3 * HOUR, **MIXED)
    assert same_bits(got[1], want[1]) and same_bits(got[2], want[2]) and same_bits(got[4][0], want[4][0])
    # the reference's divisor as written: dim - nan_count = 23 - 1, whatever the stride
    sq = want[5][0] * max(float(len(pick) - 1), 1.0)
    assert got[5][0] == pytest.approx(sq / 22.0, rel=1e-12)
    to_end = _host(t, v, 3 * HOUR, offset=50, **MIXED)  # the default count reaches the end at any offset
    assert same_bits(to_end[1], _host(t[50:], v[50:], 3 * HOUR, **MIXED)[1])
    beyond = _host(t, v, 3 * HOUR, offset=70, **MIXED)
    assert beyond[0].tolist() == [0, 0]


def test_training_further_equals_training_on_both():
    t, v = noisy_sine(90, 10, holes=(30, 31))
    a, b = api.KrlsRbfPredictor(3 * 3600), api.KrlsRbfPredictor(3 * 3600)
    first, second, both = _api_series(t[:50], v[:50]), _api_series(t[50:], v[50:]), _api_series(t, v)
    a.train(first)
    a.train(second)
    b.train(both)
    assert a.dictionary_size == b.dictionary_size > 1
    assert same_bits(a._d, b._d) and same_bits(a._alpha, b._alpha) and same_bits(a._Kinv, b._Kinv) and same_bits(a._P, b._P)


def test_clear_and_empty_predictors():
    t, v = noisy_sine(30, 12)
    p = api.KrlsRbfPredictor(3 * 3600)
    mse = p.train(_api_series(t, v))
    assert p.dictionary_size > 0 and mse >= 0.0
    p.clear()
    ta = api.TimeAxis(T0 // US, 3600, 5)
    assert p.dictionary_size == 0 and list(p.predict(ta).values) == [0.0] * 5
    assert p.train(_api_series(t, np.full(30, np.nan))) == 0.0 and p.dictionary_size == 0
    assert p.train(api.TimeSeries(api.TimeAxis(T0 // US, 3600, 0), [], api.POINT_INSTANT_VALUE)) == 0.0
    assert p.dictionary_size == 0 and list(p.predict(ta).values) == [0.0] * 5
    nan_ts = _api_series(t, np.full(30, np.nan))
    assert np.isnan(np.array(p.mse_ts(nan_ts, 2).values)).all() and p.predictor_mse(nan_ts) == 0.0


def test_mse_ts_window_and_predictor_mse():
    t, v = noisy_sine(25, 13, holes=(0, 1, 2, 12))
    ts = _api_series(t, v)
    p = ts.get_krls_predictor(3 * 3600)
    res = np.array(v) - np.array(p.predict(api.TimeAxis(T0 // US, 3600, 25)).values)
    got = np.array(p.mse_ts(ts, 1).values)
    assert np.isnan(got[0]) and np.isnan(got[1])  # no value within one point
    assert got[3] == (res[3] * res[3] + res[4] * res[4]) / 2
    assert got[12] == (res[11] * res[11] + res[13] * res[13]) / 2
    acc = 0.0
    for r in res[5:]:
        if r == r:
            acc = acc + r * r
    assert p.predictor_mse(ts, offset=5) == acc / (25 - 1)  # dim - nan_count, the NaN at 12


@pytest.mark.parametrize("args", [(0,), (-3600,), (3600, -1e-3), (3600, 1e-3, -0.01), (3600, 1e-3, 0.01, 0)])
def test_arguments_are_refused(args):
    with pytest.raises(RuntimeError):
        api.KrlsRbfPredictor(*args)
    t, v = noisy_sine(5, 1)
    with pytest.raises(RuntimeError):
        _api_series(t, v).krls_interpolation(*args)


def test_an_expression_is_evaluated_first():
    t, v = noisy_sine(50, 14)
    ts = _api_series(t, v)
    want = _api_series(t, np.array((ts * 2.0).values)).krls_interpolation(3 * 3600)
    assert same_bits((ts * 2.0).krls_interpolation(3 * 3600).values, want.values)


def test_ts_vector_batch_form_on_the_host():
    series = [noisy_sine(n, 20 + n) for n in (30, 45, 60)]
    tsv = api.TsVector([_api_series(t, v) for t, v in series])
    got = tsv.krls_interpolation([3 * 3600, 2 * 3600, 3600], [1e-3, 2e-3, 3e-3], 0.01, host=True)
    for k, ts in enumerate(tsv):
        want = ts.krls_interpolation((3 - k) * 3600, (k + 1) * 1e-3)
        assert same_bits(got[k].values, want.values)
    with pytest.raises(RuntimeError):
        tsv.krls_interpolation([3600, 3600], host=True)
