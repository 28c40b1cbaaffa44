"""KRLS interpolation of `shyft.api`: KrlsRbfPredictor (api/boostpython/api_time_series.cpp:1748-1892;
prediction::krls_rbf_predictor, core/predictions.h:30-343) and the calls behind TimeSeries / TsVector
.krls_interpolation and .get_krls_predictor(s) (api_time_series.cpp:876-991; krls_interpolation_ts,
core/time_series_dd.h:1368-1442). The algorithm is restated in csrc/host/krls.hpp from its published form; parity with
the last bit of dlib's krls is not pinned. Training and prediction go through region.krls_train_csr / krls_predict: the
kernels of kernels/krls.hip, or with host=True the host restatement, bit-identical. The sums of predictor_mse and
mse_ts are formed here, in the reference's order, from the residuals those give. Times and dt are in seconds as in the
reference; the engine works in int64 microseconds. to_str_blob (dlib's archive format) is not offered."""
from __future__ import annotations

import numpy as np

from . import _api
from ._api import POINT_AVERAGE_VALUE
from ._tsprep import _csr, _one_or_each, _results, _us

_ALL = -1  # count: to the end of the series (the reference's default is the largest size_t)


def _check(dt_us, gamma, tolerance, size):
    """the conditions of the predictor's constructor (dlib::krls, its kernel, and a dt that can be divided by)"""
    if not dt_us > 0:
        raise RuntimeError("krls: dt must be greater than 0")
    if not gamma >= 0.0:
        raise RuntimeError("krls: gamma must not be negative")
    if not tolerance >= 0.0:
        raise RuntimeError("krls: tolerance must not be negative")
    if not size > 0:
        raise RuntimeError("krls: the dictionary size must be greater than 0")


def _count(count):
    return _ALL if count is None or count < 0 or count >= 2**62 else int(count)


def _dim(offset, count, stride, n):
    """krls_dim of csrc/host/krls.hpp: min(offset + count * stride, n), saturating"""
    return n if count == _ALL else min(offset + count * stride, n)


class KrlsRbfPredictor:
    """A KRLS predictor with a radial-basis kernel on time scaled by dt (predictions.h:30-343)."""

    def __init__(self, dt, gamma=1e-3, tolerance=0.01, size=1000000):
        self._dt_us, self._gamma, self._tolerance, self._size = _us(dt), float(gamma), float(tolerance), int(size)
        _check(self._dt_us, self._gamma, self._tolerance, self._size)
        self._fx = POINT_AVERAGE_VALUE  # predicted_point_fx
        self.clear()

    dt = property(lambda self: self._dt_us / 10**6 if self._dt_us % 10**6 else self._dt_us // 10**6)
    gamma = property(lambda self: self._gamma)
    tolerance = property(lambda self: self._tolerance)
    size = property(lambda self: self._size)
    dictionary_size = property(lambda self: int(self._d.shape[0]))

    def clear(self):
        """forget all training (krls::clear_dictionary)"""
        self._d, self._alpha = np.empty(0), np.empty(0)
        self._Kinv, self._P = np.empty((0, 0)), np.empty((0, 0))

    def _state(self):
        return [0, self._d.shape[0]], self._d, self._alpha, [self._Kinv], [self._P]

    def _set(self, k, d_row, d, alpha, Kinv, P):
        self._d, self._alpha = d[d_row[k]:d_row[k + 1]].copy(), alpha[d_row[k]:d_row[k + 1]].copy()
        self._Kinv, self._P = Kinv[k].copy(), P[k].copy()

    def train(self, ts, offset=0, count=None, stride=1, iterations=1, mse_tol=0.001):
        """train on the points offset, offset + stride, ... of ts that are not NaN, at most `iterations` times or until
        the mean squared error falls below mse_tol; returns that error (predictions.h:139-181). On the host."""
        return _train([self], [ts], offset, count, stride, iterations, mse_tol, True)[0]

    def predict(self, ta):
        """the predictions at the points of the time axis ta as a TimeSeries (predictions.h:193-226). On the host."""
        from . import TimeSeries
        axis = TimeSeries(ta, 0.0, self._fx)
        return _predict([self], [axis], None, True, lambda ts: self._fx)[0]

    def predictor_mse(self, ts, offset=0, count=None, stride=1):
        """the mean squared residual over ts (predictions.h:253-282). As there, the loop visits every point from offset
        on and the stride only enters the end min(offset + count * stride, len(ts)). On the host."""
        offset, count, stride = int(offset), _count(count), int(stride)
        if offset < 0 or stride < 1:
            raise RuntimeError("krls: offset must not be negative and stride must be greater than 0")
        r = np.asarray(_predict([self], [ts], True, True, None)[0], dtype=np.float64)
        dim = _dim(offset, count, stride, r.shape[0])
        r = r[offset:dim]
        nan_count = int(np.isnan(r).sum())  # a residual is NaN where the value is (an inf value gives inf or NaN as there)
        sq = r[~np.isnan(r)]
        sq = sq * sq
        mse = float(np.add.accumulate(sq)[-1]) if sq.shape[0] else 0.0  # one accumulator, in point order
        return mse / max(float(dim - nan_count), 1.0)

    def mse_ts(self, ts, points=0):
        """the mean squared residual of the points i - points .. i + points at every point i of ts, NaN where none of
        them has a value; the time axis and point type of ts (predictions.h:300-334). On the host."""
        from . import TimeSeries
        points = int(points)
        if points < 0:
            raise RuntimeError("krls: points must not be negative")
        r = np.asarray(_predict([self], [ts], True, True, None)[0], dtype=np.float64)
        n = r.shape[0]
        ok = ~np.isnan(r)
        sq = r * r
        out = np.full(n, np.nan)
        for i in range(n):
            lo, hi = max(0, i - points), min(n, i + points + 1)
            w = sq[lo:hi][ok[lo:hi]]
            if w.shape[0]:
                out[i] = float(np.add.accumulate(w)[-1]) / w.shape[0]
        return TimeSeries(_impl=ts._ts._with_values(out.tolist(), ts.point_interpretation()))


def _train(predictors, tsv, offset, count, stride, iterations, mse_tol, host):
    """train predictor k on series k, all in one region.krls_train_csr call; the list of the mse values"""
    from ..region import krls_train_csr
    n = len(predictors)
    if n == 0:
        return []
    what = "krls train"
    offset = [int(x) for x in _one_or_each(what, offset, n)]
    count = [_count(x) for x in _one_or_each(what, count, n)]
    stride = [int(x) for x in _one_or_each(what, stride, n)]
    iterations = [int(x) for x in _one_or_each(what, iterations, n)]
    mse_tol = [float(x) for x in _one_or_each(what, mse_tol, n)]
    row, t, v, t_end, fx = _csr(tsv)
    m = [p._d.shape[0] for p in predictors]
    state = None
    if any(m):
        state = (np.concatenate([[0], np.cumsum(m)]), np.concatenate([p._d for p in predictors]),
                 np.concatenate([p._alpha for p in predictors]), [p._Kinv for p in predictors],
                 [p._P for p in predictors])
    d_row, d, alpha, Kinv, P, mse, path = krls_train_csr(
        row, t, v, t_end, fx, [p._dt_us for p in predictors], [p._gamma for p in predictors],
        [p._tolerance for p in predictors], [p._size for p in predictors], offset, count, stride, iterations, mse_tol,
        state=state, host=host)
    for k, p in enumerate(predictors):
        p._set(k, d_row, d, alpha, Kinv, P)
    return [float(x) for x in mse]


def _predict(predictors, tsv, residuals, host, fx_of):
    """predictor k at the points of series k, all in one region.krls_predict call: a TsVector of the predictions, or
    with residuals the list of the arrays value - prediction"""
    from ..region import krls_predict
    from . import TsVector
    n = len(predictors)
    if n == 0:
        return [] if residuals else TsVector()
    row, t, v, t_end, fx = _csr(tsv)
    m = [p._d.shape[0] for p in predictors]
    d_row = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    values = krls_predict(d_row, np.concatenate([p._d for p in predictors]), np.concatenate([p._alpha for p in predictors]),
                          [p._dt_us for p in predictors], [p._gamma for p in predictors], row, t,
                          q_v=v if residuals else None, host=host)
    if residuals:
        return [values[row[k]:row[k + 1]] for k in range(n)]
    return _results(tsv, row, values, fx_of)


def _predictors(what, n, dt, gamma, tolerance, size):
    return [KrlsRbfPredictor(a, b, c, d) for a, b, c, d in zip(*(_one_or_each(what, x, n) for x in (dt, gamma, tolerance, size)))]


def get_krls_predictors(tsv, dt, gamma, tolerance, size, host):
    """apoint_ts::get_krls_predictor (time_series_dd.cpp:747-753) for every series: new predictors, each trained once
    over its series with train's defaults"""
    tsv = list(tsv)
    predictors = _predictors("get_krls_predictor", len(tsv), dt, gamma, tolerance, size)
    _train(predictors, tsv, 0, None, 1, 1, 0.001, host)
    return predictors


def krls_interpolation(tsv, dt, gamma, tolerance, size, host):
    """krls_interpolation_ts::values (time_series_dd.h:1368-1442): every series replaced by the predictions, at its own
    points, of a predictor trained once over it; the source's time axis and point type"""
    tsv = list(tsv)
    predictors = get_krls_predictors(tsv, dt, gamma, tolerance, size, host)
    return _predict(predictors, tsv, None, host, lambda ts: ts.point_interpretation())
