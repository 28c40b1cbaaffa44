"""The point-wise filter series of `shyft.api`: convolve_policy and derivative_method
(api/boostpython/api_time_series.cpp; core/time_series.h:900-904, core/time_series_dd.h:170-175) and the batch calls
behind TimeSeries / TsVector .convolve_w, .derivative, .inside and .decode. Every value is computed by
region.ts_*_csr: the device kernels of kernels/tsfilter.hip, or with host=True their host restatement
(host/ts_filter.hpp), bit-identical."""
from __future__ import annotations

import enum

import numpy as np

from ._api import POINT_AVERAGE_VALUE
from ._tsprep import _csr, _one_or_each, _results


class convolve_policy(enum.IntEnum):
    """What convolve_w uses for the values before the first point (time_series.h:895-904)."""
    USE_FIRST = 0  # ts.value(0): mass preserving
    USE_ZERO = 1   # zero: shape preserving
    USE_NAN = 2    # NaN for the first len(weights) - 1 points


class derivative_method(enum.IntEnum):
    """The difference derivative() takes on a stair-case series (time_series_dd.h:170-175)."""
    DEFAULT = 0
    FORWARD = 1
    BACKWARD = 2
    CENTER = 3


def _profiles(weights, n):
    """(w_row, w, w_of): `weights` is one profile (a sequence of numbers) for all n series, or a sequence of n
    profiles; series that share a profile object share its w_row entry"""
    weights = weights if isinstance(weights, np.ndarray) else list(weights)
    if len(weights) == 0 or np.ndim(weights[0]) == 0:
        per_series = [weights] * n
    else:
        per_series = list(weights)
        if len(per_series) != n:
            raise RuntimeError(f"convolve_w: the weights must be one profile or a sequence of {n}, one per series")
    profiles, w_of = [], []
    for p in per_series:
        k = next((i for i, q in enumerate(profiles) if q is p), len(profiles))
        if k == len(profiles):
            profiles.append(p)
        w_of.append(k)
    arrays = [np.asarray(p, dtype=np.float64).reshape(-1) for p in profiles]
    w_row = np.concatenate([[0], np.cumsum([a.shape[0] for a in arrays])]).astype(np.int64)
    w = np.concatenate(arrays) if arrays else np.empty(0)
    return w_row, w, np.asarray(w_of, np.int64)


def convolve_w(tsv, weights, policy, host):
    """convolve_w_ts (time_series.h:905-980): value(i) = sum_j weights[j] * value(i - j); the source's point type"""
    from ..region import ts_convolve_w_csr
    tsv = list(tsv)
    n = len(tsv)
    policies = [int(convolve_policy(int(p))) for p in _one_or_each("convolve_w", policy, n)]
    w_row, w, w_of = _profiles(weights, n)
    row, t, v, t_end, fx = _csr(tsv)
    values = np.empty(0)
    if n:
        values = ts_convolve_w_csr(row, t, v, t_end, fx, w_row, w, w_of, policies, host=host)
    return _results(tsv, row, values, lambda ts: ts.point_interpretation())


def derivative(tsv, method, host):
    """derivative_ts (time_series_dd.h:583-607; time_series_dd.cpp:311-463); POINT_AVERAGE_VALUE. A series built on a
    TimeAxisFixedDeltaT takes the reference's fixed-step branch, any other its variable one."""
    from ..region import ts_derivative_csr
    tsv = list(tsv)
    n = len(tsv)
    methods = [int(derivative_method(int(m))) for m in _one_or_each("derivative", method, n)]
    row, t, v, t_end, fx = _csr(tsv)
    values = np.empty(0)
    if n:
        values = ts_derivative_csr(row, t, v, t_end, fx, [ts._ts._fixed_dt_us for ts in tsv], methods, host=host)
    return _results(tsv, row, values, lambda ts: POINT_AVERAGE_VALUE)


def inside(tsv, min_v, max_v, nan_v, inside_v, outside_v, host):
    """inside_ts (time_series_dd.h:1538-1607): inside_v where min_v <= value < max_v (NaN = no limit), outside_v
    where not, nan_v where the value is not finite; the source's point type"""
    from ..region import ts_inside_csr
    tsv = list(tsv)
    n = len(tsv)
    p = [[float(x) for x in _one_or_each("inside", q, n)] for q in (min_v, max_v, nan_v, inside_v, outside_v)]
    row, t, v, t_end, fx = _csr(tsv)
    values = np.empty(0)
    if n:
        values = ts_inside_csr(row, t, v, t_end, fx, *p, host=host)
    return _results(tsv, row, values, lambda ts: ts.point_interpretation())


def decode(tsv, start_bit, n_bits, host):
    """decode_ts (time_series_dd.h:1609-1700; time_series_dd.cpp:942-948): n_bits bits from start_bit of the values
    taken as unsigned integers, NaN for values that are not finite, negative or above 2^52; the source's point type"""
    from ..region import ts_decode_csr
    tsv = list(tsv)
    n = len(tsv)
    starts = [int(x) for x in _one_or_each("decode", start_bit, n)]
    bits = [int(x) for x in _one_or_each("decode", n_bits, n)]
    for s, b in zip(starts, bits):  # apoint_ts::decode refuses when the series is made, with or without points
        if s < 0 or s > 51:
            raise RuntimeError(f"start_bit must be in range [0..51], was {s}")
        if b < 1 or s + b > 51:
            raise RuntimeError(f"n_bits must be > 0 and start_bit+n_bits <= 51: n_bits ={b}, start_bit={s}")
    row, t, v, t_end, fx = _csr(tsv)
    values = np.empty(0)
    if n:
        values = ts_decode_csr(row, t, v, t_end, fx, starts, bits, host=host)
    return _results(tsv, row, values, lambda ts: ts.point_interpretation())
