"""Observation preparation of `shyft.api`: the rating-curve and ice-packing parameter types
(api/boostpython/api_time_series.cpp:1425-1702) and the batch calls behind TimeSeries / TsVector .rating_curve,
.ice_packing, .ice_packing_recession and .min_max_check_linear_fill (:651-653, :992-1253). Times and windows are in
seconds as in the reference; the engine works in int64 microseconds. Every value is computed by region.ts_*_csr: the
device kernels of kernels/tsprep.hip, or with host=True their host restatement (host/ts_prep.hpp), bit-identical."""
from __future__ import annotations

import enum

import numpy as np

from . import _api
from ._api import POINT_AVERAGE_VALUE

_I64_MAX = 2**63 - 1
_TICK_LIMIT = _I64_MAX // 4          # the engine's supported tick range (a quarter of int64)
max_utctime = _I64_MAX // 10**6       # seconds; the reference's max_utctime is the largest int64 microsecond count


def _us(t) -> int:
    """seconds -> microseconds"""
    if isinstance(t, (int, np.integer)):
        return int(t) * 10**6
    return int(round(float(t) * 1e6))


def _span_us(dt) -> int:
    """a time span in seconds as ticks, clamped into the supported tick range"""
    if abs(float(dt)) >= _TICK_LIMIT / 1e6:
        return _TICK_LIMIT if dt > 0 else -_TICK_LIMIT
    return _us(dt)


def _ulp_equal(a: float, b: float) -> bool:
    """epsilon_difference(a, b) < 2 (core_serialization / time_series.h:1283-1285): equal, or neighbours"""
    a, b = float(a), float(b)
    return a == b or abs(a - b) <= np.spacing(max(abs(a), abs(b)))


# ---- rating curve ------------------------------------------------------------------------------------------------------
class RatingCurveSegment:
    """One rating-curve equation a*(h - b)^c, valid from the water level `lower` on (time_series.h:1255-1328)."""

    def __init__(self, lower=0.0, a=0.0, b=0.0, c=0.0):
        self._lower = float(lower)
        self.a, self.b, self.c = float(a), float(b), float(c)

    @property
    def lower(self):
        return self._lower

    def valid(self, level):
        return self._lower <= level

    def flow(self, levels, i0=0, iN=None):
        """the flow of a level, or of levels[i0:iN]; `lower` is not checked"""
        f = RatingCurveFunction()
        f._segments = [RatingCurveSegment(-np.inf, self.a, self.b, self.c)]
        if np.ndim(levels) == 0:
            return f.flow(levels)
        levels = list(levels)
        return f.flow(levels[i0:len(levels) if iN is None else min(len(levels), iN)])

    def __eq__(self, o):
        return (isinstance(o, RatingCurveSegment) and _ulp_equal(self.lower, o.lower) and _ulp_equal(self.a, o.a)
                and _ulp_equal(self.b, o.b) and _ulp_equal(self.c, o.c))

    def __ne__(self, o):
        return not self == o

    __hash__ = None

    def __str__(self):
        return f"rating_curve_segment{{ lower={self.lower:g} a={self.a:g} b={self.b:g} c={self.c:g} }}"

    __repr__ = __str__


class RatingCurveFunction:
    """Rating-curve segments kept sorted on `lower`; flow(level) uses the segment whose range holds the level
    (time_series.h:1330-1443)."""

    def __init__(self, segments=None, is_sorted=True):
        self._segments = [RatingCurveSegment(s.lower, s.a, s.b, s.c) for s in (segments or [])]
        lowers = [s.lower for s in self._segments]
        if not is_sorted:
            if len(set(lowers)) != len(lowers):  # std::sort leaves the order of equal keys unspecified
                raise RuntimeError("rating_curve_function: two segments with equal lower in an unsorted list")
            self._segments.sort(key=lambda s: s.lower)
        elif any(not a <= b for a, b in zip(lowers, lowers[1:])):
            raise RuntimeError("rating_curve_function: the segment list is not sorted on lower")

    def size(self):
        return len(self._segments)

    def __len__(self):
        return len(self._segments)

    def __iter__(self):
        return iter(list(self._segments))

    def add_segment(self, lower, a=None, b=None, c=None):
        """add_segment(lower, a, b, c) or add_segment(segment): inserted by upper_bound on lower"""
        seg = lower if isinstance(lower, RatingCurveSegment) else RatingCurveSegment(lower, a, b, c)
        seg = RatingCurveSegment(seg.lower, seg.a, seg.b, seg.c)
        k = len(self._segments)
        for i, s in enumerate(self._segments):  # upper_bound: the first segment with seg.lower < s.lower
            if seg.lower < s.lower:
                k = i
                break
        self._segments.insert(k, seg)

    def flow(self, levels):
        """the flow of one level, or a DoubleVector of the flows of a list of levels; NaN below the first segment"""
        from . import DoubleVector
        from ..region import ts_rating_curve_csr
        if not self._segments:
            raise RuntimeError("no rating-curve segments")
        scalar = np.ndim(levels) == 0
        lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
        n = lv.shape[0]
        if n == 0:
            return DoubleVector()
        pack_row, curve_t, curve_row, seg = _packs_csr([_single_curve(self)])
        r = ts_rating_curve_csr([0, n], np.arange(n), lv, [n], [0], pack_row, curve_t, curve_row, seg, host=True)
        return float(r[0]) if scalar else DoubleVector(r.tolist())

    def __str__(self):
        return "rating_curve_function{" + "".join(f" {s}," for s in self._segments) + " }"

    __repr__ = __str__


class RatingCurveParameters:
    """Rating-curve functions with the times they become valid from (time_series.h:1445-1546): a time before the
    first curve gives NaN, the last curve is valid indefinitely, a pack without curves gives NaN everywhere."""

    def __init__(self):
        self._curves = []  # (t [s], RatingCurveFunction), ascending and unique in t

    def add_curve(self, t, curve):
        """curve is valid from t [s] on; a curve already at t is kept (std::map::emplace). Returns self."""
        if not any(_us(t) == _us(t0) for t0, _ in self._curves):
            self._curves.append((t, RatingCurveFunction(list(curve), True)))
            self._curves.sort(key=lambda c: _us(c[0]))
        return self

    def __iter__(self):
        return iter(list(self._curves))

    def flow(self, t, level=None):
        """flow(t, level): the flow of a level at time t [s]; flow(ts): a DoubleVector of the flows of a level
        series, point by point"""
        from . import DoubleVector, TimeSeries
        from ..region import ts_rating_curve_csr
        if level is None and isinstance(t, TimeSeries):
            return DoubleVector(np.asarray(t.rating_curve(self)._ts._values).tolist())
        tu = _us(t)
        pack_row, curve_t, curve_row, seg = _packs_csr([self])
        return float(ts_rating_curve_csr([0, 1], [tu], [float(level)], [tu + 1], [0], pack_row, curve_t, curve_row, seg,
                                         host=True)[0])

    def __str__(self):
        return "rating_curve_parameters{" + "".join(f" {t}: [ {f} ]," for t, f in self._curves) + " }"

    __repr__ = __str__


def _single_curve(f):
    p = RatingCurveParameters()
    p._curves = [(-(_TICK_LIMIT // 10**6), f)]
    return p


def _packs_csr(packs):
    """the three-level CSR of region.ts_rating_curve_csr of a list of RatingCurveParameters"""
    pack_row, curve_t, curve_row, seg = [0], [], [0], []
    for p in packs:
        for t, f in p._curves:
            curve_t.append(_us(t))
            seg.extend((s.lower, s.a, s.b, s.c) for s in f._segments)
            curve_row.append(len(seg))
        pack_row.append(len(curve_t))
    return (np.asarray(pack_row, np.int64), np.asarray(curve_t, np.int64), np.asarray(curve_row, np.int64),
            np.asarray(seg, np.float64).reshape(-1, 4))


# ---- ice packing -------------------------------------------------------------------------------------------------------
class ice_packing_temperature_policy(enum.IntEnum):
    """How ice_packing treats missing temperatures (time_series.h:1674-1683)."""
    DISALLOW_MISSING = 0
    ALLOW_INITIAL_MISSING = 1
    ALLOW_ANY_MISSING = 2


class IcePackingParameters:
    """threshold_window [s]: the look-back window of the average temperature; threshold_temperature: ice packs
    when the average is below it (time_series.h:1653-1672)."""

    def __init__(self, threshold_window, threshold_temperature):
        self.threshold_window = threshold_window
        self.threshold_temperature = float(threshold_temperature)

    def __eq__(self, o):
        return (isinstance(o, IcePackingParameters) and _us(self.threshold_window) == _us(o.threshold_window)
                and _ulp_equal(self.threshold_temperature, o.threshold_temperature))

    def __ne__(self, o):
        return not self == o

    __hash__ = None


class IcePackingRecessionParameters:
    """alpha [1/s]: the recession factor; recession_minimum: the floor of the recession curve
    (time_series_dd.h:1186-1208)."""

    def __init__(self, alpha, recession_minimum):
        self.alpha = float(alpha)
        self.recession_minimum = float(recession_minimum)

    def __eq__(self, o):
        return (isinstance(o, IcePackingRecessionParameters) and self.alpha == o.alpha
                and _ulp_equal(self.recession_minimum, o.recession_minimum))

    def __ne__(self, o):
        return not self == o

    __hash__ = None


# ---- the batch calls ---------------------------------------------------------------------------------------------------
def _csr(tsv):
    """(row, t, v, t_end, fx) of the series of a list of TimeSeries, in microseconds"""
    return _api._resample_plan([ts._ts for ts in tsv], _api.TimeAxisFixedDeltaT(0, 1, 0))[:5]


def _per_series(what, p, n, kind):
    """one parameter object for all n series, or a sequence of n"""
    if isinstance(p, kind):
        return [p] * n
    p = list(p)
    if len(p) != n or not all(isinstance(x, kind) for x in p):
        raise RuntimeError(f"{what}: the parameters must be one {kind.__name__} or a sequence of {n}, one per series")
    return p


def _results(tsv, row, values, fx_of, extra=None):
    from . import TimeSeries, TsVector
    out = TsVector()
    for k, ts in enumerate(tsv):
        r = TimeSeries(_impl=ts._ts._with_values(values[row[k]:row[k + 1]], fx_of(ts)))
        if extra is not None:
            r._ice_packing = extra(k)
        out.append(r)
    return out


def rating_curve(tsv, rc_param, host):
    """rating_curve_ts (time_series.h:1548-1647): the level series' points through rc_param; their point type"""
    from ..region import ts_rating_curve_csr
    tsv = list(tsv)
    params = _per_series("rating_curve", rc_param, len(tsv), RatingCurveParameters)
    packs, pack_of = [], []
    for p in params:  # series that share a parameter object share its pack
        k = next((i for i, q in enumerate(packs) if q is p), len(packs))
        if k == len(packs):
            packs.append(p)
        pack_of.append(k)
    row, t, v, t_end, fx = _csr(tsv)
    values = np.empty(0)
    if len(tsv):
        values = ts_rating_curve_csr(row, t, v, t_end, fx, *_packs_csr(packs), np.asarray(pack_of, np.int64), host=host)
    return _results(tsv, row, values, lambda ts: ts.point_interpretation())


def _detect(temps, params, policies, qrow, qt, host):
    from ..region import ts_ice_packing_csr
    row, t, v, t_end, fx = _csr(temps)
    if not len(temps):
        return np.empty(0)
    return ts_ice_packing_csr(row, t, v, t_end, fx, qrow, qt, [_span_us(p.threshold_window) for p in params],
                              [p.threshold_temperature for p in params], [int(q) for q in policies], host=host)


def ice_packing(tsv, ip_params, ipt_policy, host):
    """ice_packing_ts (time_series.h:1685-1834) at the temperature series' own points; POINT_AVERAGE_VALUE. The
    results remember their temperature series, parameters and policy, so ice_packing_recession can evaluate the
    detector at the flow's time points as the reference's ice_packing_ts(t) does."""
    tsv = list(tsv)
    params = _per_series("ice_packing", ip_params, len(tsv), IcePackingParameters)
    policies = _per_series("ice_packing", ipt_policy, len(tsv), int)  # the enum is an int
    row, t, _, _, _ = _csr(tsv)
    values = _detect(tsv, params, policies, row, t, host)
    frozen = [IcePackingParameters(p.threshold_window, p.threshold_temperature) for p in params]
    return _results(tsv, row, values, lambda ts: POINT_AVERAGE_VALUE,
                    lambda k: (tsv[k], frozen[k], ice_packing_temperature_policy(int(policies[k]))))


def ice_packing_recession(flows, ip_tsv, ipr_params, host):
    """ice_packing_recession_ts (time_series_dd.h:1220-1365): the flow, replaced by the recession curve wherever the
    indicator says ice-packing; the flow's point type. An indicator made by ice_packing is evaluated at the flow's
    time points (one more batch call), any other series is sampled by its own f(t)."""
    from ..region import ts_ice_packing_recession_csr
    flows, ip_tsv = list(flows), list(ip_tsv)
    if len(ip_tsv) != len(flows):
        raise RuntimeError(f"ice_packing_recession: ip_ts holds {len(ip_tsv)} series, there are {len(flows)} flow series")
    params = _per_series("ice_packing_recession", ipr_params, len(flows), IcePackingRecessionParameters)
    row, t, v, t_end, fx = _csr(flows)
    ice = np.empty(t.shape[0])
    made = [k for k, ip in enumerate(ip_tsv) if getattr(ip, "_ice_packing", None) is not None]
    if made:
        src = [ip_tsv[k]._ice_packing for k in made]
        qrow = np.concatenate([[0], np.cumsum([row[k + 1] - row[k] for k in made])]).astype(np.int64)
        qt = np.concatenate([t[row[k]:row[k + 1]] for k in made]) if qrow[-1] else np.empty(0, np.int64)
        got = _detect([s[0] for s in src], [s[1] for s in src], [s[2] for s in src], qrow, qt, host)
        for j, k in enumerate(made):
            ice[row[k]:row[k + 1]] = got[qrow[j]:qrow[j + 1]]
    for k, ip in enumerate(ip_tsv):
        if k not in made:
            ice[row[k]:row[k + 1]] = ip._ts._sample_us(t[row[k]:row[k + 1]].tolist())
    periods = [ip._ts._total_period_us() for ip in ip_tsv]
    values = np.empty(0)
    if len(flows):
        values = ts_ice_packing_recession_csr(row, t, v, t_end, fx, ice, [p[0] for p in periods], [p[1] for p in periods],
                                              [p.alpha for p in params], [p.recession_minimum for p in params], host=host)
    return _results(flows, row, values, lambda ts: ts.point_interpretation())


def _one_or_each(what, x, n):
    if np.ndim(x) == 0:
        return [x] * n
    x = list(x)
    if len(x) != n:
        raise RuntimeError(f"{what}: the parameters must be one value or a sequence of {n}, one per series")
    return x


def min_max_check_linear_fill(tsv, v_min, v_max, dt_max, host):
    """qac_ts without a replacement series (time_series_dd.h:1487-; time_series_dd.cpp:1335-1376); the source's
    point type. dt_max [s] is clamped into the engine's tick range."""
    from ..region import ts_min_max_fill_csr
    tsv = list(tsv)
    n = len(tsv)
    lo, hi, span = _one_or_each("min_max_check_linear_fill", v_min, n), _one_or_each("min_max_check_linear_fill", v_max, n), \
        _one_or_each("min_max_check_linear_fill", dt_max, n)
    row, t, v, t_end, fx = _csr(tsv)
    values = np.empty(0)
    if n:
        values = ts_min_max_fill_csr(row, t, v, t_end, fx, [float(x) for x in lo], [float(x) for x in hi],
                                     [_span_us(x) for x in span], host=host)
    return _results(tsv, row, values, lambda ts: ts.point_interpretation())
