"""shyft_amd.api -- the reference's `shyft.api` names over the MI355X engine.

Mirrors the parts of `shyft.api` (shyft/api/__init__.py, api/boostpython/api_*.cpp,
expose.h, expose_statistics.h) that the region-model hot path uses: geo cells,
time axes and point series, region environment and interpolation parameters,
statistics, river network. The heavy objects (region models, their
interpolation, run_cells, statistics, routing) are the C++ host classes of
shyft_amd/csrc/host bound by pybind11 in `_api`; those drive the HIP engine
through the C ABI of include/shyft_hip.h. There is no CPU fallback: importing
this package requires the built extension and libshyft_hip.so.
"""
from __future__ import annotations

import numpy as np

from .._native import lib as _lib

_lib()  # one HIP runtime per process: map it (and libshyft_hip.so) before the extension module

from ._api import (  # noqa: F401  (re-exported names)
    GeoPoint, LandTypeFractions, RoutingInfo, GeoCellData, TimeAxisFixedDeltaT, point_interpretation_policy,
    POINT_INSTANT_VALUE, POINT_AVERAGE_VALUE, IDWParameter, IDWTemperatureParameter, IDWPrecipitationParameter,
    InterpolationParameter, UHGParameter, River, RiverNetwork, make_uhg_from_gamma, average_values, FlowAdjustResult,
    find_min_single_variable, BTKParameter, OKCovarianceType, OKParameter, GAUSSIAN, EXPONENTIAL,
    KalmanParameter, KalmanState, KalmanFilter, no_utctime,
)
from . import _api
from . import _tsprep
from . import _ts_expr
from ._ts_expr import time_shift  # noqa: F401  (re-exported name)
from ._tsprep import (  # noqa: F401  (re-exported names)
    RatingCurveSegment, RatingCurveFunction, RatingCurveParameters, IcePackingParameters,
    IcePackingRecessionParameters, ice_packing_temperature_policy, max_utctime,
)

from . import _tsfilter
from ._tsfilter import convolve_policy, derivative_method  # noqa: F401  (re-exported names)
from . import _krls
from ._krls import KrlsRbfPredictor  # noqa: F401  (re-exported name)

USE_FIRST, USE_ZERO, USE_NAN = convolve_policy.USE_FIRST, convolve_policy.USE_ZERO, convolve_policy.USE_NAN
DEFAULT, FORWARD, BACKWARD, CENTER = (derivative_method.DEFAULT, derivative_method.FORWARD, derivative_method.BACKWARD,
                                      derivative_method.CENTER)
DISALLOW_MISSING = ice_packing_temperature_policy.DISALLOW_MISSING
ALLOW_INITIAL_MISSING = ice_packing_temperature_policy.ALLOW_INITIAL_MISSING
ALLOW_ANY_MISSING = ice_packing_temperature_policy.ALLOW_ANY_MISSING

TimeAxis = TimeAxisFixedDeltaT
ts_point_fx = point_interpretation_policy


# ---- time (core/utctime_utilities.h; shyft's `time` is seconds) -----------------------------------------------------
def deltahours(n):
    return 3600 * n


def deltaminutes(n):
    return 60 * n


class Calendar:
    """UTC calendar (utctime_utilities.cpp:230-277); only the UTC zone is on the hot path."""

    YEAR, MONTH, DAY, HOUR = 365 * 86400, 30 * 86400, 86400, 3600

    def __init__(self, tz: str | int = 0):
        if tz not in (0, "UTC", "Etc/UTC"):
            raise RuntimeError("Calendar: only UTC is supported by the MI355X engine")

    def time(self, Y, M=1, D=1, h=0, m=0, s=0):
        return int(_api.utc_time(Y, M, D, h, m, s))

    def day_of_year(self, t):
        import datetime
        return datetime.datetime.fromtimestamp(t, datetime.timezone.utc).timetuple().tm_yday

    # calendar arithmetic (utctime_utilities.cpp:281-366) for the UTC zone, where every utc offset is 0
    QUARTER, WEEK, HOUR_3, MINUTE, SECOND = 3 * 30 * 86400, 7 * 86400, 3 * 3600, 60, 1

    @staticmethod
    def _calendar_units(t):
        """(year, month, day, seconds into the day) of t"""
        days, rest = divmod(t, 86400)
        z = int(days) + 719468
        era = z // 146097
        doe = z - era * 146097
        yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
        doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
        mp = (5 * doy + 2) // 153
        m = mp + 3 if mp < 10 else mp - 9
        return yoe + era * 400 + (m <= 2), m, doy - (153 * mp + 2) // 5 + 1, rest

    def _time_of(self, year, month, day, rest):
        return self.time(year, month, day) + rest

    def add(self, t, dt, n):
        """t plus n units of dt (calendar::add, :281-319): YEAR, QUARTER and MONTH step the calendar fields, any
        other dt is plain t + n * dt."""
        n = int(n)
        span = n * dt
        trunc = lambda a, b: int(abs(a) // b) * (1 if a >= 0 else -1)  # noqa: E731  (C++ division rounds towards zero)
        if dt == Calendar.YEAR:
            y, m, d, rest = self._calendar_units(t)
            return self._time_of(y + trunc(span, Calendar.YEAR), m, d, rest)
        if dt in (Calendar.QUARTER, Calendar.MONTH):
            if dt == Calendar.QUARTER:  # it appears as 3 x MONTH
                n = 3 * n
            y, m, d, rest = self._calendar_units(t)
            n_years = trunc(trunc(span, Calendar.MONTH), 12)
            y += n_years
            m += n - n_years * 12  # the remaining months, then repair under- or overflow
            if m < 1:
                m, y = m + 12, y - 1
            elif m > 12:
                m, y = m - 12, y + 1
            return self._time_of(y, m, d, rest)
        return t + span

    def _diff_units(self, t1, t2, dt):
        """(n, remainder) of calendar::diff_units (:321-366): the whole units of dt from t1 to t2, complementary to
        add, and what is left after them"""
        if dt == 0:
            return 0, 0
        sgn = 1
        if t1 > t2:
            sgn, t1, t2 = -1, t2, t1
        n = int((t2 - t1) // dt)  # a rough estimate for MONTH, QUARTER and YEAR
        if dt < Calendar.DAY:
            rem = t2 - self.add(t1, dt, n) if dt > Calendar.HOUR else t2 - (t1 + n * dt)
            return n * sgn, rem
        if dt == Calendar.MONTH:
            n -= n // 72  # MONTH is 30 days, a real one about 30.4375: one month too many after 72
        elif dt == Calendar.QUARTER:
            n -= n // (3 * 72)
        elif dt == Calendar.YEAR:
            n -= n // (4 * 365 * 365)
        t2x = self.add(t1, dt, n)
        if t2x > t2:  # one step too far
            n -= 1
            rem = t2 - self.add(t1, dt, n)
        elif t2x < t2:  # one step short, maybe
            t2xx = self.add(t1, dt, n + 1)
            if t2xx > t2:
                rem = t2 - t2x
            else:
                n, rem = n + 1, t2 - t2xx
        else:
            rem = 0
        return n * sgn, rem

    def diff_units(self, t1, t2, dt):
        return self._diff_units(t1, t2, dt)[0]


class UtcPeriod:
    def __init__(self, start, end):
        self.start, self.end = start, end

    def timespan(self):
        return self.end - self.start

    def contains(self, t):
        return self.start <= t < self.end

    def __repr__(self):
        return f"UtcPeriod({self.start}, {self.end})"


# ---- vectors (boost.python vector_indexing_suite stand-ins) -----------------------------------------------------------
class _Vector(list):
    def push_back(self, x):
        self.append(x)

    def size(self):
        return len(self)

    def to_numpy(self):
        return np.asarray(self)


class IntVector(_Vector):
    @staticmethod
    def from_numpy(a):
        return IntVector(int(x) for x in np.asarray(a))


class DoubleVector(_Vector):
    @staticmethod
    def from_numpy(a):
        return DoubleVector(float(x) for x in np.asarray(a))


class UtcTimeVector(_Vector):
    pass


class GeoCellDataVector(_Vector):
    pass


class _Scope(int):
    """an enum value (distinct from a time-step index when passed positionally)"""


class stat_scope:  # core/cell_model.h:183-186
    cell = cell_ix = _Scope(0)
    catchment = catchment_ix = _Scope(1)


# ---- point time series (core/time_series.h:323-414) -----------------------------------------------------------------
class TimeSeries:
    """A point series on a fixed_dt or point time axis (the apoint_ts results of the statistics)."""

    def __init__(self, ta=None, values=None, point_fx=POINT_AVERAGE_VALUE, _impl=None, fill_value=None):
        if _impl is not None:
            self._ts = _impl
            return
        if isinstance(ta, TimeSeries):  # copy constructor
            import copy
            self._ts = copy.deepcopy(ta._ts)
            return
        if values is None and fill_value is not None:
            values = float(fill_value)
        if isinstance(values, (int, float)):
            values = [float(values)] * ta.size()
        self._ts = _api._PointTs(ta, [float(v) for v in np.asarray(values, dtype=np.float64)], point_fx)
        self._ta = ta

    # An arithmetic result holds an expression tree (_expr, with its point type _fx) and no series (_impl) until it
    # is read: _ts evaluates the tree on the host on first read and keeps the result. A concrete series has no tree.
    # A partition (partition_by) is a shifted view, (_view_of, _view_shift): a source `_PointTs` seen some seconds
    # later. It has no series of its own until _ts is read; api.percentiles reads the pair instead.
    _impl = _expr = _fx = _view_of = None
    _view_shift = 0

    @property
    def _ts(self):
        if self._impl is None:
            if self._view_of is not None:
                self._ts = self._view_of._shifted(self._view_shift)
            else:
                _ts_expr.evaluate([self], host=True)
        return self._impl

    @_ts.setter
    def _ts(self, impl):
        self._impl, self._expr, self._view_of = impl, None, None

    @staticmethod
    def _shifted_view(source, shift):
        """the `_PointTs` source seen shift seconds later, not materialised"""
        ts = TimeSeries.__new__(TimeSeries)
        ts._view_of, ts._view_shift = source, shift
        return ts

    def value(self, i):
        return self._ts.value(i)

    def set(self, i, v):
        self._ts.set(i, v)
        self._expr = None  # from here on a concrete series: a later expression sees the new value

    def size(self):
        return self._ts.size()

    def __len__(self):
        return self._ts.size()

    def __call__(self, t):
        return self._ts(t)

    def time(self, i):
        return self._ts.time(i)

    def point_interpretation(self):
        if self._impl is None:  # a view and an expression answer without evaluating
            return self._view_of.point_interpretation() if self._view_of is not None else self._fx
        return self._ts.point_interpretation()

    def index_of(self, t):
        """the index of the interval that holds t, -1 outside the series (point_ts::index_of, time_series.h:343;
        time_shift_ts::index_of, time_series_dd.h:742)"""
        if self._impl is None and self._view_of is not None:
            return self._view_of.index_of(t - self._view_shift)
        return self._ts.index_of(t)

    def total_period(self):
        return UtcPeriod(*self._ts.total_period())

    @property
    def values(self):
        return DoubleVector(self._ts._values.tolist())

    @property
    def v(self):
        return self.values

    def __deepcopy__(self, memo):
        import copy
        return TimeSeries(_impl=copy.deepcopy(self._ts, memo))

    def average(self, ta):
        """true average onto a fixed_dt axis (average_accessor, time_series.h:2033-2072)."""
        return TimeSeries(ta, self._ts.average(ta), POINT_AVERAGE_VALUE)

    def integral(self, ta):
        """the integral (value x seconds) of the non-NaN parts of every interval of a fixed_dt axis (integral_ts,
        time_series_dd.h:512-538), on the host."""
        return _resampled([self], ta, _RESAMPLE_INTEGRAL, True)[0]

    def accumulate(self, ta):
        """the integral from the start of a fixed_dt axis to each of its time points: 0.0 first, NaN from the end of
        the series on (accumulate_ts, time_series_dd.h:633-679), on the host."""
        return _resampled([self], ta, _RESAMPLE_ACCUMULATE, True)[0]

    # observation preparation (api_time_series.cpp:651-653, 992-1253), one series on the host
    def rating_curve(self, rc_param):
        """the flow of a water-level series through the RatingCurveParameters (rating_curve_ts,
        time_series.h:1548-1647); the level's point type"""
        return _tsprep.rating_curve([self], rc_param, True)[0]

    def ice_packing(self, ip_params, ipt_policy):
        """the ice-packing indicator of a temperature series at its own points: 1.0 where the average over the
        threshold window lies below the threshold temperature, 0.0 where not, NaN where the policy cannot tell
        (ice_packing_ts, time_series.h:1685-1834); POINT_AVERAGE_VALUE"""
        return _tsprep.ice_packing([self], ip_params, ipt_policy, True)[0]

    def ice_packing_recession(self, ip_ts, ipr_params):
        """this flow series with the recession curve wherever the indicator ip_ts says ice-packing
        (ice_packing_recession_ts, time_series_dd.h:1220-1365); the flow's point type"""
        return _tsprep.ice_packing_recession([self], [ip_ts], ipr_params, True)[0]

    def min_max_check_linear_fill(self, v_min, v_max, dt_max=_tsprep.max_utctime):
        """values that are NaN or outside [v_min, v_max] (NaN = no limit) replaced by the line through the nearest
        valid neighbours, NaN when those are more than dt_max seconds apart (qac_ts, time_series_dd.cpp:1335-1376);
        the source's point type"""
        return _tsprep.min_max_check_linear_fill([self], v_min, v_max, dt_max, True)[0]

    # point-wise filters (api_time_series.cpp; time_series_dd.cpp:494-496, 930-948), one series on the host
    def convolve_w(self, weights, policy):
        """this series convolved with the weights: value(i) = sum_j weights[j] * value(i - j), the convolve_policy
        standing in for the values before the first point (convolve_w_ts, time_series.h:905-980); the source's point
        type"""
        return _tsfilter.convolve_w([self], weights, policy, True)[0]

    def derivative(self, method=_tsfilter.derivative_method.DEFAULT):
        """the derivative of this series: the slope between points for a POINT_INSTANT_VALUE series, the
        derivative_method's difference for a stair-case one (derivative_ts, time_series_dd.cpp:311-463);
        POINT_AVERAGE_VALUE"""
        return _tsfilter.derivative([self], method, True)[0]

    def inside(self, min_v, max_v, nan_v=float("nan"), inside_v=1.0, outside_v=0.0):
        """inside_v where min_v <= value < max_v (a NaN limit is no limit), outside_v where not, nan_v where the value
        is not finite (inside_ts, time_series_dd.h:1538-1607); the source's point type"""
        return _tsfilter.inside([self], min_v, max_v, nan_v, inside_v, outside_v, True)[0]

    def decode(self, start_bit, n_bits):
        """n_bits bits from start_bit of the values taken as unsigned integers; NaN for a value that is not finite,
        negative or above 2^52 (decode_ts, time_series_dd.h:1609-1700); the source's point type"""
        return _tsfilter.decode([self], start_bit, n_bits, True)[0]

    # KRLS interpolation (api_time_series.cpp:876-991; time_series_dd.cpp:744-753), one series on the host
    def krls_interpolation(self, dt, gamma=1e-3, tolerance=0.01, size=1000000):
        """this series smoothed and gap-filled: the predictions, at its own points, of a KrlsRbfPredictor(dt, gamma,
        tolerance, size) trained once over it (krls_interpolation_ts, time_series_dd.h:1368-1442); the source's time
        axis and point type"""
        return _krls.krls_interpolation([self], dt, gamma, tolerance, size, True)[0]

    def get_krls_predictor(self, dt, gamma=1e-3, tolerance=0.01, size=1000000):
        """a KrlsRbfPredictor(dt, gamma, tolerance, size) trained once over this series"""
        return _krls.get_krls_predictors([self], dt, gamma, tolerance, size, True)[0]

    # arithmetic (time_series_dd.cpp:94-122, 922-928): every result is a lazy expression, the other operand a
    # TimeSeries or a number. Nothing is computed until the result is read or evaluated.
    def __add__(self, o):
        return _ts_expr.binary(_ts_expr.ADD, self, o)

    def __radd__(self, o):
        return _ts_expr.binary(_ts_expr.ADD, o, self)

    def __sub__(self, o):
        return _ts_expr.binary(_ts_expr.SUB, self, o)

    def __rsub__(self, o):
        return _ts_expr.binary(_ts_expr.SUB, o, self)

    def __mul__(self, o):
        return _ts_expr.binary(_ts_expr.MUL, self, o)

    def __rmul__(self, o):
        return _ts_expr.binary(_ts_expr.MUL, o, self)

    def __truediv__(self, o):
        return _ts_expr.binary(_ts_expr.DIV, self, o)

    def __rtruediv__(self, o):
        return _ts_expr.binary(_ts_expr.DIV, o, self)

    def __neg__(self):
        return _ts_expr.binary(_ts_expr.MUL, -1.0, self)  # time_series_dd.cpp:101

    def min(self, x):
        return _ts_expr.function(_ts_expr.MIN, self, x)

    def max(self, x):
        return _ts_expr.function(_ts_expr.MAX, self, x)

    def pow(self, x):
        return _ts_expr.function(_ts_expr.POW, self, x)

    def abs(self):
        return _ts_expr.absolute(self)

    def time_shift(self, dt):
        """this series dt seconds later (time_shift_ts, time_series_dd.h:707-751)"""
        return _ts_expr.shifted(self, dt)

    def partition_by(self, calendar, t, partition_interval, n_partitions, common_t0):
        """n_partitions pieces of this series, piece i starting calendar.add(t, partition_interval, i), all moved to
        start at common_t0 (apoint_ts::partition_by, time_series_dd.cpp:653-663; core/time_series.h:2451-2494): a
        TsVector whose element i is this series shifted by common_t0 - calendar.add(t, partition_interval, i). The
        elements are shifted views of one stored series; api.percentiles takes them as they are, anything else that
        reads one makes it a concrete series first."""
        if n_partitions < 1:
            raise RuntimeError("n_partitions should be > 0")
        if partition_interval <= 0:
            raise RuntimeError("partition_interval should be > 0, typically Calendar::YEAR|MONTH|WEEK|DAY")
        if calendar._diff_units(t, common_t0, partition_interval)[1] != 0:
            raise RuntimeError("t0 must align with a complete calendar multiple dt from t")
        source = self._ts
        return TsVector(TimeSeries._shifted_view(source, common_t0 - calendar.add(t, partition_interval, i))
                        for i in range(int(n_partitions)))

    def evaluate(self, *, host=False):
        """the concrete series of this expression: one device call, or with host=True the host restatement,
        bit-identical. The result is kept, so reading this series afterwards computes nothing."""
        import copy
        return TimeSeries(_impl=copy.deepcopy(_ts_expr.evaluate([self], host)[0]))


# ---- average / integral / accumulate of a set of series in one call (region.resample) -------------------------------
_RESAMPLE_AVERAGE, _RESAMPLE_INTEGRAL, _RESAMPLE_ACCUMULATE = 0, 1, 2  # region.RESAMPLE_*


def _resampled(tsv, ta, mode, host):
    """every series of tsv onto ta by one region.resample call; the result's point type is the reference's
    (time_series_dd.h:466, :525, :646)"""
    from ..region import resample
    values = resample([ts._ts for ts in tsv], ta, mode, host=host)
    fx = POINT_INSTANT_VALUE if mode == _RESAMPLE_ACCUMULATE else POINT_AVERAGE_VALUE
    out = TsVector()
    for k in range(values.shape[1]):
        out.append(TimeSeries(_impl=_api._PointTs(ta, values[:, k], fx)))
    return out


def _resample_any(ts, ta, mode, host):
    if isinstance(ts, TimeSeries):
        return _resampled([ts], ta, mode, True)[0]
    return _resampled(ts, ta, mode, host)


def average(ts, time_axis, *, host=False):
    """api.average: the true average of a TimeSeries (on the host) or of every series of a TsVector (one device
    call) on time_axis; POINT_AVERAGE_VALUE."""
    return _resample_any(ts, time_axis, _RESAMPLE_AVERAGE, host)


def integral(ts, time_axis, *, host=False):
    """api.integral: the integral over every interval of time_axis, of a TimeSeries (on the host) or of every series
    of a TsVector (one device call); POINT_AVERAGE_VALUE."""
    return _resample_any(ts, time_axis, _RESAMPLE_INTEGRAL, host)


def accumulate(ts, time_axis, *, host=False):
    """api.accumulate: the integral from the start of time_axis to each time point, of a TimeSeries (on the host) or
    of every series of a TsVector (one device call); POINT_INSTANT_VALUE."""
    return _resample_any(ts, time_axis, _RESAMPLE_ACCUMULATE, host)


# ---- percentiles of a set of series (core/time_series_statistics.h:107-246; api_time_series.cpp) ---------------------
class statistics_property:  # time_series_statistics.h:107-111
    AVERAGE = -1
    MIN_EXTREME = -1000
    MAX_EXTREME = 1000


def _percentile_plan(tsv, time_axis, host):
    """The stored series and the views of a vector for region.ts_percentiles_csr: (row, t, v, t_end, fx, src, shift,
    t0, dt, T). A shifted view that has not been read becomes (its source, its shift) and views of one source (by
    object identity) share a row; the expressions still pending are evaluated together in one _ts_expr.evaluate call;
    a concrete series is its own row with shift 0."""
    pending = [ts for ts in tsv if ts._impl is None and ts._view_of is None]
    if pending:
        _ts_expr.evaluate(pending, host)
    t0, dt, T = _api._resample_plan([], time_axis)[5:]
    rows, row_of, src, shift, lo, hi = [], {}, [], [], [], []
    for ts in tsv:
        view = ts._impl is None
        impl = ts._view_of if view else ts._impl
        d = _api._to_us(ts._view_shift) if view else 0
        if id(impl) not in row_of:
            row_of[id(impl)] = len(rows)
            rows.append(impl)
            lo.append(t0 - d)
            hi.append(t0 + T * dt - d)
        r = row_of[id(impl)]
        src.append(r)
        shift.append(d)
        lo[r], hi[r] = min(lo[r], t0 - d), max(hi[r], t0 + T * dt - d)
    # a stored series is copied in the window its views read on this axis only (view_window, host/ts_percentiles.hpp)
    return tuple(_api._percentile_rows(rows, lo, hi)) + (src, shift, t0, dt, T)


def percentiles(ts_vector, time_axis, percentiles, *, host=True):
    """api.percentiles (calculate_percentiles, time_series_statistics.h:184-246): every series goes through its true
    average onto time_axis, non-finite samples are dropped, and each entry of `percentiles` (0..100 by R7,
    statistics_property.AVERAGE, MIN_EXTREME / MAX_EXTREME) gives one series; the extremes are the true extremes of the
    points inside each interval. The results carry the point interpretation of the first series.

    host=True, the default, computes on the host (region.ts_percentiles_csr(host=True)). Unlike the newer batched
    methods this function keeps the host as its default: it has callers and tests that run on machines without a
    GPU, and its behaviour must not change for them. host=False is one fused device call, bit-identical; a vector of
    more than region.TS_PERCENTILES_MAX_SERIES series or a list of more than region.PERCENTILES_MAX entries is
    beyond the device's limits and goes to the host as well. The partitions of partition_by are passed as views of
    their one stored series and are not materialised."""
    from ..region import ts_percentiles_csr, TS_PERCENTILES_MAX_SERIES, PERCENTILES_MAX
    tsv, pcts = list(ts_vector), [int(p) for p in percentiles]
    fx_p = tsv[0].point_interpretation() if tsv else POINT_AVERAGE_VALUE
    out = TsVector()
    if not pcts:
        return out
    *csr, src, shift, t0, dt, T = _percentile_plan(tsv, time_axis, host)
    on_host = host or len(tsv) > TS_PERCENTILES_MAX_SERIES or len(pcts) > PERCENTILES_MAX
    values = ts_percentiles_csr(*csr, src, shift, t0, dt, T, pcts, host=on_host)
    for k in range(len(pcts)):
        out.append(TimeSeries(_impl=_api._PointTs(time_axis, values[k], fx_p)))
    return out


_percentiles_of = percentiles  # the method below has a parameter of the function's name


class TsVector(_Vector):
    """api.TsVector: a vector of TimeSeries (api_time_series.cpp)."""

    def percentiles(self, time_axis, percentiles, *, host=True):
        """api.percentiles of this vector; host=True by default, as there"""
        return _percentiles_of(self, time_axis, percentiles, host=host)

    def average(self, ta, *, host=False):
        """the true average of every series on a fixed_dt axis, all in one device call (region.resample), or with
        host=True on the host, bit-identical; a TsVector of POINT_AVERAGE_VALUE series on ta."""
        return _resampled(self, ta, _RESAMPLE_AVERAGE, host)

    def integral(self, ta, *, host=False):
        """the integral of every series over every interval of a fixed_dt axis, in one device call, or with host=True
        on the host, bit-identical; a TsVector of POINT_AVERAGE_VALUE series on ta."""
        return _resampled(self, ta, _RESAMPLE_INTEGRAL, host)

    def accumulate(self, ta, *, host=False):
        """the integral of every series from the start of a fixed_dt axis to each of its time points, in one device
        call, or with host=True on the host, bit-identical; a TsVector of POINT_INSTANT_VALUE series on ta."""
        return _resampled(self, ta, _RESAMPLE_ACCUMULATE, host)

    # observation preparation: the TimeSeries methods of the same names for every series, each one device call
    # (region.ts_*_csr), or with host=True on the host, bit-identical. A parameter is one object for all series or a
    # sequence of len(self) objects.
    def rating_curve(self, rc_param, *, host=False):
        return _tsprep.rating_curve(self, rc_param, host)

    def ice_packing(self, ip_params, ipt_policy, *, host=False):
        return _tsprep.ice_packing(self, ip_params, ipt_policy, host)

    def ice_packing_recession(self, ip_ts, ipr_params, *, host=False):
        """ip_ts: a TsVector of indicators, one per flow series. Indicators made by ice_packing are first evaluated
        at the flow's time points (a device call of their own), then the recession is one device call."""
        return _tsprep.ice_packing_recession(self, ip_ts, ipr_params, host)

    def min_max_check_linear_fill(self, v_min, v_max, dt_max=_tsprep.max_utctime, *, host=False):
        return _tsprep.min_max_check_linear_fill(self, v_min, v_max, dt_max, host)

    # point-wise filters: the TimeSeries methods of the same names for every series, each one device call
    # (region.ts_*_csr), or with host=True on the host, bit-identical. derivative and inside are the reference's
    # (api_time_series.cpp:248, :340); convolve_w and decode are this engine's batched forms. A parameter is one value
    # for all series or a sequence of len(self); `weights` is one profile for all series or a sequence of profiles.
    def convolve_w(self, weights, policy, *, host=False):
        return _tsfilter.convolve_w(self, weights, policy, host)

    def derivative(self, method=_tsfilter.derivative_method.DEFAULT, *, host=False):
        return _tsfilter.derivative(self, method, host)

    def inside(self, min_v, max_v, nan_v=float("nan"), inside_v=1.0, outside_v=0.0, *, host=False):
        return _tsfilter.inside(self, min_v, max_v, nan_v, inside_v, outside_v, host)

    def decode(self, start_bit, n_bits, *, host=False):
        return _tsfilter.decode(self, start_bit, n_bits, host)

    # KRLS interpolation of every series (this project's batch forms): the whole vector is trained in one device call
    # and predicted in a second; each parameter is one value for all series or one per series
    def krls_interpolation(self, dt, gamma=1e-3, tolerance=0.01, size=1000000, *, host=False):
        return _krls.krls_interpolation(self, dt, gamma, tolerance, size, host)

    def get_krls_predictors(self, dt, gamma=1e-3, tolerance=0.01, size=1000000, *, host=False):
        """one trained KrlsRbfPredictor per series, as a list"""
        return _krls.get_krls_predictors(self, dt, gamma, tolerance, size, host)

    # forecast skill by lead time and the forecast merge (time_series_dd.cpp:1120-1165, api_time_series.cpp:299-339)
    def average_slice(self, lead_time, delta_t, n, *, host=False):
        """the true average of every series over n slices of delta_t that start lead_time after the series' own first
        point, all in one device call (region.forecast_skill_csr), or with host=True on the host, bit-identical.
        Series k of the result is POINT_AVERAGE_VALUE on TimeAxis(ts_k.time(0) + lead_time, delta_t, n); a series
        without points is passed through unchanged."""
        from ..region import forecast_skill_csr
        _check_slice_arguments(lead_time, delta_t, n)
        filled = [k for k, ts in enumerate(self) if ts.size()]
        out = TsVector(self)
        if not filled:
            return out
        csr = _api._series_csr([self[k]._ts for k in filled])
        P = len(filled)
        _, sim, _ = forecast_skill_csr(*csr, np.arange(P + 1), np.arange(P), np.full(P, -1), _api._to_us(lead_time),
                                       _api._to_us(delta_t), int(n), host=host, slices=True)
        for j, k in enumerate(filled):
            ta = TimeAxisFixedDeltaT(self[k].time(0) + lead_time, delta_t, int(n))
            out[k] = TimeSeries(_impl=_api._PointTs(ta, sim[j * int(n):(j + 1) * int(n)], POINT_AVERAGE_VALUE))
        return out

    def nash_sutcliffe(self, observation_ts, lead_time, delta_t, n, *, host=False):
        """the Nash-Sutcliffe score (1 is a perfect match) of these forecasts against observation_ts over n slices of
        delta_t that start lead_time into each forecast, in one device call, or with host=True on the host,
        bit-identical. NaN for an empty vector or an empty observation."""
        _check_slice_arguments(lead_time, delta_t, n)
        if len(self) == 0 or observation_ts.size() == 0:  # time_series_merge.h:126-127
            return float("nan")
        if int(n) == 0:  # nash_sutcliffe_goal_function, core/time_series.h:2318-2319
            raise RuntimeError("nash_sutcliffe needs equal sized ts accessors with elements >1")
        return float(forecast_skill(TsVectorSet([self]), TsVector([observation_ts]), [lead_time], delta_t, n,
                                    host=host)[0, 0])

    # arithmetic, element by element with a number, a TimeSeries or a TsVector of the same length (ats_vector,
    # time_series_dd.cpp:1007-1118); the elements of the result are lazy expressions
    def __add__(self, o):
        return _ts_expr.vector_binary(_ts_expr.ADD, self, o)

    def __radd__(self, o):
        return _ts_expr.vector_binary(_ts_expr.ADD, o, self)

    def __sub__(self, o):
        return _ts_expr.vector_binary(_ts_expr.SUB, self, o)

    def __rsub__(self, o):
        return _ts_expr.vector_binary(_ts_expr.SUB, o, self)

    def __mul__(self, o):
        return _ts_expr.vector_binary(_ts_expr.MUL, self, o)

    def __rmul__(self, o):
        return _ts_expr.vector_binary(_ts_expr.MUL, o, self)

    def __truediv__(self, o):
        return _ts_expr.vector_binary(_ts_expr.DIV, self, o)

    def __rtruediv__(self, o):
        return _ts_expr.vector_binary(_ts_expr.DIV, o, self)

    def __neg__(self):
        return TsVector(-ts for ts in self)

    def min(self, x):
        return _ts_expr.function(_ts_expr.MIN, self, x)

    def max(self, x):
        return _ts_expr.function(_ts_expr.MAX, self, x)

    def pow(self, x):
        return _ts_expr.function(_ts_expr.POW, self, x)

    def abs(self):
        return TsVector(ts.abs() for ts in self)

    def time_shift(self, dt):
        return _ts_expr.time_shift(self, dt)

    def evaluate(self, *, host=False):
        """the concrete series of every element, all expressions in one device call (region.ts_expr_csr), or with
        host=True on the host, bit-identical"""
        import copy
        return TsVector(TimeSeries(_impl=copy.deepcopy(impl)) for impl in _ts_expr.evaluate(list(self), host))

    def forecast_merge(self, lead_time, fc_interval):
        """one series from the slice [time(0) + lead_time, + fc_interval) of every forecast, a missing forecast filled
        from its neighbours (forecast_merge, core/time_series_merge.h:47-99), on the host. The forecasts are ordered by
        start time, at least fc_interval apart, and each reaches the end of its slice."""
        if lead_time < 0:  # time_series_dd.cpp:1120-1133
            raise RuntimeError("lead_time parameter should be 0 or a positive number giving number of seconds into each "
                               "forecast to start the merge slice")
        if fc_interval <= 0:
            raise RuntimeError("fc_interval parameter should be positive number giving number of seconds between first "
                               "time point in each of the supplied forecast")
        for i in range(1, len(self)):
            if self[i - 1].total_period().start + fc_interval > self[i].total_period().start:
                raise RuntimeError("The suplied forecast vector should be strictly ordered by increasing t0 by length at "
                                   f"least fc_interval: requirement broken at index:{i}")
        return TimeSeries(_impl=_api._forecast_merge([ts._ts for ts in self], lead_time, fc_interval))


def _check_slice_arguments(lead_time, delta_t, n):
    """the argument texts of ats_vector::nash_sutcliffe and average_slice (time_series_dd.cpp:1138-1143, 1148-1153)"""
    if n < 0:
        raise RuntimeError("n, number of intervals, must be specified as > 0")
    if delta_t <= 0:
        raise RuntimeError("dt, average interval, must be specified as > 0 s")
    if lead_time < 0:
        raise RuntimeError("lead_time,t0_offset,must be specified  >= 0 s")


def forecast_skill(forecast_sets, observations, lead_times, delta_t, n, *, host=False):
    """The Nash-Sutcliffe score by location and lead time, the whole table in one device call
    (region.forecast_skill_csr; an MI355X addition without a reference counterpart). forecast_sets is a TsVectorSet
    with one TsVector of forecasts per location, observations a TsVector with one observation per location. Returns an
    ndarray [len(forecast_sets)][len(lead_times)] whose cell [l][j] equals
    forecast_sets[l].nash_sutcliffe(observations[l], lead_times[j], delta_t, n), bit for bit. host=True runs the host
    restatement."""
    from ..region import forecast_skill_csr
    L, lead_times = len(forecast_sets), list(lead_times)
    if len(observations) != L:
        raise RuntimeError(f"forecast_skill: {L} forecast sets need {L} observations, got {len(observations)}")
    for lead in lead_times or [0]:
        _check_slice_arguments(lead, delta_t, n)
    scored = [len(forecast_sets[l]) > 0 and observations[l].size() > 0 for l in range(L)]
    if int(n) == 0 and lead_times and any(scored):
        raise RuntimeError("nash_sutcliffe needs equal sized ts accessors with elements >1")
    pool, fc_of, obs_of = [], [], []  # the series of all locations once; a location's rows of the table share them
    for l in range(L):
        first = len(pool)
        if scored[l]:
            pool.extend(ts._ts for ts in forecast_sets[l])
        fc_of.append(range(first, len(pool)))
        obs_of.append(len(pool) if scored[l] else -1)
        if scored[l]:
            pool.append(observations[l]._ts)
    fc_row, fc_ix, obs_ix, offsets = [0], [], [], []
    for l in range(L):
        for lead in lead_times:
            fc_ix.extend(fc_of[l])
            fc_row.append(len(fc_ix))
            obs_ix.append(obs_of[l])
            offsets.append(_api._to_us(lead))
    ns = forecast_skill_csr(*_api._series_csr(pool), fc_row, fc_ix, obs_ix, offsets, _api._to_us(delta_t), int(n),
                            host=host)
    return ns.reshape(L, len(lead_times))


def nash_sutcliffe(observation_ts, model_ts, time_axis):
    """api.nash_sutcliffe (time_series_dd.cpp:950-954): 1 - the Nash-Sutcliffe goal function over the true averages
    of the two series on time_axis, on the host; 1.0 is a perfect match."""
    return 1.0 - _api.nash_sutcliffe_goal_function(list(observation_ts.average(time_axis)._ts._values),
                                                   list(model_ts.average(time_axis)._ts._values))


def kling_gupta(observation_ts, model_ts, time_axis, s_r, s_a, s_b):
    """api.kling_gupta (time_series_dd.cpp:956-960): 1 - the Kling-Gupta goal function with the scale factors s_r
    (correlation), s_a (variability) and s_b (bias) over the true averages of the two series on time_axis, on the
    host; 1.0 is a perfect match."""
    return 1.0 - _api.kling_gupta_goal_function(list(observation_ts.average(time_axis)._ts._values),
                                                list(model_ts.average(time_axis)._ts._values), s_r, s_a, s_b)


class TsFactory:
    """api.TsFactory (api/api.h:1630-1700)."""

    def create_time_point_ts(self, period, times, values, interpretation=POINT_INSTANT_VALUE):
        return TimeSeries(_impl=_api._PointTs([float(t) for t in times], float(period.end),
                                              [float(v) for v in values], interpretation))

    def create_point_ts(self, n, tstart, dt, values, interpretation=POINT_INSTANT_VALUE):
        return TimeSeries(TimeAxisFixedDeltaT(tstart, dt, n), values, interpretation)


class TsVectorSet(_Vector):
    """api.TsVectorSet: a vector of TsVector, the forecast sets of quantile_map_forecast (api_time_series.cpp:408-417)."""

    def __init__(self, clone_me=()):
        super().__init__(TsVector(tsv) for tsv in clone_me)


# ---- quantile mapping (core/time_series_qm.h; time_series_dd.cpp:1167-1200; api_time_series.cpp:24-31, 418-443) -------
def quantile_map_forecast(forecast_sets, set_weights, historical_data, time_axis, interpolation_start,
                          interpolation_end=no_utctime, interpolated_quantiles=False, *, host=False):
    """Computes the quantile-mapped forecast from the supplied input (api.quantile_map_forecast, the reference's 5-, 6-
    and 7-argument forms).

    forecast_sets: TsVectorSet, each a TsVector of forecasts (they may differ in size and length); set_weights: one
    weight per set, every one finite and > 0 (the reference's quantile walk does not terminate otherwise, so they are
    refused here); historical_data: TsVector of scenarios that should cover time_axis; interpolation_start /
    interpolation_end: the period (seconds since epoch, no_utctime for none) over which the result goes linearly
    from the mapped forecast to the scenario, the end defaulting to the end of the forecasts; interpolated_quantiles:
    interpolate between the forecast quantiles instead of taking the one at or below. Returns a TsVector of
    POINT_AVERAGE_VALUE series on time_axis: quantile mapped up to the end of the interpolation period (or of the
    forecasts), the scenarios' own averages after it. Values that are equal at a step are ranked by series index.

    Every series is averaged onto the mapped part of the axis once; the mapping of all steps is one call of
    region.quantile_map on the device, or on the host (same arithmetic, bit-identical) with host=True or when there
    are more than region.QM_MAX_SERIES forecasts or scenarios."""
    from ..region import quantile_map, QM_MAX_SERIES
    if len(forecast_sets) < 1:  # time_series_dd.cpp:1176-1197
        raise RuntimeError("forecast_set must contain at least one forecast")
    if len(historical_data) < 2:
        raise RuntimeError("historical_data should have more than one time-series")
    if len(forecast_sets) != len(set_weights):
        raise RuntimeError(f"The size of weights ({len(set_weights)}), must match number of forecast-sets "
                           f"({len(forecast_sets)})")
    if time_axis.size() == 0:
        raise RuntimeError("time-axis should have at least one step")
    p0, p1 = time_axis.total_period()
    if interpolation_start != no_utctime:
        if not p0 <= interpolation_start < p1:
            raise RuntimeError(f"interpolation_start {interpolation_start} is not within time_axis period [{p0}, {p1})")
        if interpolation_end != no_utctime and not p0 <= interpolation_end < p1:
            raise RuntimeError(f"interpolation_end {interpolation_end} is not within time_axis period [{p0}, {p1})")
    if not all(np.isfinite(w) and w > 0 for w in set_weights):
        raise RuntimeError("quantile_map_forecast: every set weight must be finite and > 0")
    forecasts, weights = [], []  # time_series_qm.h:406-415
    for tsv, w in zip(forecast_sets, set_weights):
        forecasts.extend(_series_of(tsv))
        weights.extend([float(w)] * len(tsv))
    historical = _series_of(historical_data)
    n_qm, fc, pri, mode, interp_weight = _api._qm_plan(forecasts, historical, time_axis, float(interpolation_start),
                                                       float(interpolation_end))
    on_host = host or fc.shape[1] > QM_MAX_SERIES or pri.shape[1] > QM_MAX_SERIES
    qm = quantile_map(fc, weights, pri, mode, interp_weight, interpolated=interpolated_quantiles, host=on_host)
    if n_qm < time_axis.size():  # merge_qm_result (:363-374)
        qm = np.concatenate([qm, _api._qm_tail(historical, time_axis, n_qm).T], axis=0)
    out = TsVector()
    for k in range(len(historical)):
        out.append(TimeSeries(time_axis, qm[:, k], POINT_AVERAGE_VALUE))
    return out


# ---- geo-located sources and the region environment (api/api.h:78-168) -----------------------------------------------
class _GeoPointSource:
    def __init__(self, mid_point=None, ts=None):
        self._mid_point = mid_point if mid_point is not None else GeoPoint()
        self.ts = ts
        self.uid = ""

    def mid_point(self):
        return self._mid_point

    def _impl(self):
        g = _api._GeoPointTs(self._mid_point, self.ts._ts)
        g.uid = self.uid or ""
        return g


class GeoPointSource(_GeoPointSource):
    """api.GeoPointSource (api/api.h:78-96): a geo-located series; the typed sources derive from it."""

    @property
    def mid_point_(self):
        return self._mid_point

    @mid_point_.setter
    def mid_point_(self, p):
        self._mid_point = p


class TemperatureSource(GeoPointSource):
    pass


class PrecipitationSource(GeoPointSource):
    pass


class RadiationSource(GeoPointSource):
    pass


class WindSpeedSource(GeoPointSource):
    pass


class RelHumSource(GeoPointSource):
    pass


class _SourceVector(_Vector):
    def values_at_time(self, t):
        return DoubleVector(s.ts(t) for s in self)


class GeoPointSourceVector(_SourceVector):
    pass


class TemperatureSourceVector(_SourceVector):
    pass


class PrecipitationSourceVector(_SourceVector):
    pass


class RadiationSourceVector(_SourceVector):
    pass


class WindSpeedSourceVector(_SourceVector):
    pass


class RelHumSourceVector(_SourceVector):
    pass


class GeoPointVector(_Vector):
    pass


def bayesian_kriging_temperature(src, dst, time_axis, btk_parameter):
    """Bayesian temperature kriging of the sources onto the destination points over time_axis
    (api/boostpython/api_interpolation.cpp:54-71), computed on the MI355X (shyft_hip_btk).
    Returns a TemperatureSourceVector, one source per destination point."""
    values = _api._bayesian_kriging_temperature([s._impl() for s in (src or [])], list(dst or []), time_axis,
                                                btk_parameter)
    out = TemperatureSourceVector()
    for d, gp in enumerate(dst):
        out.append(TemperatureSource(gp, TimeSeries(time_axis, values[:, d], POINT_AVERAGE_VALUE)))
    return out


def ordinary_kriging(src, dst, time_axis, parameter):
    """Ordinary kriging of the sources onto the destination points over time_axis
    (api/boostpython/api_interpolation.cpp:86-148), computed on the MI355X (shyft_hip_ordinary_kriging).
    src is a GeoPointSourceVector or any of the typed source vectors; NaN observations are not filtered.
    Returns a GeoPointSourceVector, one source per destination point."""
    values = _api._ordinary_kriging([s._impl() for s in (src or [])], list(dst or []), time_axis, parameter)
    out = GeoPointSourceVector()
    for d, gp in enumerate(dst):
        out.append(GeoPointSource(gp, TimeSeries(time_axis, values[:, d], POINT_AVERAGE_VALUE)))
    return out


# ---- Kalman bias prediction (core/kalman.h; api/boostpython/api_kalman.cpp) -------------------------------------------
def _series_of(v):
    """the _PointTs of every item of a source vector or a TsVector"""
    return [(x.ts if hasattr(x, "ts") else x)._ts for x in v]


class KalmanBiasPredictor(_api._KalmanBiasPredictor):
    """api.KalmanBiasPredictor (api_kalman.cpp:134-204; kalman::bias_predictor, core/kalman.h:154-238): learns the
    daily bias pattern of a forecast against observations with a KalmanFilter. `.filter`, `.state`; a single
    predictor runs on the host path of the batched filter and needs no device."""

    def update_with_forecast(self, fc_set, obs_ts, time_axis):
        """feed a set of forecasts (TemperatureSourceVector or TsVector, oldest first) and the observations on the
        steps of time_axis; afterwards .state.x is the estimated bias pattern"""
        self._update_with_forecast(_series_of(fc_set), obs_ts._ts, time_axis)

    def compute_running_bias(self, fc_ts, obs_ts, time_axis):
        """the running bias series of one merged forecast against the observations: before each day, the bias
        pattern learned so far is copied out (TimeSeries on time_axis, POINT_AVERAGE_VALUE)"""
        return TimeSeries(time_axis, self._compute_running_bias(fc_ts._ts, obs_ts._ts, time_axis), POINT_AVERAGE_VALUE)

    @staticmethod
    def update_with_geo_forecast(bias_predictor, temperature_sources, observation_ts, time_axis):
        bias_predictor.update_with_forecast(temperature_sources, observation_ts, time_axis)

    @staticmethod
    def update_with_forecast_vector(bias_predictor, temperature_sources, observation_ts, time_axis):
        bias_predictor.update_with_forecast(temperature_sources, observation_ts, time_axis)

    @staticmethod
    def compute_running_bias_ts(bias_predictor, forecast_ts, observation_ts, time_axis):
        return bias_predictor.compute_running_bias(forecast_ts, observation_ts, time_axis)


class KalmanBiasPredictorVector:
    """One KalmanBiasPredictor per point, all sharing the filter, updated in one device call (no reference
    counterpart: the per-point loop of the reference's grid post-processing, shyft/tests/api/test_grid_pp.py:46-58,
    over the points of a grid). Point j is bitwise what a single KalmanBiasPredictor gives on the series of point j.
    host=True on either method runs the host restatement of the kernel."""

    def __init__(self, filter, n_points):
        self.filter = KalmanFilter(KalmanParameter(filter.parameter))
        self.n_points = int(n_points)
        if self.n_points < 0:
            raise RuntimeError("KalmanBiasPredictorVector: n_points must not be negative")
        s0 = self.filter.create_initial_state()
        n = s0.size()
        self._w = np.array(s0.W)[0, :n // 2 + 1].copy() if n else np.empty(0)
        self._W = np.array(s0.W)
        self._x = np.zeros((n, self.n_points))
        self._k = np.zeros((n, self.n_points))
        self._P = np.repeat(np.array(s0.P).reshape(n * n, 1), self.n_points, axis=1)

    def __len__(self):
        return self.n_points

    def size(self):
        return self.n_points

    @property
    def x(self):
        return self._x.T.copy()

    @property
    def k(self):
        return self._k.T.copy()

    @property
    def P(self):
        n = self._x.shape[0]
        return self._P.T.reshape(self.n_points, n, n).copy()

    def __getitem__(self, j):
        if not -self.n_points <= j < self.n_points:
            raise IndexError(j)
        s = self.filter.create_initial_state()
        s._set(self._x[:, j].tolist(), self._k[:, j].tolist(), self._P[:, j].tolist())
        return KalmanBiasPredictor(self.filter, s)

    def _check_set(self, v, what):
        if len(v) != self.n_points:
            raise RuntimeError(f"KalmanBiasPredictorVector: {what} holds {len(v)} series, the vector has "
                               f"{self.n_points} points")
        return _series_of(v)

    def _run(self, bias, tables, n_cycles, running, host):
        from ..region import kalman_run, KALMAN_PREDICTOR
        fold = np.tile(tables["fold"], n_cycles)
        self._x, self._k, P, out = kalman_run(bias, fold, self._w, tables["v2"], self._x, self._k, self._P,
                                              mode=KALMAN_PREDICTOR, running=running, host=host)
        self._P = P.reshape(self._P.shape)
        return out

    def update_with_forecast(self, fc_sets, obs_set, time_axis, host=False):
        """fc_sets: a list of forecast cycles, oldest first; each cycle and obs_set hold n_points series (source
        vectors or TsVector), and the series of one cycle share one time axis. Per point the update sequence is the
        reference's (kalman.h:173-185): cycles outer, steps of time_axis inner."""
        obs = self._check_set(obs_set, "obs_set")
        cycles = []
        for c, fc_set in enumerate(fc_sets):
            fc = self._check_set(fc_set, f"forecast cycle {c}")
            if not _api._kalman_same_axis(fc):
                raise RuntimeError(f"KalmanBiasPredictorVector: the series of forecast cycle {c} differ in time axis")
            cycles.append(fc)
        if not cycles or not self.n_points or not time_axis.size():
            return
        obs_avg = _api._kalman_average_set(obs, time_axis)  # every observation averaged once, for all cycles
        bias = np.concatenate([_api._kalman_observed_bias_set(fc, obs_avg, time_axis) for fc in cycles], axis=0)
        self._run(bias, self.filter._tables(time_axis), len(cycles), None, host)

    def compute_running_bias(self, fc_set, obs_set, time_axis, host=False):
        """the running bias of every point (kalman.h:203-236): a vector of the input's type, one series per point"""
        obs = self._check_set(obs_set, "obs_set")
        fc = self._check_set(fc_set, "fc_set")
        t = self.filter._tables(time_axis, True)
        out = np.empty((time_axis.size(), self.n_points))
        if self.n_points and time_axis.size():
            bias = _api._kalman_observed_bias_set(fc, _api._kalman_average_set(obs, time_axis), time_axis)
            out = self._run(bias, t, 1,
                            (t["save_every"], t["piece_begin"], t["piece_ix"], t["piece_seconds"]), host)
        r = type(fc_set)()
        for j, src in enumerate(fc_set):
            ts = TimeSeries(time_axis, out[:, j], POINT_AVERAGE_VALUE)
            r.append(type(src)(src.mid_point(), ts) if hasattr(src, "ts") else ts)
        return r


class ARegionEnvironment:
    def __init__(self):
        self.temperature = TemperatureSourceVector()
        self.precipitation = PrecipitationSourceVector()
        self.radiation = RadiationSourceVector()
        self.wind_speed = WindSpeedSourceVector()
        self.rel_hum = RelHumSourceVector()

    def _impl(self):
        e = _api._RegionEnvironment()
        for name in ("temperature", "precipitation", "radiation", "wind_speed", "rel_hum"):
            setattr(e, name, [s._impl() for s in (getattr(self, name) or [])])
        return e

    def copy(self):
        import copy
        return copy.deepcopy(self)


# ---- the method-stack parameter / state objects -----------------------------------------------------------------------
class _Group:
    """Attribute view of a slice of a flat parameter/state vector (pt_gs_k.h:77-112 get/set order)."""

    def __init__(self, owner, fields):
        object.__setattr__(self, "_owner", owner)
        object.__setattr__(self, "_fields", fields)

    def __getattr__(self, name):
        f = object.__getattribute__(self, "_fields")
        if name in f:
            return object.__getattribute__(self, "_owner")._v[f[name]]
        raise AttributeError(name)

    def __setattr__(self, name, value):
        f = object.__getattribute__(self, "_fields")
        if name not in f:
            raise AttributeError(name)
        object.__getattribute__(self, "_owner")._v[f[name]] = float(value)


class _FlatParameter:
    """Base of the stack parameter classes: a flat vector with the reference's named groups."""
    NAMES: tuple = ()
    DEFAULTS: tuple = ()
    ERROR = "Parameter Accessor: .set size missmatch"

    def __init__(self, *groups):
        self._v = [float(x) for x in self.DEFAULTS]
        if len(groups) == 1 and isinstance(groups[0], _FlatParameter):
            self._v = list(groups[0]._v)

    def size(self):
        return len(self.NAMES)

    def get(self, i):
        return self._v[i]

    def set(self, p):
        p = list(p)
        if len(p) != self.size():
            raise RuntimeError(self.ERROR)
        self._v[:self.size()] = [float(x) for x in p]

    def get_name(self, i):
        if not 0 <= i < self.size():
            raise RuntimeError(self.ERROR.replace(".set size missmatch", ".get_name(i) Out of range."))
        return self.NAMES[i]

    def to_vector(self):
        return list(self._v)

    def __getattr__(self, name):
        fields = {n.split(".", 1)[1]: k for k, n in enumerate(type(self).NAMES) if n.split(".", 1)[0] == name}
        if not fields:
            raise AttributeError(name)
        return _Group(self, fields)

    def __eq__(self, other):
        return isinstance(other, type(self)) and self._v == other._v

    def __deepcopy__(self, memo):
        c = type(self)()
        c._v = list(self._v)
        return c


class _SnowDistributionParameter(_FlatParameter):
    """A stack parameter with the hbv_snow / hbv_physical_snow quantile distribution (hbv_snow.h:21-72,
    hbv_physical_snow.h:43-74): snow_s (bin weights) and snow_intervals ride behind the flat vector as
    n_bins, s[MAX_BINS], intervals[MAX_BINS]."""
    SNOW_MODEL = "hbv_snow"  # named in the bin-count error
    MAX_BINS = 8

    def __init__(self, *a):
        super().__init__(*a)
        src = a[0] if a and isinstance(a[0], _SnowDistributionParameter) else None
        self.snow_s = list(src.snow_s) if src else [1.0] * 5
        self.snow_intervals = list(src.snow_intervals) if src else [0.0, 0.25, 0.5, 0.75, 1.0]

    def to_vector(self):
        nb, mb = len(self.snow_s), self.MAX_BINS
        if not 2 <= nb <= mb or len(self.snow_intervals) != nb:
            raise RuntimeError(f"{self.SNOW_MODEL}: number of snow bins must be in [2, {mb}]")
        # normalize_snow_distribution (hbv_snow.h:63-66): s /= integrate(s, intervals) over the whole range,
        # the trapezoid sum of hbv_snow_common.h:14-40 with a = intervals[0], b = intervals[-1]
        x, f = self.snow_intervals, self.snow_s
        area = 0.0
        for k in range(nb - 1):
            area += 0.5 * (f[k] + f[k + 1]) * (x[k + 1] - x[k])
        s = [v / area for v in f] + [0.0] * (mb - nb)
        i = list(self.snow_intervals) + [0.0] * (mb - nb)
        return list(self._v) + [float(nb)] + s + i


class _FlatState:
    NAMES: tuple = ()
    DEFAULTS: tuple = ()

    def __init__(self, v=None):
        self._v = [float(x) for x in (self.DEFAULTS if v is None else v)]

    def to_vector(self):
        return list(self._v)

    def __getattr__(self, name):
        fields = {n.split(".", 1)[1]: k for k, n in enumerate(type(self).NAMES) if n.split(".", 1)[0] == name}
        if not fields:
            raise AttributeError(name)
        return _Group(self, fields)

    def __eq__(self, other):
        return isinstance(other, type(self)) and np.allclose(self._v, other._v, atol=1e-6)


# ---- cell-identified state (api/api_state.h:22-146; api/boostpython/api_state.cpp) -----------------------------------
CellStateId = _api.CellStateId


def byte_vector_to_file(path, byte_vector):
    """api.byte_vector_to_file: write a serialised state blob to a file."""
    with open(path, "wb") as f:
        f.write(bytes(byte_vector))


def byte_vector_from_file(path):
    """api.byte_vector_from_file: read a blob written by byte_vector_to_file."""
    with open(path, "rb") as f:
        return f.read()


class _StateWithId:
    """cell_state_with_id<state_t> (api_state.h:62-75): id + state."""
    _state_t = None

    def __init__(self, id=None, state=None):
        self.id = id if id is not None else CellStateId()
        self.state = state if state is not None else self._state_t()

    def __eq__(self, other):  # only id equality (api_state.h:68-70)
        return isinstance(other, _StateWithId) and self.id == other.id


class _StateWithIdVector(_Vector):
    """vector<cell_state_with_id<state_t>> with the reference's serialisation helpers. The byte layout is this
    engine's own (host/state_io.hpp), tagged with the method stack; it is not a boost archive."""
    _item_t = None
    _state_vector_t = None
    _stack = 0

    def _pairs(self):
        return [(x.id, x.state.to_vector()) for x in self]

    @classmethod
    def _from_pairs(cls, pairs):
        return cls(cls._item_t(i, cls._item_t._state_t(v)) for i, v in pairs)

    def serialize_to_bytes(self):
        return _api._serialize_states(self._stack, len(self._item_t._state_t.NAMES), self._pairs())

    @classmethod
    def deserialize_from_bytes(cls, b):
        return cls._from_pairs(_api._deserialize_states(bytes(b), cls._stack, len(cls._item_t._state_t.NAMES)))

    def serialize_to_str(self):
        import base64
        return base64.b64encode(self.serialize_to_bytes()).decode("ascii")

    @classmethod
    def deserialize_from_str(cls, s):
        import base64
        return cls.deserialize_from_bytes(base64.b64decode(s))

    @property
    def state_vector(self):
        return self._state_vector_t(x.state for x in self)


def make_state_with_id_types(prefix, state_t, state_vector_t, stack_id):
    """<prefix>StateWithId, <prefix>StateWithIdVector and the module-level deserialize_from_bytes of a stack."""
    item = type(prefix + "StateWithId", (_StateWithId,), {"_state_t": state_t})
    vec = type(prefix + "StateWithIdVector", (_StateWithIdVector,),
               {"_item_t": item, "_state_vector_t": state_vector_t, "_stack": stack_id})
    return item, vec, vec.deserialize_from_bytes


class _StateIoHandler:
    """model.state: state_io_handler<cell_t> (api_state.h:99-146)."""

    def __init__(self, model):
        self._m = model

    def extract_state(self, cids):
        """the states of the cells (all, or those of the catchment ids `cids`) with their CellStateId"""
        return self._m._state_with_id_vector_t._from_pairs(self._m._extract_state(list(cids)))

    def apply_state(self, cell_id_state_vector, cids):
        """apply states by CellStateId (filtered by cids); returns the indexes of states that matched no cell"""
        return IntVector(self._m._apply_state(list(cell_id_state_vector._pairs()), list(cids)))


# ---- cell views (core/cell_model.h:47-160) ---------------------------------------------------------------------------
FORCING = ("temperature", "precipitation", "wind_speed", "rel_hum", "radiation")
SERIES_FORCING, SERIES_STATE = 100, 200


class _CellSeries:
    def __init__(self, model, series, cell):
        self._m, self._s, self._c = model, series, cell

    def value(self, i):
        return self._m._cell_value(self._s, self._c, i)

    def set(self, i, v):
        if self._s < SERIES_FORCING or self._s >= SERIES_STATE:
            raise RuntimeError("only cell env_ts series are writable")
        self._m._set_cell_value(self._s - SERIES_FORCING, self._c, i, float(v))

    def size(self):
        n = self._m._time_axis.size()
        return n + 1 if self._s >= SERIES_STATE else n

    def __len__(self):
        return self.size()

    @property
    def values(self):
        return DoubleVector(self._m._cell_series(self._s, self._c).tolist())

    def to_numpy(self):
        return self._m._cell_series(self._s, self._c)


class _Named:
    def __init__(self, model, cell, mapping):
        self._m, self._c, self._map = model, cell, mapping

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        if name not in self._map:
            raise AttributeError(name)
        return _CellSeries(self._m, self._map[name], self._c)


class CellView:
    """model.cells[i]: geo, env_ts, state, rc, sc and parameter of one cell (a view into the device data)."""

    def __init__(self, model, i):
        self._m, self._i = model, i

    @property
    def geo(self):
        return self._m._cell_geo(self._i)

    def mid_point(self):
        return self.geo.mid_point()

    @property
    def env_ts(self):
        return _Named(self._m, self._i, {n: SERIES_FORCING + k for k, n in enumerate(FORCING)})

    @property
    def rc(self):
        return _Named(self._m, self._i, {n: k for k, n in enumerate(self._m._SERIES)})

    @property
    def sc(self):
        return _Named(self._m, self._i, {n: SERIES_STATE + k for k, n in enumerate(self._m._STATE_SERIES)})

    @property
    def state(self):
        return self._m._state_t(self._m._get_states()[self._i])

    @property
    def parameter(self):
        p = self._m._parameter_t()
        p._v = list(self._m._cell_parameter(self._i))
        return p


class CellVector(_Vector):
    pass


# ---- statistics (api/api.h:179-1597, expose_statistics.h) --------------------------------------------------------------
class _Statistics:
    """name -> (series id, weighted): sums (weighted False) or area-weighted averages (True)."""

    def __init__(self, model, spec):
        self._m, self._spec = model, spec

    def _ts(self, sid, weighted, indexes, ix_type):
        v = self._m._stat_series(sid, list(indexes), int(ix_type), weighted)
        ta = self._m._time_axis
        if sid >= SERIES_STATE:
            ta = TimeAxisFixedDeltaT(ta.start, ta.delta_t, ta.size() + 1)
        return TimeSeries(ta, v, POINT_AVERAGE_VALUE)

    def _percentiles(self, sid, indexes, percentiles, ix_type):
        """<name>_percentiles: percentiles across the selected cells per step, selected on the device
        (calculate_percentiles, core/time_series_statistics.h:112-246), one series per entry of `percentiles`."""
        v = self._m._percentiles(sid, list(indexes), int(ix_type), [int(p) for p in percentiles])
        ta = self._m._time_axis
        if sid >= SERIES_STATE:
            ta = TimeAxisFixedDeltaT(ta.start, ta.delta_t, ta.size() + 1)
        return TsVector(TimeSeries(ta, row, POINT_AVERAGE_VALUE) for row in v)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        spec = self._spec
        if name.endswith("_percentiles") and name[:-12] in spec and spec[name[:-12]][0] != "pot_ratio":
            sid = spec[name[:-12]][0]
            return lambda indexes, percentiles, ix_type=stat_scope.catchment: self._percentiles(sid, indexes, percentiles,
                                                                                                 ix_type)
        if name.endswith("_value") and name[:-6] in spec:
            sid, w = spec[name[:-6]]
            if sid == "pot_ratio":
                return lambda indexes, i, ix_type=stat_scope.catchment: self._m._pot_ratio_value(list(indexes), int(ix_type), i)
            return lambda indexes, i, ix_type=stat_scope.catchment: self._m._stat_value(sid, list(indexes), int(ix_type), w, i)
        if name not in spec:
            raise AttributeError(name)
        sid, w = spec[name]

        def f(indexes, i=None, ix_type=stat_scope.catchment):
            if isinstance(i, _Scope):  # overload (indexes, ix_type) of the reference
                ix_type, i = i, None
            if sid == "pot_ratio":
                if i is None:
                    ta = self._m._time_axis
                    ta1 = TimeAxisFixedDeltaT(ta.start, ta.delta_t, ta.size() + 1)
                    return TimeSeries(ta1, self._m._pot_ratio_series(list(indexes), int(ix_type)), POINT_AVERAGE_VALUE)
                return DoubleVector(self._m._pot_ratio_raster(list(indexes), int(ix_type), int(i)))
            if i is None:
                return self._ts(sid, w, indexes, ix_type)
            return DoubleVector(self._m._stat_raster(sid, list(indexes), int(ix_type), int(i)))
        return f


class BasicStatistics(_Statistics):
    """basic_cell_statistics (api/api.h:179-398): discharge/charge sums, forcing averages, areas."""
    AREAS = ("total_area", "forest_area", "glacier_area", "lake_area", "reservoir_area", "unspecified_area",
             "snow_storage_area", "elevation")

    def __init__(self, model):
        super().__init__(model, {"discharge": (0, False), "charge": (1, False),
                                 "temperature": (SERIES_FORCING + 0, True), "precipitation": (SERIES_FORCING + 1, True),
                                 "wind_speed": (SERIES_FORCING + 2, True), "rel_hum": (SERIES_FORCING + 3, True),
                                 "radiation": (SERIES_FORCING + 4, True)})

    def __getattr__(self, name):
        if name in self.AREAS:
            k = self.AREAS.index(name)
            return lambda indexes, ix_type=stat_scope.catchment: self._m._area_stat(k, list(indexes), int(ix_type))
        return super().__getattr__(name)


# ---- the model base (expose.h:143-430, shyft/api/pt_gs_k/__init__.py) ------------------------------------------------
class _ModelMixin:
    """Python half of a region model: keeps the reference's parameter/state objects live and pushes them into the
    C++ host class before every run (the reference's cells hold shared_ptr parameters, region_model.h:640-700)."""

    def _init_python(self, region_param, catchment_parameters=None):
        self._region_parameter = self._parameter_t(region_param)
        self._catchment_parameters = {int(k): self._parameter_t(v) for k, v in (catchment_parameters or {}).items()}
        self._ip = None
        self._env = None

    def _push_parameters(self):
        self._set_region_parameter(self._region_parameter.to_vector())
        for cid, p in self._catchment_parameters.items():
            self._update_catchment_parameter(cid, p.to_vector())

    # parameters
    def get_region_parameter(self):
        return self._region_parameter

    def set_region_parameter(self, p):
        self._region_parameter._v = list(p._v)
        self._set_region_parameter(p.to_vector())

    def set_catchment_parameter(self, catchment_id, p):
        if int(catchment_id) not in self._catchment_parameters:
            self._catchment_parameters[int(catchment_id)] = self._parameter_t(p)
            self._set_catchment_parameter(int(catchment_id), p.to_vector())

    def get_catchment_parameter(self, catchment_id):
        return self._catchment_parameters.get(int(catchment_id), self._region_parameter)

    def remove_catchment_parameter(self, catchment_id):
        self._catchment_parameters.pop(int(catchment_id), None)
        super().remove_catchment_parameter(int(catchment_id))

    # interpolation
    def interpolate(self, interpolation_parameter, env, best_effort=True):
        self._ip, self._env = interpolation_parameter, env
        return self._interpolate(interpolation_parameter, env._impl(), best_effort)

    def run_interpolation(self, interpolation_parameter, time_axis, env, best_effort=True):
        self._ip, self._env = interpolation_parameter, env
        return self._run_interpolation(interpolation_parameter, time_axis, env._impl(), best_effort)

    @property
    def interpolation_parameter(self):
        return self._ip if self._ip is not None else self._ip_parameter

    @property
    def region_env(self):
        return self._env

    @property
    def time_axis(self):
        return self._time_axis

    def run_cells(self, use_ncore=0, start_step=0, n_steps=0):
        self._push_parameters()
        super().run_cells(use_ncore, start_step, n_steps)

    def adjust_state_to_target_flow(self, wanted_flow_m3s, cids, start_step=0, scale_range=3.0, scale_eps=1e-3,
                                    max_iter=300, n_steps=1):
        """Tune the discharge state of `cids` so the average flow over [start_step, start_step+n_steps) is
        wanted_flow_m3s (region_model.h:626-637); returns FlowAdjustResult(q_0, q_r, diagnostics)."""
        self._push_parameters()
        return super().adjust_state_to_target_flow(float(wanted_flow_m3s), list(cids), int(start_step),
                                                   float(scale_range), float(scale_eps), int(max_iter), int(n_steps))

    # states
    def set_states(self, states):
        self._set_states([s.to_vector() for s in states])

    def get_states(self, end_states=None):
        sv = self._state_vector_t(self._state_t(v) for v in self._get_states())
        if end_states is not None:
            end_states.clear()
            end_states.extend(sv)
            return end_states
        return sv

    @property
    def current_state(self):
        return self.get_states()

    @property
    def state(self):
        return _StateIoHandler(self)

    @property
    def initial_state(self):
        return self._state_vector_t(self._state_t(v) for v in self._initial_state)

    @initial_state.setter
    def initial_state(self, sv):
        self._initial_state = [s.to_vector() for s in sv]

    # cells
    def get_cells(self):
        return CellVector(CellView(self, i) for i in range(self.size()))

    @property
    def cells(self):
        return self.get_cells()

    # statistics
    @property
    def statistics(self):
        return BasicStatistics(self)

    # routing
    @property
    def river_network(self):
        return _RiverNetworkProxy(self)

    @river_network.setter
    def river_network(self, rn):
        self._river_network = rn

    def river_output_flow_m3s(self, rid):
        return TimeSeries(self._time_axis, self._river_output_flow_m3s(rid), POINT_AVERAGE_VALUE)

    def ensemble_river_output_flow_m3s(self, parameters, rids):
        """MI355X addition: river_output_flow_m3s of the rivers `rids` for every parameter vector of `parameters`,
        all vectors as one device ensemble (run and routing), each with the routing groups its own
        routing.velocity / alpha / beta give. Starts from the model's current state and leaves the model's state,
        parameters and responses untouched. Returns one list of TimeSeries (in `rids` order) per vector, each
        bit-identical to set_region_parameter + run_cells + river_output_flow_m3s from the same state."""
        rids = [int(r) for r in rids]
        self._ensemble_run([p.to_vector() for p in parameters], False)
        v = self._ensemble_routed(rids, 2)
        return [[TimeSeries(self._time_axis, v[m, q], POINT_AVERAGE_VALUE) for q in range(len(rids))]
                for m in range(len(parameters))]

    def river_upstream_inflow_m3s(self, rid):
        return TimeSeries(self._time_axis, self._river_upstream_inflow_m3s(rid), POINT_AVERAGE_VALUE)

    def river_local_inflow_m3s(self, rid):
        return TimeSeries(self._time_axis, self._river_local_inflow_m3s(rid), POINT_AVERAGE_VALUE)

    # catchment aggregates (region_model.h:873-905)
    def catchment_discharges(self):
        return [TimeSeries(self._time_axis, v, POINT_AVERAGE_VALUE) for v in self._catchment_sums(0)]

    def catchment_charges(self):
        return [TimeSeries(self._time_axis, v, POINT_AVERAGE_VALUE) for v in self._catchment_sums(1)]

    def catchment_percentiles(self, series, percentiles):
        """Percentiles across the cells of every catchment in one device call (no reference counterpart: the
        per-catchment form of statistics.<name>_percentiles): a list, in catchment_ids order, of TsVector with one
        series per entry of `percentiles`. series: a response series name of the stack, or its id."""
        sid = self._SERIES.index(series) if isinstance(series, str) else int(series)
        ta = self._time_axis
        if sid >= SERIES_STATE:
            ta = TimeAxisFixedDeltaT(ta.start, ta.delta_t, ta.size() + 1)
        v = self._catchment_percentiles(sid, [int(p) for p in percentiles])
        return [TsVector(TimeSeries(ta, row, POINT_AVERAGE_VALUE) for row in c) for c in v]


class _RiverNetworkProxy:
    """model.river_network: edits go to the model's C++ river network (a by-value member there)."""

    def __init__(self, model):
        self._m = model

    def __getattr__(self, name):
        rn = self._m._river_network
        attr = getattr(rn, name)
        if not callable(attr):
            return attr

        def call(*a, **k):
            rn2 = self._m._river_network
            r = getattr(rn2, name)(*a, **k)
            self._m._river_network = rn2
            return self if r is rn2 else r
        return call


# ---- calibration (model_calibration.h; expose.h:472-730) -------------------------------------------------------------
from ._calibration import (  # noqa: E402,F401
    NASH_SUTCLIFFE, KLING_GUPTA, ABS_DIFF, RMSE, DISCHARGE, SNOW_COVERED_AREA, SNOW_WATER_EQUIVALENT,
    ROUTED_DISCHARGE, CELL_CHARGE, TsTransform, TargetSpecificationPts, TargetSpecificationVector,
)
from ._api import (  # noqa: E402,F401
    nash_sutcliffe_goal_function, kling_gupta_goal_function, rmse_goal_function, abs_diff_sum_goal_function,
    abs_diff_sum_goal_function_scaled,
)


# ---- the model types of a method stack (expose.h:143-170, :447-458) --------------------------------------------------
def _make_models(prefix, base_cls, native_model, native_optimizer, docs):
    """(Model, OptModel, create_opt_model_clone, create_full_model_clone, Optimizer) of a stack: the region models
    with the all-response and the discharge collector (`<prefix>Model`, `<prefix>OptModel`, docstrings `docs`) over
    the stack's _ModelMixin subclass base_cls and its C++ host class native_model, and their optimizer type."""
    from ._calibration import make_optimizer_type
    parameter_t = base_cls._parameter_t

    def construct(self, full, args, devices, shard_flags):
        if len(args) == 1 and isinstance(args[0], native_model):  # a deep copy of another model of the stack
            other = args[0]
            native_model.__init__(self, other, full)
            self._region_parameter = parameter_t(other._region_parameter)
            self._catchment_parameters = {k: parameter_t(v) for k, v in other._catchment_parameters.items()}
            self._ip, self._env = other._ip, other._env  # the reference shares region_env (region_model.h:446-448)
            return
        geo, region_param = args[0], args[1]
        cps = args[2] if len(args) > 2 else {}
        native_model.__init__(self, list(geo), region_param.to_vector(),
                              {int(k): v.to_vector() for k, v in cps.items()}, full,
                              [int(d) for d in (devices or [])], int(shard_flags))
        self._init_python(region_param, cps)

    def model_type(name, full, doc):
        def __init__(self, *args, devices=None, shard_flags=0):
            construct(self, full, args, devices, shard_flags)
        return type(name, (base_cls, native_model),
                    {"__init__": __init__, "__doc__": doc, "__module__": base_cls.__module__})

    model = model_type(prefix + "Model", True, docs[0])
    opt_model = model_type(prefix + "OptModel", False, docs[1])

    def create_opt_model_clone(src_model):
        return opt_model(src_model)

    def create_full_model_clone(src_model):
        return model(src_model)

    # the model types know their optimizer, parameter and state types (expose.h:147-170, model_calibrator)
    optimizer = make_optimizer_type(prefix + "Optimizer", native_optimizer)
    for m in (model, opt_model):
        m.optimizer_t, m.parameter_t, m.state_t = optimizer, parameter_t, base_cls._state_t
    return model, opt_model, create_opt_model_clone, create_full_model_clone, optimizer


def __getattr__(name):
    """api.min, api.max and api.pow (time_series_dd.cpp:112-122, 1090-1118). They are served on attribute access
    (`api.max(ts, 300.0)`, `from shyft_amd.api import max`) and are not globals of this module, whose own code keeps
    the builtins of those names."""
    if name in ("min", "max", "pow"):
        return getattr(_ts_expr, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
