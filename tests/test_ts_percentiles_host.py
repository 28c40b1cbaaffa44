"""Percentiles of a vector of series on the host entry (shyft_hip_ts_percentiles_host, host=True) against the
independent restatement of tests/ts_percentiles_cases.py, views against materialised shifts, the extremes' edge
cases, the refusals, Calendar.add / diff_units, TimeSeries.partition_by and api.percentiles over partitions. No device.

Everywhere two values agree when their bits are equal, both are NaN or both are zero (cases.same); no tolerance."""
import itertools
import math

import numpy as np
import pytest

from tests import ts_percentiles_cases as cases

S_LIST = (1, 2, 5, 64, 65, 300)
T_LIST = (1, 2, 5, 65)
NaN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def api():
    from shyft_amd import api
    return api


@pytest.fixture(scope="module")
def region():
    from shyft_amd import region
    return region


def check_all_lists(region, batch, src, shift, ta_t0, ta_dt, T):
    for pcts in cases.PCT_LISTS:
        got = region.ts_percentiles_csr(*batch, src, shift, ta_t0, ta_dt, T, pcts, host=True)
        want = cases.reference_percentiles(region, batch, src, shift, ta_t0, ta_dt, T, pcts)
        assert got.shape == (len(pcts), T)
        assert cases.same(got, want), (pcts, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want)))))


AXIS_EPOCH = list(itertools.product(cases.AXES, range(3)))


@pytest.mark.parametrize("n", range(len(AXIS_EPOCH)))
def test_host_equals_the_restatement_on_every_axis_kind_and_epoch(region, n):
    """every axis kind x epoch, S and T rotating, every percentile list"""
    kind, epoch = AXIS_EPOCH[n]
    S, T = S_LIST[n % len(S_LIST)], T_LIST[n % len(T_LIST)]
    batch = cases.batch_for(kind, S, epoch, 100 + n)
    t0, dt = cases.EPOCHS[epoch]
    check_all_lists(region, batch, *cases.identity_views(batch), *cases.axis(kind, t0, dt, T), T)


@pytest.mark.parametrize("S,T", list(itertools.product(S_LIST, T_LIST)))
def test_host_equals_the_restatement_for_every_size(region, S, T):
    """every S x T, the axis kind and the epoch rotating, every percentile list"""
    n = S_LIST.index(S) * len(T_LIST) + T_LIST.index(T)
    kind, epoch = cases.AXES[n % len(cases.AXES)], n % 3
    batch = cases.batch_for(kind, S, epoch, 200 + n)
    t0, dt = cases.EPOCHS[epoch]
    check_all_lists(region, batch, *cases.identity_views(batch), *cases.axis(kind, t0, dt, T), T)


def test_the_batches_hold_the_lengths_hazards_and_point_types():
    row, t, v, t_end, fx = cases.batch_for("own", 300, 0, 1)
    assert set(np.diff(row).tolist()) == set(cases.LENGTHS)
    assert np.isnan(v).any() and np.isinf(v).any() and set(fx.tolist()) == {0, 1}
    assert len(cases.PCT_LISTS[-1]) == 40


def test_views_equal_materialised_shifts(region):
    """R = 3 rows, 17 views with positive, negative and zero shifts, two of them identical; against the same call
    with every view its own row"""
    t0, dt = cases.EPOCHS[0]
    for seed, lengths in ((5, (65, 1000, 64)), (6, (2, 3, 63))):
        batch = cases.make_batch(3, t0, dt, seed, lengths=lengths)
        assert set(batch[4].tolist()) == {0, 1}  # stair-case and linear rows
        src = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 0], dtype=np.int32)
        shift = np.array([0, dt, -dt, 3 * dt + 7, -5 * dt - 1, dt // 2, 24 * dt, -24 * dt, 1, -1, 0, 0, 17 * dt, 2 * dt,
                          -2 * dt + 3, 3 * dt + 7, 3 * dt + 7], dtype=np.int64)
        assert len(src) == 17 and (shift > 0).any() and (shift < 0).any() and (shift == 0).any()
        m = cases.materialise(batch, src, shift)
        for kind, T in (("own", 65), ("x24", 5), ("shifted", 65), ("half", 65)):
            ta = cases.axis(kind, t0, dt, T)
            for pcts in cases.PCT_LISTS[1:]:
                a = region.ts_percentiles_csr(*batch, src, shift, *ta, T, pcts, host=True)
                b = region.ts_percentiles_csr(*m, *cases.identity_views(m), *ta, T, pcts, host=True)
                assert cases.same(a, b), (kind, pcts)
                assert cases.same(a, cases.reference_percentiles(region, batch, src, shift, *ta, T, pcts))


def one(region, t, v, t_end, fx, ta_t0, ta_dt, T, pcts, shift=0):
    return region.ts_percentiles_csr([0, len(t)], t, v, [t_end], [fx], [0], [shift], ta_t0, ta_dt, T, pcts, host=True)


def test_extremes_are_of_the_points_not_of_the_averages(region):
    # a stair-case series with no point inside interval 1: its average there is finite, its extremes NaN
    r = one(region, [0, 25], [1.0, 3.0], 40, 1, 0, 10, 4, [50, -1000, 1000])
    assert r[0].tolist() == [1.0, 1.0, 2.0, 3.0]
    assert np.array_equal(r[1], [1.0, NaN, 3.0, NaN], equal_nan=True)
    assert np.array_equal(r[2], [1.0, NaN, 3.0, NaN], equal_nan=True)
    # an axis that starts before the first point, and exactly on it
    r = one(region, [20, 30, 35], [5.0, -7.0, 9.0], 40, 1, 0, 10, 4, [-1000, 1000])
    assert np.array_equal(r, [[NaN, NaN, 5.0, -7.0], [NaN, NaN, 5.0, 9.0]], equal_nan=True)
    r = one(region, [20, 30, 35], [5.0, -7.0, 9.0], 40, 1, 20, 10, 2, [-1000, 1000])
    assert r.tolist() == [[5.0, -7.0], [5.0, 9.0]]
    # an axis that starts between two points: the point left of it is not folded
    r = one(region, [20, 30, 35], [5.0, -7.0, 9.0], 40, 1, 25, 10, 2, [-1000, 1000])
    assert np.array_equal(r, [[-7.0, 9.0], [-7.0, 9.0]], equal_nan=True)
    # an axis that starts at t_end, and after it
    for ta_t0 in (40, 50):
        r = one(region, [20, 30, 35], [5.0, -7.0, 9.0], 40, 1, ta_t0, 10, 3, [-1000, 1000, 50])
        assert np.isnan(r).all()
    # the same through a view: the series moved 100 later starts where the axis does
    r = one(region, [20, 30, 35], [5.0, -7.0, 9.0], 40, 1, 120, 10, 2, [-1000, 1000], shift=100)
    assert r.tolist() == [[5.0, -7.0], [5.0, 9.0]]
    # an interval whose only points are non-finite; MIN and MAX of nothing but NaN
    r = one(region, [0, 5, 10, 15], [NaN, INF, 2.0, -INF], 20, 1, 0, 10, 2, [-1000, 1000])
    assert np.array_equal(r, [[NaN, 2.0], [NaN, 2.0]], equal_nan=True)
    r = one(region, [0, 5, 10, 15], [NaN] * 4, 20, 1, 0, 10, 2, [-1000, 1000, -1])
    assert np.isnan(r).all()
    # across views the fold takes every view's points
    r = region.ts_percentiles_csr([0, 2, 4], [0, 10, 0, 10], [1.0, 2.0, -4.0, 8.0], [20, 20], [1, 1], [0, 1, 1], [0, 0, 10],
                                  0, 10, 3, [-1000, 1000], host=True)
    assert np.array_equal(r, [[-4.0, -4.0, 8.0], [1.0, 8.0, 8.0]], equal_nan=True)


def test_intervals_without_a_finite_sample_are_nan_for_every_entry(region):
    pcts = cases.PCT_LISTS[-1]
    batch = ([0, 3, 6], [0, 10, 20, 0, 10, 20], [NaN, 1.0, INF, -INF, 3.0, NaN], [30, 30], [1, 1])
    r = region.ts_percentiles_csr(*batch, [0, 1], [0, 0], 0, 10, 3, pcts, host=True)
    assert np.isnan(r[:, 0]).all() and np.isnan(r[:, 2]).all()   # NaN and -inf, then +inf and NaN: nothing finite
    want = {0: 1.0, 50: 2.0, 100: 3.0, -1: 2.0, -1000: 1.0, 1000: 3.0, 555: NaN}
    for k, p in enumerate(pcts):
        if p in want:
            assert r[k, 1] == want[p] or (math.isnan(want[p]) and math.isnan(r[k, 1])), p
        else:
            assert 1.0 < r[k, 1] < 3.0, p
    batch = tuple(np.asarray(x) for x in batch)
    assert cases.same(r, cases.reference_percentiles(region, batch, [0, 1], [0, 0], 0, 10, 3, pcts))


def test_a_single_finite_sample_is_every_percentile_and_the_average(region):
    pcts = list(range(101)) + [-1]
    batch = ([0, 2, 4], [0, 10, 0, 10], [0.1, 7.25, NaN, NaN], [20, 20], [1, 1])
    r = region.ts_percentiles_csr(*batch, [0, 1], [0, 0], 0, 10, 2, pcts, host=True)
    sample = region.resample_csr(*batch, 0, 10, 2, 0, host=True)[:, 0]   # the average of the one finite series
    assert np.isfinite(sample).all() and abs(sample[0] - 0.1) < 1e-12 and abs(sample[1] - 7.25) < 1e-12
    assert (r[:, 0] == sample[0]).all() and (r[:, 1] == sample[1]).all()


def test_refusals(region):
    from shyft_amd._native import ShyftHipError
    ok = ([0, 2], [0, 10], [1.0, 2.0], [20], [1])
    with pytest.raises(ShyftHipError, match=r"view 1 has src 1 outside the 1 series"):
        region.ts_percentiles_csr(*ok, [0, 1], [0, 0], 0, 10, 2, [50], host=True)
    with pytest.raises(ShyftHipError, match=r"view 0 has src -1"):
        region.ts_percentiles_csr(*ok, [-1], [0], 0, 10, 2, [50], host=True)
    with pytest.raises(ShyftHipError, match=r"time_axis::point_dt\(\) needs time-points in increasing order"):
        region.ts_percentiles_csr([0, 3], [0, 20, 10], [1.0, 2.0, 3.0], [30], [0], [0], [0], 0, 10, 4, [50], host=True)
    with pytest.raises(ShyftHipError, match=r"time_axis::point_dt\(\) illegal end-of-axis"):
        region.ts_percentiles_csr([0, 2], [0, 10], [1.0, 2.0], [10], [0], [0], [0], 0, 10, 4, [50], host=True)
    for dt in (0, -10):
        with pytest.raises(ShyftHipError, match="delta-t larger than 0"):
            region.ts_percentiles_csr(*ok, [0], [0], 0, dt, 4, [50], host=True)
    # a one-point series: on a period start as stored, strictly inside a period once it is moved
    one_point = ([0, 1], [10], [1.0], [20], [1])
    r = region.ts_percentiles_csr(*one_point, [0], [0], 0, 10, 4, [50], host=True)
    assert np.array_equal(r[0], [NaN, 1.0, NaN, NaN], equal_nan=True)
    with pytest.raises(ShyftHipError, match="one-point series"):
        region.ts_percentiles_csr(*one_point, [0], [5], 0, 10, 4, [50], host=True)
    r = region.ts_percentiles_csr([0, 1], [5], [1.0], [15], [1], [0], [5], 0, 10, 4, [50], host=True)
    assert np.array_equal(r[0], [NaN, 1.0, NaN, NaN], equal_nan=True)
    with pytest.raises(ValueError):
        region.ts_percentiles_csr(*ok, [0, 0], [0], 0, 10, 2, [50], host=True)


def test_empty_calls(region):
    ok = ([0, 2], [0, 10], [1.0, 2.0], [20], [1])
    assert np.isnan(region.ts_percentiles_csr(*ok, [], [], 0, 10, 3, [50, -1], host=True)).all()
    assert region.ts_percentiles_csr(*ok, [0], [0], 0, 10, 0, [50], host=True).shape == (1, 0)
    assert region.ts_percentiles_csr(*ok, [0], [0], 0, 10, 3, [], host=True).shape == (0, 3)


def test_region_ts_percentiles_takes_point_series(api, region):
    ta = api.TimeAxis(0, 3600, 48)
    tsv = [api.TimeSeries(ta, np.arange(48.0) * k, api.POINT_AVERAGE_VALUE)._ts for k in range(5)]
    day = api.TimeAxis(0, 86400, 2)
    r = region.ts_percentiles(tsv, day, [0, 50, 100, -1000], host=True)
    assert r.tolist() == [[0.0, 0.0], [23.0, 71.0], [46.0, 142.0], [0.0, 0.0]]


# ---- Calendar.add / diff_units (utctime_utilities.cpp:281-366) ---------------------------------------------------------
def test_calendar_add(api):
    c, C = api.Calendar(), api.Calendar
    assert (C.QUARTER, C.WEEK, C.HOUR_3, C.MINUTE, C.SECOND) == (90 * 86400, 7 * 86400, 10800, 60, 1)
    assert (C.YEAR, C.MONTH, C.DAY, C.HOUR) == (365 * 86400, 30 * 86400, 86400, 3600)
    # YEAR across leap years
    assert c.add(c.time(2015, 9, 1), C.YEAR, 1) == c.time(2016, 9, 1)
    assert c.add(c.time(2015, 9, 1), C.YEAR, 1) - c.time(2015, 9, 1) == 366 * 86400
    assert c.add(c.time(2016, 9, 1, 7, 30, 15), C.YEAR, 4) == c.time(2020, 9, 1, 7, 30, 15)
    assert c.add(c.time(1930, 9, 1), C.YEAR, 86) == c.time(2016, 9, 1)
    assert c.add(c.time(2016, 3, 1), C.YEAR, -1) == c.time(2015, 3, 1)
    assert c.add(c.time(1968, 1, 1), C.YEAR, -3) == c.time(1965, 1, 1)  # before 1970
    # MONTH with overflow and underflow
    assert c.add(c.time(2016, 11, 15), C.MONTH, 3) == c.time(2017, 2, 15)
    assert c.add(c.time(2016, 2, 15), C.MONTH, -3) == c.time(2015, 11, 15)
    assert c.add(c.time(2016, 1, 1), C.MONTH, 12) == c.time(2017, 1, 1)
    assert c.add(c.time(2016, 1, 1), C.MONTH, 26) == c.time(2018, 3, 1)
    assert c.add(c.time(2016, 1, 1), C.MONTH, -26) == c.time(2013, 11, 1)
    assert c.add(c.time(2016, 6, 1, 12), C.MONTH, 0) == c.time(2016, 6, 1, 12)
    # QUARTER is three months
    assert c.add(c.time(2016, 1, 1), C.QUARTER, 1) == c.time(2016, 4, 1)
    assert c.add(c.time(2016, 11, 1), C.QUARTER, 1) == c.time(2017, 2, 1)
    assert c.add(c.time(2016, 1, 1), C.QUARTER, -5) == c.time(2014, 10, 1)
    assert c.add(c.time(2016, 1, 1), C.QUARTER, 8) == c.time(2018, 1, 1)
    # the plain units
    t = c.time(2016, 2, 28, 23)
    assert c.add(t, C.DAY, 2) == c.time(2016, 3, 1, 23)
    assert c.add(t, C.HOUR, 2) == c.time(2016, 2, 29, 1)
    assert c.add(t, C.WEEK, -1) == c.time(2016, 2, 21, 23)
    assert c.add(t, C.HOUR_3, 3) == t + 9 * 3600 and c.add(t, C.MINUTE, -5) == t - 300 and c.add(t, C.SECOND, 7) == t + 7


def test_calendar_diff_units_is_complementary_to_add(api):
    c, C = api.Calendar(), api.Calendar
    t0 = c.time(1930, 9, 1)
    assert c.diff_units(t0, c.time(2016, 9, 1), C.YEAR) == 86
    assert c.diff_units(c.time(2016, 9, 1), t0, C.YEAR) == -86
    assert c.diff_units(t0, c.time(2016, 9, 1), api.deltahours(1)) == (c.time(2016, 9, 1) - t0) // 3600
    for dt in (C.YEAR, C.QUARTER, C.MONTH, C.WEEK, C.DAY, C.HOUR_3, C.HOUR, C.MINUTE):
        # the reference's estimate for QUARTER is corrected by one step only, which reaches 40 quarters and not 100
        for n in (0, 1, 5, 13, 40) if dt == C.QUARTER else (0, 1, 5, 13, 100, 1000):
            t1 = c.add(t0, dt, n)
            assert c._diff_units(t0, t1, dt) == (n, 0), (dt, n)
            assert c._diff_units(t1, t0, dt)[0] == -n
            assert c._diff_units(t0, t1 + 1, dt) == (n, 1)            # a remainder after n whole units
            if n:
                assert c._diff_units(t0, t1 - 1, dt)[0] == n - 1      # one short of n
    # the rough estimate (t2 - t1) / dt is one too large, or one too small, and is corrected
    t1 = c.time(2016, 1, 1)
    assert (c.time(2016, 12, 31) - t1) // C.YEAR == 1                 # 365 days of a leap year: not a whole year yet
    assert c._diff_units(t1, c.time(2016, 12, 31), C.YEAR) == (0, 365 * 86400)
    assert (c.time(2016, 3, 1) - c.time(2016, 2, 1)) // C.MONTH == 0  # February: 29 days, still one whole month
    assert c._diff_units(c.time(2016, 2, 1), c.time(2016, 3, 1), C.MONTH) == (1, 0)
    assert (c.time(2020, 1, 1) - c.time(2010, 1, 1)) // C.MONTH == 121
    assert c._diff_units(c.time(2010, 1, 1), c.time(2020, 1, 1), C.MONTH) == (120, 0)
    assert c._diff_units(c.time(2016, 1, 1), c.time(2016, 1, 1, 5), C.HOUR_3) == (1, 2 * 3600)
    assert c.diff_units(t1, t1 + 3, 0) == 0


# ---- TimeSeries.partition_by and api.percentiles over partitions -------------------------------------------------------
@pytest.fixture(scope="module")
def partitions(api):
    """shyft/tests/api/test_time_series.py:485-523 shrunk: 6 years hourly, 5 yearly partitions from 1 September"""
    c = api.Calendar()
    t0 = c.time(2010, 9, 1)
    dt = api.deltahours(1)
    n = c.diff_units(t0, c.time(2016, 9, 1), dt)
    ta = api.TimeAxis(t0, dt, n)
    src = api.TimeSeries(ta=ta, values=api.DoubleVector.from_numpy(np.arange(len(ta))),
                         point_fx=api.point_interpretation_policy.POINT_AVERAGE_VALUE)
    common_t0 = c.time(2016, 9, 1)
    return c, t0, dt, src, common_t0, src.partition_by(c, t0, api.Calendar.YEAR, 5, common_t0)


def test_partition_by(api, partitions):
    c, t0, dt, src, common_t0, parts = partitions
    assert isinstance(parts, api.TsVector) and len(parts) == 5
    ty = t0
    for ts in parts:
        ix = ts.index_of(common_t0)
        assert ts.value(ix) == c.diff_units(t0, ty, dt)
        ty = c.add(ty, api.Calendar.YEAR, 1)
    with pytest.raises(RuntimeError, match="t0 must align with a complete calendar multiple dt from t"):
        src.partition_by(c, t0, api.Calendar.YEAR, 5, common_t0 + 3600)
    with pytest.raises(RuntimeError, match="n_partitions should be > 0"):
        src.partition_by(c, t0, api.Calendar.YEAR, 0, common_t0)
    with pytest.raises(RuntimeError, match="partition_interval should be > 0"):
        src.partition_by(c, t0, 0, 5, common_t0)


def test_partitions_are_views_until_read(api, partitions):
    c, t0, dt, src, common_t0, _ = partitions
    parts = src.partition_by(c, t0, api.Calendar.YEAR, 5, common_t0)
    assert all(ts._impl is None for ts in parts)
    assert all(ts.point_interpretation() == api.POINT_AVERAGE_VALUE for ts in parts)
    assert [ts.index_of(common_t0) for ts in parts] == [0, 8760, 17544, 26304, 35064]   # 2012 and 2016 are leap years
    assert all(ts._impl is None for ts in parts)
    ta = api.TimeAxis(common_t0, api.deltahours(24), 365)
    r = api.percentiles(parts, ta, [0, 10, 25, -1, 50, 75, 90, 100])
    assert len(r) == 8 and all(ts._impl is None for ts in parts)
    assert parts[1].value(0) == 0.0 and parts[1]._impl is not None and parts[0]._impl is None
    shifts = [common_t0 - c.add(t0, api.Calendar.YEAR, i) for i in range(5)]
    for ts, d in zip(parts, shifts):
        moved = api.time_shift(src, d)
        assert ts.size() == moved.size() and ts.total_period().start == moved.total_period().start
        assert cases.same_bits(np.asarray(ts.values), np.asarray(moved.values))
        assert [ts.time(i) for i in (0, 1, ts.size() - 1)] == [moved.time(i) for i in (0, 1, moved.size() - 1)]


@pytest.mark.parametrize("fx", ["POINT_AVERAGE_VALUE", "POINT_INSTANT_VALUE"])
def test_percentiles_of_partitions_equal_percentiles_of_time_shifts(api, fx):
    c = api.Calendar()
    t0, common_t0, dt = c.time(2010, 9, 1), c.time(2016, 9, 1), api.deltahours(1)
    n = c.diff_units(t0, common_t0, dt)
    v = np.sin(np.arange(n) / 50.0) * 30 + np.arange(n) % 17
    v[1000:1100] = np.nan
    src = api.TimeSeries(api.TimeAxis(t0, dt, n), v, getattr(api, fx))
    parts = src.partition_by(c, t0, api.Calendar.YEAR, 5, common_t0)
    shifted = api.TsVector([api.time_shift(src, common_t0 - c.add(t0, api.Calendar.YEAR, i)) for i in range(5)])
    ta = api.TimeAxis(common_t0, api.deltahours(24), 365)
    pcts = [0, 10, 25, -1, 50, 75, 90, 100, -1000, 1000]
    a, b = api.percentiles(parts, ta, pcts), shifted.percentiles(ta, pcts)
    assert len(a) == len(b) == len(pcts) and all(ts._impl is None for ts in parts)
    for x, y in zip(a, b):
        assert x.point_interpretation() == getattr(api, fx) and x.size() == 365
        assert cases.same(np.asarray(x.values), np.asarray(y.values))
    assert np.isfinite(np.asarray(a[4].values)).all()


def test_a_vector_of_a_series_an_expression_and_a_view(api, partitions):
    c, t0, dt, src, common_t0, parts = partitions
    ta_src = api.TimeAxis(common_t0, dt, 240)
    concrete = api.TimeSeries(ta_src, np.arange(240.0) % 13, api.POINT_AVERAGE_VALUE)
    view = src.partition_by(c, t0, api.Calendar.YEAR, 5, common_t0)[2]
    tsv = api.TsVector([concrete, concrete * 2.0 + 1.0, view])
    assert tsv[1]._impl is None and tsv[2]._impl is None
    ta = api.TimeAxis(common_t0, api.deltahours(24), 10)
    got = api.percentiles(tsv, ta, [0, 50, 100, -1, -1000, 1000])
    assert tsv[1]._impl is not None and tsv[2]._impl is None   # the expression is evaluated, the view is not
    want = api.percentiles(api.TsVector([concrete, (concrete * 2.0 + 1.0).evaluate(host=True),
                                         api.time_shift(src, view._view_shift)]), ta, [0, 50, 100, -1, -1000, 1000])
    for x, y in zip(got, want):
        assert cases.same(np.asarray(x.values), np.asarray(y.values))


def test_the_planner_copies_the_axis_window_only_and_changes_nothing(api, region):
    """api.percentiles hands each stored series over in the window its views read (view_window,
    host/ts_percentiles.hpp); the values are those of the whole series, on axes inside the series, across its start
    and its end, before and after it, and on one that falls between two points"""
    rng = np.random.default_rng(3)
    n, dt = 1000, 3600
    tsv = api.TsVector()
    for k in range(6):
        v = rng.normal(5.0, 10.0, n)
        v[rng.random(n) < 0.1] = np.nan
        if k == 3:
            v[400:520] = np.nan
        tsv.append(api.TimeSeries(api.TimeAxis(0, dt, n), v, api.POINT_INSTANT_VALUE if k % 2 else api.POINT_AVERAGE_VALUE))
    irregular = np.cumsum(rng.integers(1, 3 * dt, n)).astype(float)
    tsv.append(api.TimeSeries(_impl=api._api._PointTs(irregular.tolist(), float(irregular[-1] + 5), rng.normal(0, 1, n).tolist(),
                                                      api.POINT_INSTANT_VALUE)))
    tsv.append(tsv[0].partition_by(api.Calendar(), 0, api.Calendar.DAY, 3, 20 * 86400)[2])
    stored = [ts._ts for ts in api.TsVector(tsv[:-1])] + [tsv[-1]._view_of._shifted(tsv[-1]._view_shift)]
    pcts = [0, 25, 50, -1, 100, -1000, 1000]
    axes = [(500 * dt, dt, 24), (500 * dt + 7, 1800, 5), (-30 * dt, dt, 48), (990 * dt, dt, 30), (-100 * dt, dt, 20),
            (1500 * dt, dt, 20), (500 * dt + 10, 20, 3), (0, 86400, 45), (999 * dt, dt, 1), (400 * dt, dt // 4, 65)]
    for t0, step, T in axes:
        ta = api.TimeAxis(t0, step, T)
        got = np.array([ts.values for ts in api.percentiles(tsv, ta, pcts)])
        want = region.ts_percentiles(stored, ta, pcts, host=True)
        assert cases.same(got, want), (t0, step, T)
    row = api._api._percentile_rows(stored[:1], [500 * dt * 10**6], [524 * dt * 10**6])[0]
    assert row.tolist() == [0, 25]  # points 500 .. 524: the last one at or before the start to the first at or after the end
