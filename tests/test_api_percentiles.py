"""api.percentiles / TsVector.percentiles (calculate_percentiles, core/time_series_statistics.h:184-246) on the host:
the two scenarios of the reference's shyft/tests/api/test_time_series.py:262-344 with the same numbers (hourly series
onto a daily axis, the min/max-extreme spikes, the embedded NaN), the alternative syntax and an empty vector.
No GPU call."""
import math

import pytest

from shyft_amd import api

WANTED = [api.statistics_property.MIN_EXTREME, 0, 10, 50, api.statistics_property.AVERAGE, 70, 100,
          api.statistics_property.MAX_EXTREME]


def ten_constant_series(ta):
    tsv = api.TsVector()
    for i in range(10):
        tsv.append(api.TimeSeries(ta=ta, fill_value=i, point_fx=api.point_interpretation_policy.POINT_AVERAGE_VALUE))
    return tsv


def test_percentiles():
    c = api.Calendar()
    t0 = c.time(2016, 1, 1)
    dt = api.deltahours(1)
    n = 240
    ta = api.TimeAxisFixedDeltaT(t0, dt, n)
    timeseries = ten_constant_series(ta)
    wanted_percentiles = api.IntVector(WANTED)
    ta_day = api.TimeAxisFixedDeltaT(t0, dt * 24, n // 24)
    ta_day2 = api.TimeAxis(t0, dt * 24, n // 24)
    percentiles = api.percentiles(timeseries, ta_day, wanted_percentiles)
    percentiles2 = timeseries.percentiles(ta_day2, wanted_percentiles)  # the alternative syntax
    assert isinstance(percentiles, api.TsVector)
    assert len(percentiles2) == len(percentiles) == len(WANTED)
    for i in range(len(ta_day)):
        assert percentiles[0].value(i) == pytest.approx(0.0, abs=1e-3)  # min-extreme
        assert percentiles[1].value(i) == pytest.approx(0.0, abs=1e-3)  # 0-percentile
        assert percentiles[2].value(i) == pytest.approx(0.9, abs=1e-3)  # 10-percentile
        assert percentiles[3].value(i) == pytest.approx(4.5, abs=1e-3)  # 50-percentile
        assert percentiles[4].value(i) == pytest.approx(4.5, abs=1e-3)  # average
        assert percentiles[5].value(i) == pytest.approx(6.3, abs=1e-3)  # 70-percentile
        assert percentiles[6].value(i) == pytest.approx(9.0, abs=1e-3)  # 100-percentile
        assert percentiles[7].value(i) == pytest.approx(9.0, abs=1e-3)  # max-extreme
    for a, b in zip(percentiles, percentiles2):  # TsVector.percentiles equals api.percentiles
        assert list(a.values) == list(b.values)
        assert a.size() == len(ta_day)
        assert a.point_interpretation() == api.point_interpretation_policy.POINT_AVERAGE_VALUE


def test_percentiles_with_min_max_extremes():
    c = api.Calendar()
    t0 = c.time(2016, 1, 1)
    dt = api.deltahours(1)
    n = 240
    ta = api.TimeAxis(t0, dt, n)
    timeseries = ten_constant_series(ta)
    ts = timeseries[1]  # this one gets the extremes
    for i in range(0, 240, 24):
        ts.set(i + 0, 1.0 - 100 * i / 24.0)
        ts.set(i + 1, 1.0 + 100 * i / 24.0)  # when i == 0 this gives 1.0
        ts.set(i + 2, float("nan"))  # ignored by the average
    ta_day = api.TimeAxis(t0, dt * 24, n // 24)
    percentiles = api.percentiles(timeseries, ta_day, api.IntVector(WANTED))
    for i in range(len(ta_day)):
        if i == 0:  # first day: the extremes come from series 0 and 9
            assert percentiles[0].value(i) == pytest.approx(0.0, abs=1e-3)
            assert percentiles[7].value(i) == pytest.approx(9.0, abs=1e-3)
        else:
            assert percentiles[0].value(i) == pytest.approx(1.0 - 100.0 * i * 24.0 / 24.0, abs=1e-3)
            assert percentiles[7].value(i) == pytest.approx(1.0 + 100.0 * i * 24.0 / 24.0, abs=1e-3)
        assert percentiles[1].value(i) == pytest.approx(0.0, abs=1e-3)
        assert percentiles[2].value(i) == pytest.approx(0.9, abs=1e-3)
        assert percentiles[3].value(i) == pytest.approx(4.5, abs=1e-3)
        assert percentiles[4].value(i) == pytest.approx(4.5, abs=1e-3)
        assert percentiles[5].value(i) == pytest.approx(6.3, abs=1e-3)
        assert percentiles[6].value(i) == pytest.approx(9.0, abs=1e-3)


def test_first_series_sets_the_point_interpretation():
    t0 = api.Calendar().time(2016, 1, 1)
    ta = api.TimeAxis(t0, api.deltahours(1), 4)
    tsv = api.TsVector()
    tsv.append(api.TimeSeries(ta=ta, fill_value=1.0, point_fx=api.point_interpretation_policy.POINT_INSTANT_VALUE))
    tsv.append(api.TimeSeries(ta=ta, fill_value=3.0, point_fx=api.point_interpretation_policy.POINT_AVERAGE_VALUE))
    r = tsv.percentiles(ta, [50, 101])
    assert r[0].point_interpretation() == api.point_interpretation_policy.POINT_INSTANT_VALUE
    assert r[0].value(0) == 2.0
    assert all(math.isnan(r[1].value(i)) for i in range(4))  # not a statistics property


def test_empty_vector_and_empty_list():
    t0 = api.Calendar().time(2016, 1, 1)
    ta = api.TimeAxis(t0, api.deltahours(1), 5)
    r = api.percentiles(api.TsVector(), ta, WANTED)
    assert len(r) == len(WANTED)
    for ts in r:
        assert ts.size() == 5
        assert all(math.isnan(ts.value(i)) for i in range(5))
    assert len(api.percentiles(ten_constant_series(ta), ta, [])) == 0
