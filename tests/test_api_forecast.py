"""TsVector.average_slice, TsVector.nash_sutcliffe and api.forecast_skill on the device: each is one device call and
equals its host=True twin bit for bit; the table of api.forecast_skill equals the single calls cell by cell."""
import math

import numpy as np
import pytest

from tests import resample_cases as rc

pytestmark = pytest.mark.gpu

HOUR = 3600


@pytest.fixture(scope="module")
def api():
    from shyft_amd import api
    return api


@pytest.fixture(scope="module")
def region():
    from shyft_amd import region
    return region


@pytest.fixture(scope="module")
def locations(api):
    """3 locations: 12 hourly 66-step forecasts 6 h apart (some values NaN) and an observation of 120 hours, which
    the late slices run past; the third location's observation is irregular and linear between points"""
    rng = np.random.default_rng(5)
    t0 = api.Calendar().time(2017, 1, 1)
    sets, observations = api.TsVectorSet(), api.TsVector()
    for loc in range(3):
        fc = api.TsVector()
        for i in range(12):
            v = np.sin(0.314 + 3.14 * (i * 6 + np.arange(66)) / 240.0) * (1.0 + loc) + rng.normal(0.0, 0.05, 66)
            v[rng.random(66) < 0.05] = np.nan
            fc.append(api.TimeSeries(api.TimeAxis(t0 + i * 6 * HOUR, HOUR, 66), v, api.POINT_AVERAGE_VALUE))
        sets.append(fc)
        truth = np.sin(0.314 + 3.14 * np.arange(120) / 240.0) * (1.0 + loc)
        if loc == 2:
            times = [t0 + i * HOUR + (0 if i == 0 else int(rng.integers(0, 1800))) for i in range(120)]
            observations.append(api.TsFactory().create_time_point_ts(api.UtcPeriod(t0, t0 + 120 * HOUR), times, truth,
                                                                     api.POINT_INSTANT_VALUE))
        else:
            observations.append(api.TimeSeries(api.TimeAxis(t0, HOUR, 120), truth, api.POINT_AVERAGE_VALUE))
    return sets, observations


def test_average_slice_is_one_device_call_and_equals_the_host(api, region, locations):
    fc = api.TsVector(locations[0][0])
    empty = api.TimeSeries(api.TimeAxis(0, HOUR, 0), [], api.POINT_AVERAGE_VALUE)
    fc.insert(3, empty)
    for lead, dt, n in ((0, HOUR, 6), (5 * HOUR, 2 * HOUR, 12), (60 * HOUR, 3 * HOUR, 4), (HOUR // 2, 1800, 65)):
        n0 = region.forecast_skill_calls()
        dev = fc.average_slice(lead, dt, n)
        assert region.forecast_skill_calls() == n0 + 1
        host = fc.average_slice(lead, dt, n, host=True)
        assert region.forecast_skill_calls() == n0 + 1
        assert len(dev) == len(host) == len(fc) and dev[3] is empty
        for k, (d, h) in enumerate(zip(dev, host)):
            if k == 3:
                continue
            assert d.size() == n and d.time(0) == fc[k].time(0) + lead and d.total_period().end == d.time(0) + n * dt
            assert d.point_interpretation() == api.POINT_AVERAGE_VALUE
            assert rc.same_bits(np.asarray(d.values), np.asarray(h.values)), (lead, dt, n, k)
            want = fc[k].average(api.TimeAxis(fc[k].time(0) + lead, dt, n))
            assert rc.same_bits(np.asarray(d.values), np.asarray(want.values))


def test_nash_sutcliffe_is_one_device_call_and_equals_the_host(api, region, locations):
    sets, observations = locations
    for loc in range(3):
        for lead, dt, n in ((0, HOUR, 6), (7 * HOUR, 2 * HOUR, 3), (48 * HOUR, HOUR, 12)):
            n0 = region.forecast_skill_calls()
            dev = sets[loc].nash_sutcliffe(observations[loc], lead, dt, n)
            assert region.forecast_skill_calls() == n0 + 1
            host = sets[loc].nash_sutcliffe(observations[loc], lead, dt, n, host=True)
            assert region.forecast_skill_calls() == n0 + 1
            assert math.isfinite(host) and host <= 1.0
            assert rc.same_bits(np.asarray([dev]), np.asarray([host])), (loc, lead, dt, n, dev, host)


def test_forecast_skill_table_is_one_device_call_and_equals_the_single_calls(api, region, locations):
    sets, observations = locations
    leads = [0, 6 * HOUR, 12 * HOUR, 30 * HOUR, 59 * HOUR]
    n0 = region.forecast_skill_calls()
    table = api.forecast_skill(sets, observations, leads, HOUR, 6)
    assert region.forecast_skill_calls() == n0 + 1
    assert table.shape == (3, 5) and np.isfinite(table).all()
    assert rc.same_bits(table, api.forecast_skill(sets, observations, leads, HOUR, 6, host=True))
    assert region.forecast_skill_calls() == n0 + 1
    single = np.array([[sets[loc].nash_sutcliffe(observations[loc], lead, HOUR, 6) for lead in leads] for loc in range(3)])
    assert region.forecast_skill_calls() == n0 + 16
    assert rc.same_bits(table, single)
    assert (table <= 1.0).all()  # 1 - a quotient of two sums of squares
    # a location without forecasts and one without an observation are NaN rows, as the single calls are
    sets2 = api.TsVectorSet([sets[0], api.TsVector(), sets[2]])
    obs2 = api.TsVector([observations[0], observations[1],
                         api.TimeSeries(api.TimeAxis(0, HOUR, 0), [], api.POINT_AVERAGE_VALUE)])
    table2 = api.forecast_skill(sets2, obs2, leads, HOUR, 6)
    assert rc.same_bits(table2[0], table[0]) and np.isnan(table2[1:]).all()
