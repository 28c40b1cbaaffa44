"""Forecast skill by lead time and the forecast merge on the host (host/forecast.hpp through host=True and
TsVector.forecast_merge): the reference's own scenarios (shyft/tests/api/test_ts_vector_nash_sutcliffe.py,
test_forecast_merge.py and test/merge_test.cpp:92-190) written afresh, the NaN and inf handling of the score, and the
refusals of shyft_hip_forecast_skill and its host twin, which come before the first HIP call and so run without a
GPU."""
import math

import numpy as np
import pytest

from tests import forecast_cases as fcs
from tests import resample_cases as rc

HOUR = 3600
SEC = 10**6


@pytest.fixture(scope="module")
def api():
    from shyft_amd import api
    return api


@pytest.fixture(scope="module")
def region():
    from shyft_amd import region
    return region


def two_pass_score(obs, sim):
    """1 - nash_sutcliffe_goal_function (core/time_series.h:2316-2344) in plain Python floats, sequentially"""
    err2 = mean = 0.0
    count = 0
    for o, m in zip(obs, sim):
        if math.isfinite(o) and math.isfinite(m):
            d = o - m
            err2 += d * d
            mean += o
            count += 1
    mean = mean / float(count) if count else float("nan")
    var2 = 0.0
    for o, m in zip(obs, sim):
        if math.isfinite(o) and math.isfinite(m):
            d = o - mean
            var2 += d * d
    if var2 == 0.0:  # IEEE division, which Python refuses to do
        return 1.0 - (float("nan") if err2 == 0.0 or err2 != err2 else math.copysign(float("inf"), err2))
    return 1.0 - err2 / var2


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def arome(api):
    """the reference's Python scenario: 40 hourly 66-step forecasts 6 h apart and the observation under them"""
    t0 = api.Calendar().time(2017, 1, 1)
    fc = api.TsVector()
    for i in range(40):
        v = [math.sin(0.314 + 3.14 * (i * 6 + t) / 240.0) for t in range(66)]
        fc.append(api.TimeSeries(api.TimeAxis(t0 + i * 6 * HOUR, HOUR, 66), v, api.POINT_AVERAGE_VALUE))
    obs = api.TimeSeries(api.TimeAxis(t0, HOUR, 240), [math.sin(0.314 + 3.14 * i / 240.0) for i in range(240)],
                         api.POINT_AVERAGE_VALUE)
    return fc, obs


GRID = [(lead, n, dt) for lead in range(12) for n in (1, 2, 3, 4, 6, 12) for dt in (1, 2, 3)]


def test_average_slice_is_the_average_of_the_same_portion_and_the_score_its_two_pass_sum(api, arome):
    fc, obs = arome
    for lead, n, dt in GRID:
        slices = fc.average_slice(lead * HOUR, dt * HOUR, n, host=True)
        assert len(slices) == len(fc)
        sim, ob = [], []
        for s, f in zip(slices, fc):
            ta = api.TimeAxis(f.time(0) + lead * HOUR, dt * HOUR, n)
            expected = f.average(ta)
            assert s.size() == n and s.point_interpretation() == api.POINT_AVERAGE_VALUE
            assert [s.time(i) for i in range(n)] == [ta.time(i) for i in range(n)]
            assert s.total_period().end == ta.total_period()[1]
            assert rc.same_bits(np.asarray(s.values), np.asarray(expected.values)), (lead, n, dt)
            sim.extend(expected.values)
            ob.extend(obs.average(ta).values)
        ns = fc.nash_sutcliffe(obs, lead * HOUR, dt * HOUR, n, host=True)
        want = two_pass_score(ob, sim)
        assert bits(ns) == bits(want), (lead, n, dt, ns, want)
        assert abs(ns - 1.0) < 0.05  # the reference's assertAlmostEqual(ns, 1.0, 1)


def test_the_reference_cpp_scenario_lies_inside_its_bounds(api):
    t0 = api.Calendar().time(2017, 1, 1)
    fc = api.TsVector()
    for i in range(100):
        v = [(i * 6 + t) + math.sin(0.314 + 3.14 * (i * 6 + t) / 240.0) for t in range(66)]
        fc.append(api.TimeSeries(api.TimeAxis(t0 + i * 6 * HOUR, HOUR, 66), v, api.POINT_AVERAGE_VALUE))
    n_obs = 6 * 100 + 66
    obs = api.TimeSeries(api.TimeAxis(t0, HOUR, n_obs), [i + 1.5 * math.cos(3.1415 * i / 240.0) for i in range(n_obs)],
                         api.POINT_AVERAGE_VALUE)
    ns = fc.nash_sutcliffe(obs, 0, HOUR, 6, host=True)
    print("ns", repr(ns))
    assert 0.99996 <= ns <= 1.0
    assert abs(ns - 0.999966088973) < 1e-11  # a numpy restatement of the scenario


def _merge_forecasts(api, n_fc):
    t0 = api.Calendar().time(2017, 1, 1)
    fc = api.TsVector()
    for i in range(n_fc):
        fc.append(api.TimeSeries(api.TimeAxis(t0 + i * 6 * HOUR, HOUR, 66), [i + t / 66.0 for t in range(66)],
                                 api.POINT_AVERAGE_VALUE))
    return t0, fc


def test_forecast_merge_of_the_reference_scenario(api):
    n_fc = 10
    t0, fc = _merge_forecasts(api, n_fc)
    for lead in range(12):
        m = fc.forecast_merge(lead * HOUR, 6 * HOUR)
        assert m.size() == n_fc * 6 and m.point_interpretation() == api.POINT_AVERAGE_VALUE
        for i in range(m.size()):
            k = i // 6
            assert abs(m.value(i) - (k + (i + lead - k * 6) / 66.0)) <= 1e-10
            assert m.time(i) == t0 + lead * HOUR + i * HOUR
        assert m.total_period().end == t0 + lead * HOUR + m.size() * HOUR


def test_forecast_merge_fills_a_missing_forecast_from_its_neighbours(api):
    n_fc = 10
    t0, fc = _merge_forecasts(api, n_fc)
    del fc[1]
    for lead in range(20):
        m = fc.forecast_merge(lead * HOUR, 6 * HOUR)
        assert m.size() == n_fc * 6
        for i in range(m.size()):
            k, hour = i // 6, i % 6
            if k == 1:
                k = 0 if hour + lead < 6 else 2
            assert abs(m.value(i) - (k + (i + lead - k * 6) / 66.0)) <= 1e-10, (lead, i)
            assert m.time(i) == t0 + lead * HOUR + i * HOUR
        assert m.total_period().end == t0 + lead * HOUR + m.size() * HOUR


def test_forecast_merge_python_scenario_empty_vector_and_errors(api):
    t0 = api.Calendar().time(2017, 1, 1)
    fc = api.TsVector()
    for i in range(40):
        mrk = (i + 1) / 100.0
        fc.append(api.TimeSeries(api.TimeAxis(t0 + i * 6 * HOUR, HOUR, 66),
                                 np.linspace(1 + mrk, 1 + 66 + mrk, 66, endpoint=False), api.POINT_AVERAGE_VALUE))
    m0_6, m1_7 = fc.forecast_merge(0, 6 * HOUR), fc.forecast_merge(HOUR, 6 * HOUR)
    assert m0_6.size() == m1_7.size() == 40 * 6
    assert m0_6.value(0) == pytest.approx(1.01) and m0_6.value(6) == pytest.approx(1.02)
    assert m1_7.value(0) == pytest.approx(2.01) and m1_7.value(6) == pytest.approx(2.02)
    assert api.TsVector().forecast_merge(0, 6 * HOUR).size() == 0
    with pytest.raises(RuntimeError, match="lead_time parameter should be 0 or a positive number"):
        fc.forecast_merge(-1, 6 * HOUR)
    with pytest.raises(RuntimeError, match="fc_interval parameter should be positive number"):
        fc.forecast_merge(0, 0)
    with pytest.raises(RuntimeError, match="at least fc_interval: requirement broken at index:1"):
        fc.forecast_merge(0, 7 * HOUR)
    with pytest.raises(RuntimeError, match="forecast_merge: forecast 0 ends inside its slice"):
        fc.forecast_merge(61 * HOUR, 6 * HOUR)
    # a walk that takes the last point asks for the time of the next one, as the reference's does: 60 h + 6 h of 66
    with pytest.raises(RuntimeError, match="forecast_merge: forecast 0 ends inside its slice"):
        fc.forecast_merge(60 * HOUR, 6 * HOUR)
    assert fc.forecast_merge(59 * HOUR, 6 * HOUR).size() == 40 * 6
    late = api.TsVector([fc[0], fc[30]])    # the first forecast cannot reach the start of the second
    with pytest.raises(RuntimeError, match="forecast_merge: forecast 0 ends inside its slice"):
        late.forecast_merge(0, 6 * HOUR)


def test_scores_without_finite_pairs_and_against_a_constant_observation(api):
    nan, inf = float("nan"), float("inf")
    ta = api.TimeAxis(0, HOUR, 6)
    series = lambda v: api.TimeSeries(ta, v, api.POINT_AVERAGE_VALUE)  # noqa: E731
    fc = api.TsVector([series([1.0, 2.0, 3.0, nan, inf, 4.0])])
    assert math.isnan(fc.nash_sutcliffe(series([nan, nan, -inf, 1.0, 2.0, inf]), 0, HOUR, 6, host=True))
    assert fc.nash_sutcliffe(series([2.0] * 6), 0, HOUR, 6, host=True) == -inf
    assert math.isnan(api.TsVector([series([2.0] * 6)]).nash_sutcliffe(series([2.0] * 6), 0, HOUR, 6, host=True))
    # the reference's early NaN, and its goal function's refusal of no pairs at all
    assert math.isnan(api.TsVector().nash_sutcliffe(series([2.0] * 6), 0, HOUR, 6, host=True))
    assert math.isnan(fc.nash_sutcliffe(api.TimeSeries(api.TimeAxis(0, HOUR, 0), [], api.POINT_AVERAGE_VALUE), 0, HOUR, 6,
                                        host=True))
    with pytest.raises(RuntimeError, match="nash_sutcliffe needs equal sized ts accessors with elements >1"):
        fc.nash_sutcliffe(series([2.0] * 6), 0, HOUR, 0, host=True)
    for bad, text in (((0, HOUR, -1), "n, number of intervals, must be specified as > 0"),
                      ((0, 0, 6), "dt, average interval, must be specified as > 0 s"),
                      ((-1, HOUR, 6), "lead_time,t0_offset,must be specified  >= 0 s")):
        with pytest.raises(RuntimeError, match=text):
            fc.nash_sutcliffe(series([2.0] * 6), *bad, host=True)
        with pytest.raises(RuntimeError, match=text):
            fc.average_slice(*bad, host=True)
    empty = api.TimeSeries(api.TimeAxis(0, HOUR, 0), [], api.POINT_AVERAGE_VALUE)
    passed = api.TsVector([empty, fc[0]]).average_slice(0, 2 * HOUR, 3, host=True)
    assert passed[0] is empty and passed[1].size() == 3 and passed[1].value(0) == 1.5


def test_free_nash_sutcliffe_and_kling_gupta_are_one_minus_the_goal_functions(api):
    ta = api.TimeAxis(0, HOUR, 48)
    obs = api.TimeSeries(ta, [math.sin(i / 5.0) + 2.0 for i in range(48)], api.POINT_AVERAGE_VALUE)
    mod = api.TimeSeries(ta, [math.sin(i / 5.0 + 0.1) + 2.1 for i in range(48)], api.POINT_AVERAGE_VALUE)
    daily = api.TimeAxis(0, 6 * HOUR, 8)
    o, m = list(obs.average(daily).values), list(mod.average(daily).values)
    assert api.nash_sutcliffe(obs, obs, ta) == 1.0 and api.kling_gupta(obs, obs, ta, 1.0, 1.0, 1.0) == 1.0
    assert bits(api.nash_sutcliffe(obs, mod, daily)) == bits(two_pass_score(o, m))
    assert api.nash_sutcliffe(obs, mod, daily) == 1.0 - api.nash_sutcliffe_goal_function(o, m)
    assert api.kling_gupta(obs, mod, daily, 1.0, 0.5, 2.0) == 1.0 - api.kling_gupta_goal_function(o, m, 1.0, 0.5, 2.0)
    assert 0.0 < api.kling_gupta(obs, mod, daily, 1.0, 1.0, 1.0) < 1.0


def test_host_twin_slices_are_the_resample_averages_and_the_score_their_two_pass_sum(region):
    """the batch of the GPU tests through the host twin alone: every slice equals shyft_hip_resample_host of the same
    series on the same axis, and every score the plain-Python sum over them"""
    for epoch in range(3):
        batch, prob = fcs.make_case(14, 1, epoch, 50 + epoch)
        row, t = batch[0], batch[1]
        fc_row, fc_ix, obs_ix, off, dt, n = prob
        ns, sim, obs = region.forecast_skill_csr(*batch, *prob, host=True, slices=True)
        j = 0
        for p in range(len(n)):
            first = j
            for f in fc_ix[fc_row[p]:fc_row[p + 1]]:
                ta_t0 = int(t[row[f]] + off[p])
                pair = fcs.pick(batch, [f, max(int(obs_ix[p]), 0)])
                avg = region.resample_csr(*pair, ta_t0, int(dt[p]), int(n[p]), host=True)
                assert rc.same_bits(sim[j:j + n[p]], avg[:, 0])
                assert rc.same_bits(obs[j:j + n[p]], avg[:, 1] if obs_ix[p] >= 0 else np.full(n[p], np.nan))
                j += n[p]
            want = two_pass_score(obs[first:j].tolist(), sim[first:j].tolist())
            assert rc.same_bits(ns[p:p + 1], np.asarray([want])), (epoch, p, ns[p], want)
        assert j == len(sim) == len(obs)
        assert np.isfinite(ns).any() and np.isnan(ns).any() and np.isfinite(sim).any() and np.isnan(sim).any()


def _pool():
    """three forecasts of 3, 2 and 0 points, an observation of 4 points and one of 1 point"""
    return dict(row=np.array([0, 3, 5, 5, 9, 10], dtype=np.int64),
                t=np.array([0, 1, 2, 1, 2, 0, 1, 2, 3, 1], dtype=np.int64) * SEC + np.array([0] * 9 + [SEC // 2]),
                v=np.arange(10.0), t_end=np.array([3, 3, 0, 4, 2], dtype=np.int64) * SEC,
                fx=np.array([1, 0, 1, 1, 1], dtype=np.int32))


def _skill(region, host, **kw):
    a = dict(_pool(), fc_row=[0, 2], fc_ix=[0, 1], obs_ix=[3], t0_offset=0, dt=SEC, n=2)
    a.update(kw)
    return region.forecast_skill_csr(a["row"], a["t"], a["v"], a["t_end"], a["fx"], a["fc_row"], a["fc_ix"], a["obs_ix"],
                                     a["t0_offset"], a["dt"], a["n"], host=host)


REFUSALS = [
    (dict(fc_ix=[0, 2]), "forecast_skill: a forecast has no points"),
    (dict(dt=0), "dt, average interval, must be specified as > 0 s"),
    (dict(dt=-SEC), "dt, average interval, must be specified as > 0 s"),
    (dict(t0_offset=-1), "lead_time,t0_offset,must be specified  >= 0 s"),
    (dict(n=-1), "n, number of intervals, must be specified as > 0"),
    (dict(fc_ix=[0, 5]), "forecast_skill: a forecast index lies outside the series"),
    (dict(fc_ix=[-1, 1]), "forecast_skill: a forecast index lies outside the series"),
    (dict(obs_ix=[5]), "forecast_skill: an observation index lies outside the series"),
    (dict(obs_ix=[-2]), "forecast_skill: an observation index lies outside the series"),
    (dict(obs_ix=[4]), "point_dt.time(i): a one-point series cannot be integrated over a period that starts before its "
                       "point and holds it"),
    (dict(t0_offset=2**62), "forecast_skill: times beyond a quarter of the 64-bit range are not supported"),
    (dict(n=2**62), "forecast_skill: times beyond a quarter of the 64-bit range are not supported"),
    (dict(t=_pool()["t"][::-1].copy()), "time_axis::point_dt() needs time-points in increasing order"),
]


@pytest.mark.parametrize("host", (False, True))
@pytest.mark.parametrize("change,text", REFUSALS)
def test_refusals_come_before_any_launch_with_their_texts(region, host, change, text):
    from shyft_amd._native import ShyftHipError
    n0 = region.forecast_skill_calls()
    with pytest.raises(ShyftHipError) as e:
        _skill(region, host, **change)
    assert str(e.value) == text
    assert region.forecast_skill_calls() == n0


def test_the_accepted_pool_and_a_one_point_observation_on_a_period_start(region):
    ns = _skill(region, True)
    assert ns.shape == (1,) and math.isfinite(ns[0])
    # the one-point observation at 1.5 s: refused inside a period, taken when a period starts on it
    ns, sim, obs = region.forecast_skill_csr(*_pool().values(), [0, 1], [0], [4], SEC // 2, SEC, 2, host=True, slices=True)
    assert rc.same_bits(obs, np.asarray([np.nan, 9.0]))
    # nothing to do: NaN scores, no slices
    ns, sim, obs = region.forecast_skill_csr(*_pool().values(), [0, 2, 2], [0, 1], [3, 3], 0, SEC, 0, host=True, slices=True)
    assert np.isnan(ns).all() and ns.shape == (2,) and sim.shape == obs.shape == (0,)
    assert region.forecast_skill_csr(*_pool().values(), [0], [], [], 0, SEC, 2, host=True).shape == (0,)
