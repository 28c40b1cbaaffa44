"""pt_gs_k and pt_ss_k off the hourly 2015 time axis, on the CPU: the oracle's calendar against Python's datetime
(proleptic Gregorian, independent of the C++ copies), Skaugen's accumulation across step lengths, and the conditions
on the cases of tests/time_axis_cases.py that make tests/test_time_axis_gpu.py worth running: each is asserted on the
oracle alone, so a case that stops exercising its event fails here and not silently there. (The library's own calendar
tables are checked by tools/host_tables_check.cpp, tests/test_host_tables.py; kirchner at other step lengths in
tests/test_oracle_bounds.py.)"""
import datetime as dt_

import numpy as np
import pytest

from tests import oracle_lib
from tests import time_axis_cases as tc

YEAR_RANGES = ((1899, 1901), (1967, 1972), (1999, 2001), (2015, 2017), (2099, 2101), (2399, 2401))


def _check_instant(L, t):
    assert L.oracle_day_of_year(t) == tc.day_of_year(t), (t, tc.when(t))
    assert L.oracle_trim_year(t) == t - tc.time_in_year_us(t), (t, tc.when(t))


def test_oracle_calendar_equals_datetime_at_every_midnight():
    """calendar::day_of_year and trim(t, YEAR) (utctime_utilities.cpp:230-253) at every midnight of the years around
    the century rule, the epoch and the leap years the cases use, and 1 us before and after it: exact."""
    L = oracle_lib.load()
    for y0, y1 in YEAR_RANGES:
        day = dt_.date(y0, 1, 1)
        while day.year <= y1:
            t = tc.utc(day.year, day.month, day.day)
            for d in (-1, 0, 1):
                _check_instant(L, t + d)
            day += dt_.timedelta(days=1)


def test_oracle_calendar_equals_datetime_at_random_instants():
    L = oracle_lib.load()
    rng = np.random.default_rng(1800)
    for t in rng.integers(tc.utc(1800, 1, 1), tc.utc(2501, 1, 1), 4000):
        _check_instant(L, int(t))


def test_skaugen_accumulation_is_the_same_in_one_daily_step_as_in_24_hourly():
    """24 cold hourly steps (-10 degC, 0.5 mm/h) against one 24 h step of the same input: the stored snow swe * sca.
    Tolerance 1e-12 relative: 24 rounded additions of a value near 12 mm are within 24 * 2^-53 = 2.7e-15 of the single
    product 0.5 * 24, and the rest of the cold step is the same expression; 1e-12 leaves room for the unit-count
    rounding of the state. (Measured: exactly equal.)"""
    hourly = np.array([4.077, 40.77, 0.0, 0.0, 0.0, 0.0, 0.0])
    daily = hourly.copy()
    for _ in range(24):
        oracle_lib.skaugen_step(hourly, tc.HOUR, -10.0, 0.5)
    oracle_lib.skaugen_step(daily, tc.DAY, -10.0, 0.5)
    a, b = hourly[3] * hourly[2], daily[3] * daily[2]
    print("swe*sca hourly", repr(a), "daily", repr(b))
    assert a > 11.0 and abs(a - b) <= 1e-12 * abs(b)


# ---- conditions on the cases ----

@pytest.mark.parametrize("name", tc.NAMES)
@pytest.mark.parametrize("stack", ["pt_gs_k", "pt_ss_k"])
def test_every_axis_gives_finite_series(stack, name):
    r = tc.oracle(stack, name)
    for k in ("full", "state_series", "state"):
        assert np.isfinite(r[k]).all(), k


@pytest.mark.parametrize("name", tc.NAMES)
def test_axis_is_small_and_its_start_is_what_its_name_says(name):
    t0, dt, T = tc.AXIS[name]
    assert 0 < T <= 64 and dt > 0
    if "pre_epoch" in name:
        assert all(t < 0 for t in tc.times(name))
    if name == "odd_dt":
        assert (dt / 1e6) != int(dt / 1e6) and dt % tc.HOUR != 0


@pytest.mark.parametrize("name", tc.NAMES)
def test_second_set_has_its_start_melt_day_and_a_season_edge_inside_the_axis(name):
    """Recomputed with datetime: the first step whose day of year is winter_end_day_of_year is neither the first nor
    absent, and is_snow_season (gamma_snow.h:89-93) flips between two steps of the axis."""
    wed, nwd = tc.SECOND_SET[name]
    ts = tc.times(name)
    doy = [tc.day_of_year(t) for t in ts]
    assert wed in doy and doy[0] != wed, doy
    lo, hi = (wed - nwd) * tc.DAY, wed * tc.DAY
    season = [lo <= tc.time_in_year_us(t) < hi for t in ts]
    assert any(a != b for a, b in zip(season, season[1:])), season
    p = tc.ptgsk_sets(name)[1]
    assert p[tc.PK_ISO] == 1.0 and (p[tc.PK_WED], p[tc.PK_NWD]) == (wed, nwd)


def test_year_end_axis_reaches_doy_366_then_wraps():
    ts = tc.times("24h_year_end_leap")
    doy = [tc.day_of_year(t) for t in ts]
    k = doy.index(366)
    assert doy[k + 1] == 1 and tc.time_in_year_us(ts[k + 1]) == 0
    sets = tc.ptgsk_sets("24h_year_end_leap")
    assert (sets[0][tc.PK_WED], sets[1][tc.PK_WED]) == (366, 1)
    # the odd axis has New Year inside a step
    ts = tc.times("odd_dt")
    years = [tc.when(t).year for t in ts]
    k = years.index(2015)
    assert 0 < k and ts[k] - tc.time_in_year_us(ts[k]) > ts[k - 1] and tc.time_in_year_us(ts[k]) > 0


def _sets_with_event(name):
    """parameter sets whose winter_end_day_of_year lies on the axis (or on it moved by a day)"""
    doy = {tc.day_of_year(t) for t in tc.times(name)}
    return [s for s in (0, 1) if int(tc.ptgsk_sets(name)[s][tc.PK_WED]) in doy]


@pytest.mark.parametrize("name", tc.NAMES)
def test_calendar_is_observable_for_ptgsk(name):
    """The same forcing and state on the axis moved by one day give another state series, in cells of every
    parameter set with an event on the axis: the day-of-year and time-in-year tables reach the result."""
    a, b = tc.oracle("pt_gs_k", name), tc.oracle("pt_gs_k", name, shift_us=tc.DAY)
    differs = (a["state_series"] != b["state_series"]).any(axis=(0, 1))
    assert differs.any()
    events = _sets_with_event(name)
    assert 1 in events
    for s in events:
        assert differs[tc.set_ix() == s].any(), f"set {s}"


@pytest.mark.parametrize("stack", ["pt_gs_k", "pt_ss_k"])
def test_step_length_is_observable(stack):
    a = tc.oracle(stack, "3h_leap")
    b = tc.oracle(stack, "3h_leap", dt_us=tc.HOUR)
    assert (a["full"][0] != b["full"][0]).any()


def test_ptgsk_winter_axis_has_snowfall_on_a_wet_pack():
    """The corr_lwc (Brent job) path of gamma_snow.h:377: snow falls on an accumulating pack that holds liquid water
    and adds more than 1 % to it. From the oracle's state series of the default set on 3h_leap."""
    name = "3h_leap"
    assert name in tc.WINTER
    _, p, _, _, f = tc.inputs("pt_gs_k", name, 0)
    s = tc.oracle("pt_gs_k", name, 0)["state_series"][:, :-1]
    lwc, sdc, acc = s[2], s[5], s[6]
    dt = tc.AXIS[name][1]
    snow = np.where(f[0] < p[0][4], f[1] * p[0][16] * dt / tc.HOUR, 0.0)
    sdc_snow = snow / (1.0 - p[0][21])
    jobs = (acc < 0.0) & (lwc > 0.0) & (sdc > 0.0) & (snow > 1e-10) & (sdc_snow > 0.01 * (sdc + sdc_snow))
    print("steps with jobs", int(jobs.any(axis=1).sum()), "jobs", int(jobs.sum()))
    assert jobs.any(axis=1).sum() >= 3


@pytest.mark.parametrize("name", ["3h_leap", "24h_2000", "24h_2100"])
def test_ptssk_reaches_partial_snow_cover(name):
    """0 < sca < 1: partial melts went through sca_rel_red. (The year-end axes stay below -2 degC: no melt there.)"""
    sca = tc.oracle("pt_ss_k", name)["state_series"][1]
    partial = (sca > 0.0) & (sca < 1.0)
    print("cells with partial cover", int(partial.any(axis=0).sum()))
    assert partial.any()


@pytest.mark.parametrize("name", tc.NAMES)
def test_both_stacks_hold_a_snow_pack(name):
    for stack in ("pt_gs_k", "pt_ss_k"):
        swe = tc.oracle(stack, name)["full"][3]
        assert swe.max() > 10.0, (stack, swe.max())
