"""Time axes off the hourly 2015 grid, shared by tests/test_time_axis_host.py (CPU: the conditions that make the
cases worth running) and tests/test_time_axis_gpu.py (device against oracle, bit for bit).

Every axis is (name, t0_us, dt_us, T) with T <= 64, the smallest that still contains its events:

  3h_leap                2016-02-27T00Z, 3 h: Feb 29 (doy 60) from step 16, Mar 1 (doy 61 only in a leap year) from 24
  24h_year_end_leap      2016-12-28, 24 h: doy 366 at step 3; at step 4 doy is 1 and the time in the year wraps to 0
  1h_year_end_pre_epoch  1967-12-31T12Z, 1 h: negative times, New Year into the leap year 1968 at step 12
  3h_pre_epoch_leap      1968-02-28, 3 h: Feb 29 from step 8, Mar 1 from step 16, all before 1970
  15min_wed              2015-04-09T22:00Z, 900 s: the default winter_end_day_of_year 100 begins at step 8
  odd_dt                 2014-12-31T20:30:12.345678Z, 7 min + 1 us: dt in seconds is no integer, dt in hours is not
                         representable, and New Year falls inside step 29
  24h_2100               2100-02-27, 24 h: 2100 is not a leap year
  24h_2000               2000-02-27, 24 h: 2000 is one

odd_dt keeps the 12 345 678 us offset from a whole second but starts 3.5 h before 2015-01-01 and not at it: from
there 60 steps of 7 min reach no day boundary, and the second parameter set needs its start_melt day and a
snow-season edge inside the axis.

Forcing is synthetic.forcing's hourly year sampled at each step's starting hour of the year (modulo 8760), so the
winter axes snow and the spring axes melt. The starting state comes from the oracle run hourly over the weeks before
t0 with the default parameters, so every axis starts on a snow pack. pt_gs_k has two parameter sets, the default one
and one with calculate_iso_pot_energy whose winter_end_day_of_year / n_winter_days put the start_melt day and a
snow-season edge inside the axis; pt_ss_k two copies of the default differing in one Skaugen parameter.

The oracle results are computed once per (axis, launch) and shared read-only."""
from __future__ import annotations

import datetime as dt_
import functools

import numpy as np

from shyft_amd import synthetic
from tests import oracle_lib

US = 1_000_000
MIN = 60 * US
HOUR = synthetic.HOUR_US
DAY = 24 * HOUR
EPOCH = dt_.datetime(1970, 1, 1)
N = 300          # cells of a case: one full 256-lane workgroup and a ragged one
N_SMALL = 70     # its first cells: one full wavefront and a ragged one


def utc(y, m, d, h=0, mi=0, s=0, us=0) -> int:
    """microseconds since 1970-01-01Z of a proleptic Gregorian UTC instant, by datetime."""
    return (dt_.datetime(y, m, d, h, mi, s, us) - EPOCH) // dt_.timedelta(microseconds=1)


def when(t_us: int) -> dt_.datetime:
    return EPOCH + dt_.timedelta(microseconds=int(t_us))


def day_of_year(t_us: int) -> int:
    return when(t_us).timetuple().tm_yday


def time_in_year_us(t_us: int) -> int:
    w = when(t_us)
    return (w - dt_.datetime(w.year, 1, 1)) // dt_.timedelta(microseconds=1)


AXES = (
    ("3h_leap", utc(2016, 2, 27), 3 * HOUR, 32),
    ("24h_year_end_leap", utc(2016, 12, 28), DAY, 8),
    ("1h_year_end_pre_epoch", utc(1967, 12, 31, 12), HOUR, 24),
    ("3h_pre_epoch_leap", utc(1968, 2, 28), 3 * HOUR, 24),
    ("15min_wed", utc(2015, 4, 9, 22), 15 * MIN, 16),
    ("odd_dt", synthetic.T0_2015_US - 7 * HOUR // 2 + 12_345_678, 7 * MIN + 1, 60),
    ("24h_2100", utc(2100, 2, 27), DAY, 4),
    ("24h_2000", utc(2000, 2, 27), DAY, 4),
)
AXIS = {name: (t0, dt, T) for name, t0, dt, T in AXES}
NAMES = tuple(AXIS)
WINTER = ("3h_leap", "24h_year_end_leap", "1h_year_end_pre_epoch", "3h_pre_epoch_leap", "odd_dt", "24h_2100", "24h_2000")
# days of hourly oracle run before t0 that build the starting state. 15min_wed: the winter from New Year on. The
# late-February axes: 8 days, a pack thin enough that the thaws on the axis leave pt_ss_k cells partly covered
# (after 45 days every pack there is so deep that sca stays exactly 1)
SPINUP_DAYS = {name: 8 if when(AXIS[name][0]).month == 2 else 45 for name in NAMES}
SPINUP_DAYS["15min_wed"] = 98

# (winter_end_day_of_year, n_winter_days) of the second pt_gs_k set: the start_melt day begins inside the axis and a
# snow-season edge, (wed - nwd) * 24 h or wed * 24 h after New Year, lies strictly inside it
SECOND_SET = {
    "3h_leap": (60, 2),                 # start_melt from step 16; season [step 8, step 24)
    "24h_year_end_leap": (1, 221),      # start_melt at step 4; season ends at step 5
    "1h_year_end_pre_epoch": (1, 1),    # start_melt and season from step 12
    "3h_pre_epoch_leap": (60, 1),       # start_melt and season [step 8, step 16)
    "15min_wed": (100, 1),              # start_melt and season from step 8
    "odd_dt": (1, 1),                   # start_melt and season from step 30, the first to begin in 2015
    "24h_2100": (60, 1),                # start_melt and season: step 2
    "24h_2000": (60, 1),                # the same step, Feb 29 here
}
# winter_end_day_of_year of the first set where it is not the default 100: doy 366 exists on this axis only
FIRST_SET_WED = {"24h_year_end_leap": 366}
PK_C1, PK_SNOW_CV, PK_CV_FOREST, PK_CV_ALT, PK_WED, PK_ISO, PK_NWD = 0, 14, 17, 18, 22, 23, 28


def times(name, shift_us=0, dt_us=None):
    t0, dt, T = AXIS[name]
    dt = dt if dt_us is None else dt_us
    return [t0 + shift_us + i * dt for i in range(T)]


def _hours_of_year(ts):
    return np.array([time_in_year_us(t) // HOUR % 8760 for t in ts], dtype=np.int64)


def forcing_at(n, ts, z=None):
    """[5][len(ts)][n]: the synthetic hourly year at each instant's hour of the year, modulo 8760."""
    hours = _hours_of_year(ts)
    uniq = np.unique(hours)
    rows = {}
    start = 0
    for k in range(1, len(uniq) + 1):  # one generator call per run of consecutive hours
        if k == len(uniq) or uniq[k] != uniq[k - 1] + 1:
            f = synthetic.forcing(n, int(uniq[start]), k - start, z=z)
            for j in range(start, k):
                rows[int(uniq[j])] = f[:, j - start]
            start = k
    return np.ascontiguousarray(np.stack([rows[int(h)] for h in hours], axis=1))


def ptgsk_geo(n=N):
    return synthetic.geo11(N)[:n]


def ptssk_geo(n=N):
    """glacier, lake and reservoir fractions as tests/test_ptssk_parity.py::_case draws them."""
    geo = synthetic.geo11(N, n_catchments=4)
    rng = np.random.default_rng(5)
    geo[:, 6] = rng.choice([0.0, 0.05, 0.3], N)
    geo[:, 7] = rng.choice([0.0, 0.05], N)
    geo[:, 8] = rng.choice([0.0, 0.19], N)
    geo[:, 10] = 1.0 - geo[:, 6:10].sum(axis=1)
    return geo[:n]


def set_ix(n=N):
    return (np.arange(n) % 3 == 0).astype(np.int32)


def ptgsk_sets(name):
    """[2][31]: the default set (on 24h_year_end_leap with winter_end_day_of_year 366) and the second one."""
    p0 = synthetic.default_ptgsk_parameters()
    p0[PK_WED] = FIRST_SET_WED.get(name, p0[PK_WED])
    p1 = synthetic.default_ptgsk_parameters()
    p1[PK_C1] = -2.2
    p1[PK_SNOW_CV] = 0.6
    p1[PK_CV_FOREST] = 0.1
    p1[PK_CV_ALT] = 1e-4
    p1[PK_ISO] = 1.0
    p1[PK_WED], p1[PK_NWD] = SECOND_SET[name]
    return np.stack([p0, p1])


def ptssk_sets():
    p0 = synthetic.default_ptssk_parameters()
    p1 = p0.copy()
    p1[9] = 3.5     # ss.cx
    return np.stack([p0, p1])


def _frozen(a):
    a.setflags(write=False)
    return a


def _spinup(stack, name, geo):
    t0, _, _ = AXIS[name]
    n_steps = SPINUP_DAYS[name] * 24
    ts = [t0 - (n_steps - i) * HOUR for i in range(n_steps)]
    f = forcing_at(N, ts, z=geo[:, 2])
    if stack == "pt_gs_k":
        return oracle_lib.ptgsk_run(geo, synthetic.default_ptgsk_parameters(), synthetic.default_ptgsk_state(N), ts[0],
                                    HOUR, f)["state"]
    return oracle_lib.ptssk_run(geo, synthetic.default_ptssk_parameters(), synthetic.default_ptssk_state(N), ts[0], HOUR,
                                f)["state"]


@functools.lru_cache(maxsize=None)
def case(stack, name):
    """The N-cell inputs of a stack on an axis: geo [N][11], forcing [5][T][N], params [2][*], set_ix [N],
    state [N][*]; a launch on fewer cells takes their first rows."""
    geo = ptgsk_geo() if stack == "pt_gs_k" else ptssk_geo()
    return {"geo": _frozen(geo), "forcing": _frozen(forcing_at(N, times(name), z=geo[:, 2])),
            "params": _frozen(ptgsk_sets(name) if stack == "pt_gs_k" else ptssk_sets()), "set_ix": _frozen(set_ix()),
            "state": _frozen(_spinup(stack, name, geo))}


def inputs(stack, name, which="both", n=N):
    """(geo, params, set_ix or None, state, forcing) of a launch: `which` is 'both' (per-cell sets) or 0 / 1 (that
    set alone: the uniform-parameter launch)."""
    c = case(stack, name)
    p, ix = (c["params"], c["set_ix"][:n]) if which == "both" else (c["params"][which:which + 1], None)
    return c["geo"][:n], p, ix, c["state"][:n], np.ascontiguousarray(c["forcing"][:, :, :n])


@functools.lru_cache(maxsize=None)
def oracle(stack, name, which="both", n=N, shift_us=0, dt_us=None, start_step=0, n_steps=0):
    """The oracle's full run (every response series, the state series, the end state) of inputs(...), on the axis
    or on it moved by shift_us / stepped by dt_us with the same forcing."""
    t0, dt, _ = AXIS[name]
    geo, p, ix, st, f = inputs(stack, name, which, n)
    run = oracle_lib.ptgsk_run if stack == "pt_gs_k" else oracle_lib.ptssk_run
    r = run(geo, p, st, t0 + shift_us, dt if dt_us is None else dt_us, f, start_step, n_steps, ix, full=True,
            collect_state=True)
    return {k: _frozen(r[k]) for k in ("full", "state_series", "state")}
