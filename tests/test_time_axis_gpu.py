"""pt_gs_k and pt_ss_k off the hourly 2015 time axis: the HIP kernels and the host code that feeds them (the
dt-derived parameter columns, the day-of-year and time-in-year tables) against the CPU oracle, bit for bit, on the
axes of tests/time_axis_cases.py: sub-hourly, 3 h and 24 h steps, a step of 7 min + 1 us, leap days, doy 366, the
wrap at New Year, times before 1970 and the century rule. tests/test_time_axis_host.py asserts on the oracle alone that
each case reaches its event (a start_melt day and a snow-season edge inside the axis, Brent jobs, partial snow cover)
and that both the calendar and dt change the result. No tolerance anywhere; a failure names the axis, the series,
the first differing step and cell, and both values."""
import numpy as np
import pytest

from tests import oracle_lib
from tests import time_axis_cases as tc

pytestmark = pytest.mark.gpu

STACK_ID = {"pt_gs_k": 1, "pt_ss_k": 3}
N_STATE_SERIES = {"pt_gs_k": 9, "pt_ss_k": 7}


def _assert_bitexact(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        i = tuple(int(v) for v in np.argwhere(~same)[0])
        where = {3: "(series, step, cell)", 2: "(step, cell) / (cell, field)"}.get(got.ndim, "index")
        raise AssertionError(f"{what}: {int((~same).sum())} values differ; first at {where} {i}: "
                             f"gpu {got[i]!r} oracle {want[i]!r}")


def _load(r, stack, name, which, n, full=True, state_series=True, axis=None):
    """geo, parameters, the time axis, collection, state and forcing of a case into region r"""
    from shyft_amd.region import COLLECT_ALL, COLLECT_DISCHARGE
    t0, dt, T = tc.AXIS[name] if axis is None else axis
    geo, p, ix, st, f = tc.inputs(stack, name, which, n)
    r.set_geo(geo)
    r.set_parameters(p, ix)
    r.set_time_axis(t0, dt, T)
    r.set_collection(COLLECT_ALL if full else COLLECT_DISCHARGE, state_series)
    r.set_state(st)
    for v in range(5):
        r.set_forcing(v, 0, f[v])


def _read(r, stack, T, full=True, state_series=True):
    out = {"full": np.stack([r.get_series(k, 0, T) for k in range(8 if full else 2)]), "state": r.get_state()}
    if state_series:
        out["state_series"] = np.stack([r.get_state_series(k, 0, T + 1) for k in range(N_STATE_SERIES[stack])])
    return out


def _hip(stack, name, which="both", n=tc.N, full=True, state_series=True, instance=0, start_step=0, n_steps=0,
         single_steps=False, devices=None):
    from shyft_amd.region import HipRegion, KNOB_PTGSK_INSTANCE
    T = tc.AXIS[name][2]
    r = HipRegion(STACK_ID[stack], n, devices=devices)
    try:
        _load(r, stack, name, which, n, full, state_series)
        if instance:
            r.set_test_knob(KNOB_PTGSK_INSTANCE, instance)
        if single_steps:
            for i in range(start_step, start_step + n_steps):
                r.run_cells(0, i, 1)
        else:
            r.run_cells(0, start_step, n_steps)
        return _read(r, stack, T, full, state_series)
    finally:
        r.close()


def _check(got, want, what, steps=slice(None), lean=False):
    """every collected response series, the state-collector series (where collected) and the end state"""
    _assert_bitexact(got["full"][:, steps], want["full"][:2 if lean else 8, steps], f"{what}: response series")
    if "state_series" in got:
        _assert_bitexact(got["state_series"], want["state_series"], f"{what}: state series")
    _assert_bitexact(got["state"], want["state"], f"{what}: end state")


# ---- pt_ss_k: the two instances of launch_ptssk_run on every axis ----

@pytest.mark.parametrize("name", tc.NAMES)
def test_ptssk_every_axis_bitexact(name):
    for which in ("both", 0):  # per-lane parameter sets; one uniform set
        got = _hip("pt_ss_k", name, which)
        _check(got, tc.oracle("pt_ss_k", name, which), f"pt_ss_k {name} sets={which}")


# ---- pt_gs_k: every axis x the launch instances of launch_ptgsk_run ----

@pytest.mark.parametrize("instance,n", [(2, tc.N_SMALL), (4, tc.N)])
@pytest.mark.parametrize("name", tc.NAMES)
def test_ptgsk_every_axis_and_launch_instance_bitexact(name, instance, n):
    """KNOB_PTGSK_INSTANCE 2 on 70 cells (a full wavefront and a ragged one) and 4 on 300 (a full 256-lane workgroup
    and a ragged one); the general kernel (COLLECT_ALL with state series) and the lean one (COLLECT_DISCHARGE without:
    discharge, charge and the end state); per-lane parameter sets and each set alone (the uniform launch)."""
    for which in ("both", 0, 1):
        want = tc.oracle("pt_gs_k", name, which, n)
        what = f"pt_gs_k {name} instance {instance} n={n} sets={which}"
        _check(_hip("pt_gs_k", name, which, n, instance=instance), want, what + " general")
        lean = _hip("pt_gs_k", name, which, n, full=False, state_series=False, instance=instance)
        _check(lean, want, what + " lean", lean=True)


# ---- run_cells one step at a time from an odd step ----

@pytest.mark.parametrize("name", ["3h_leap", "24h_year_end_leap"])
@pytest.mark.parametrize("stack", ["pt_gs_k", "pt_ss_k"])
def test_stepwise_from_an_odd_step_equals_the_single_run_and_the_oracle(stack, name):
    T = tc.AXIS[name][2]
    start, n_steps = 1, T - 1
    want = tc.oracle(stack, name, "both", tc.N, start_step=start, n_steps=n_steps)
    steps = slice(start, T)
    single = _hip(stack, name, state_series=False, start_step=start, n_steps=n_steps)
    stepwise = _hip(stack, name, state_series=False, start_step=start, n_steps=n_steps, single_steps=True)
    _check(single, want, f"{stack} {name} steps [1, T) in one run", steps)
    _check(stepwise, want, f"{stack} {name} steps [1, T) one at a time", steps)
    _assert_bitexact(stepwise["full"][:, steps], single["full"][:, steps], f"{stack} {name}: stepwise vs single run")


# ---- a live region changes its axis ----

@pytest.mark.parametrize("stack,name", [("pt_gs_k", "3h_leap"), ("pt_ss_k", "24h_2100")])
def test_live_region_takes_a_new_axis(stack, name):
    """A region that has run on an hourly axis gets the case's axis by set_time_axis, then state and forcing, and
    runs: the same bits as a fresh region on that axis and as the oracle. The dt-derived parameter columns and the
    doy / time-in-year tables are rebuilt."""
    from shyft_amd import synthetic
    from shyft_amd.region import HipRegion
    T = tc.AXIS[name][2]
    fresh = _hip(stack, name)
    r = HipRegion(STACK_ID[stack], tc.N)
    try:
        _load(r, stack, name, "both", tc.N, axis=(synthetic.T0_2015_US, tc.HOUR, T))
        r.run_cells(0, 0, 0)
        hourly = _read(r, stack, T)
        # geo and parameters stay as they are: only the axis, the state and the forcing are set again
        t0, dt, _ = tc.AXIS[name]
        _, _, _, st, f = tc.inputs(stack, name)
        r.set_time_axis(t0, dt, T)
        r.set_state(st)
        for v in range(5):
            r.set_forcing(v, 0, f[v])
        r.run_cells(0, 0, 0)
        got = _read(r, stack, T)
    finally:
        r.close()
    assert not np.array_equal(hourly["full"][0], got["full"][0])
    _check(got, fresh, f"{stack} {name}: live region against a fresh one")
    _check(got, tc.oracle(stack, name), f"{stack} {name}: live region")


# ---- the ensemble's member region inherits dt and both calendar tables ----

def test_ensemble_members_with_their_own_winter_end_day():
    """ensemble_run on 3h_leap with 3 members whose winter_end_day_of_year is 59, 60 and 61 (each begins inside the
    axis), compared as tests/test_ensemble.py::_check does: the catchment sums of discharge and charge of member m
    equal, bit for bit, those of the region run alone with member m's parameters from the same state; the
    area-weighted snow-cover sums are within 1e-13 relative of the host's sum of the per-cell series."""
    from shyft_amd.region import COLLECT_DISCHARGE_SNOW, HipRegion, PT_GS_K
    name, n, n_members = "3h_leap", tc.N, 3
    t0, dt, T = tc.AXIS[name]
    geo, p, _, st, f = tc.inputs("pt_gs_k", name, 1)
    geo = geo.copy()
    geo[:, 4] = 1 + (np.arange(n) * 5) // n
    members = np.tile(p, (n_members, 1))
    members[:, tc.PK_WED] = (59, 60, 61)
    r = HipRegion(PT_GS_K, n)
    try:
        r.set_geo(geo)
        r.set_parameters(p)
        r.set_time_axis(t0, dt, T)
        r.set_collection(COLLECT_DISCHARGE_SNOW)
        r.set_state(st)
        for v in range(5):
            r.set_forcing(v, 0, f[v])
        s0 = r.get_state().copy()
        r.ensemble_run(members, 0, 0, COLLECT_DISCHARGE_SNOW)
        assert np.array_equal(r.get_state(), s0), "ensemble run modified the region state"
        q = r.ensemble_sums(0, 0, T)
        charge = r.ensemble_sums(1, 0, T)
        sca_w = r.ensemble_sums(2, 0, T, area_weighted=True)
        cids = r.catchment_ids()
        area, cell_cid = geo[:, 3], geo[:, 4].astype(np.int64)
        for m in range(n_members):
            r.set_parameters(members[m:m + 1])
            r.set_state(s0)
            r.run_cells(0, 0, 0)
            _assert_bitexact(q[m], r.catchment_sums(0, 0, T), f"member {m}: discharge sums")
            _assert_bitexact(charge[m], r.catchment_sums(1, 0, T), f"member {m}: charge sums")
            sca = r.get_series(2, 0, T)
            for c, cid in enumerate(cids):
                sel = cell_cid == cid
                np.testing.assert_allclose(sca_w[m, c], (sca[:, sel] * area[sel]).sum(axis=1), rtol=1e-13, atol=1e-9)
            # member m alone is the oracle's run with its parameters
            want = oracle_lib.ptgsk_run(geo, members[m], st, t0, dt, f, full=True)
            _assert_bitexact(r.get_series(0, 0, T), want["full"][0], f"member {m}: discharge against the oracle")
        assert not np.array_equal(q[0], q[1]) and not np.array_equal(q[1], q[2])
    finally:
        r.close()


# ---- a sharded region hands dt and the axis to every shard ----

@pytest.mark.parametrize("stack", ["pt_gs_k", "pt_ss_k"])
def test_two_shards_on_the_year_end_axis_equal_unsharded(stack):
    name = "24h_year_end_leap"
    ref = _hip(stack, name)
    sh = _hip(stack, name, devices=[0, 0])
    _check(sh, ref, f"{stack} {name}: 2 shards against the unsharded region")
    _check(sh, tc.oracle(stack, name), f"{stack} {name}: 2 shards")


# ---- the Python API on a 3 h axis ----

def test_api_model_on_a_3h_axis_in_2016_equals_the_region():
    """A pt_gs_k model through shyft_amd.api on a TimeAxis of 3 h steps from 2016-02-27 (across Feb 29), in frost so
    that the snow routine runs: its discharge equals the direct HipRegion run on the model's interpolated forcing."""
    from shyft_amd import api
    from shyft_amd.api import pt_gs_k
    from shyft_amd.region import COLLECT_DISCHARGE, HipRegion, PT_GS_K
    from tests.test_api_region_model import build_model, constant_source, interpolation_parameter
    n, T = 20, 32
    model = build_model(pt_gs_k.PTGSKModel, pt_gs_k.PTGSKParameter, n)
    ta = api.TimeAxisFixedDeltaT(api.Calendar().time(2016, 2, 27, 0, 0, 0), api.deltahours(3), T)
    assert ta.start * 10**6 == tc.AXIS["3h_leap"][0]
    period = api.UtcPeriod(*ta.total_period())
    gp = model.get_cells()[n // 2].geo.mid_point()
    env = api.ARegionEnvironment()
    env.precipitation.append(constant_source(api.PrecipitationSource, gp, period, 1.5))
    env.temperature.append(constant_source(api.TemperatureSource, gp, period, -0.6))
    env.wind_speed.append(constant_source(api.WindSpeedSource, gp, period, 2.0))
    env.rel_hum.append(constant_source(api.RelHumSource, gp, period, 0.7))
    env.radiation = api.RadiationSourceVector()
    env.radiation.append(constant_source(api.RadiationSource, gp, period, 100.0))
    model.initialize_cell_environment(ta)
    model.interpolate(interpolation_parameter(), env)
    s0 = pt_gs_k.PTGSKStateVector()
    for _ in range(n):
        si = pt_gs_k.PTGSKState()
        si.kirchner.q = 2.0
        s0.append(si)
    model.set_states(s0)
    model.run_cells()
    cids = api.IntVector()
    q = model.statistics.discharge(cids).values.to_numpy()
    assert q.shape == (T,) and np.isfinite(q).all()
    assert model.gamma_snow_response.sca(cids).values.to_numpy().max() > 0.0
    r = HipRegion(PT_GS_K, n)
    try:
        geo = np.zeros((n, 11))
        for i in range(n):
            geo[i] = [500 + 1000.0 * i, 500.0, 500.0 * i / n, 1e6, 1, 0.9, 0.01, 0.05, 0.19, 0.30, 0.45]
        r.set_geo(geo)
        r.set_parameters(np.array(pt_gs_k.PTGSKParameter().to_vector()))
        r.set_time_axis(ta.start * 10**6, 3 * tc.HOUR, T)
        r.set_collection(COLLECT_DISCHARGE)
        st = np.tile(np.array(pt_gs_k.PTGSKState().to_vector()), (n, 1))
        st[:, 8] = 2.0
        r.set_state(st)
        for v in range(5):
            r.set_forcing(v, 0, np.stack([model.cells[i].env_ts.__getattr__(api.FORCING[v]).to_numpy()
                                          for i in range(n)], axis=1))
        r.run_cells()
        cells = r.get_series(0, 0, T)
    finally:
        r.close()
    assert np.allclose(cells.sum(axis=1), q, rtol=1e-13, atol=0)


# ---- what set_time_axis refuses (include/shyft_hip.h) ----

def test_set_time_axis_refuses_what_the_tables_do_not_cover():
    from shyft_amd.region import HipRegion, PT_GS_K
    r = HipRegion(PT_GS_K, 4)
    try:
        for t0, dt, T in ((0, 0, 4), (0, -tc.HOUR, 4), (0, tc.HOUR, 0)):
            with pytest.raises(RuntimeError, match="invalid time_axis"):
                r.set_time_axis(t0, dt, T)
        for t0, dt, T in ((2**62 + 1, tc.HOUR, 4), (-2**62 - 1, tc.HOUR, 4), (2**62 - 3 * tc.HOUR, tc.HOUR, 4),
                          (0, 2**62, 4)):
            with pytest.raises(RuntimeError, match="beyond"):
                r.set_time_axis(t0, dt, T)
        r.set_time_axis(2**62 - 4 * tc.HOUR, tc.HOUR, 4)      # the last step ends at the limit
        r.set_time_axis(-2**62, tc.DAY, 4)
    finally:
        r.close()
