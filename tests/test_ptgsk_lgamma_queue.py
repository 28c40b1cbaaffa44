"""The lgamma queue of the 256-lane pt_gs_k run kernel against the oracle, bit for bit.

A lane whose snow-distribution shape (the state's alpha) changes in a step needs a new dlgamma(shape) for the step's
final calc_snow_state. gs_front knows that shape before the Brent result (only lwc depends on it), so the 256-lane
instances queue the new shapes of a workgroup-step in LDS and the wavefronts that are not solving Brent jobs evaluate
them, compacted, between the step's two barriers; the owner's lgamma cache slot then hits in gs_back
(kernels/ptgsk.hip). The arithmetic is the same function of the same argument, so every case here is
the oracle's bits: series, final state and state series.

The region is 300 cells of the synthetic 1M-cell region (one full 256-lane workgroup and one with 212 out-of-range
lanes), the catchment ids rewritten in runs of 50 cells. Two windows of 720 hourly steps from the default state:
January (time axis from Jan 1) and autumn (time axis from hour 6,900, mid-October: packs form, melt out and reset).
lgamma_events() below replays the lgamma cache on the oracle's state series, on the CPU, and the module asserts from
it that the windows hold every kind of workgroup-step the queue distinguishes before any GPU result is looked at.
tools/ptgsk_lgamma_count.py prints the same tallies by season."""
import functools

import numpy as np
import pytest

from shyft_amd import synthetic

pytestmark = pytest.mark.gpu

N, T = 300, 720
BLOCK = 256
ODD_STEP0 = 1
WINDOWS = {"jan": 0, "autumn": 6900}   # first hour of the time axis, counted from 2015-01-01
GS_TOL = 1.0e-10
SSF = 1.0 - 0.05 - 0.19                # snow_storage_fraction of synthetic.geo11 (1 - lake - reservoir)


def _geo():
    g = synthetic.geo11(N, n_total=1 << 20)
    g[:, 4] = 1 + (np.arange(N) // 50) % 3   # catchments 1, 2, 3 in runs of 50 cells
    return g


def _params(override):
    p = synthetic.default_ptgsk_parameters()
    if not override:
        return p.reshape(1, -1), None
    p2 = p.copy()
    p2[0:3] = (-2.2, 0.9, -0.08)   # kirchner c1 c2 c3
    p2[4] = -0.2                   # gs.tx
    p2[16] = 1.1                   # p_corr.scale_factor
    return np.stack([p, p2]), (_geo()[:, 4] == 2).astype(np.int32)   # catchment 2 takes the second set


def _t0(window):
    return synthetic.T0_2015_US + WINDOWS[window] * synthetic.HOUR_US


def _forcing(window):
    return synthetic.forcing(N, WINDOWS[window], T)


@functools.lru_cache(maxsize=None)
def _oracle(window="jan", override=False, step0=0):
    from tests import oracle_lib
    p, ix = _params(override)
    return oracle_lib.ptgsk_run(_geo(), p, synthetic.default_ptgsk_state(N), _t0(window), synthetic.HOUR_US,
                                _forcing(window), start_step=step0, n_steps=T - step0, set_ix=ix, full=True,
                                collect_state=True)


def lgamma_events(state_series, temp, prec_mm_h, p, hour0=0, block=BLOCK):
    """Replay of the kernel's per-lane lgamma cache on an oracle state series [9][T+1][n] (gamma_snow.h:291-493 as
    device/ptgsk_dev.h splits it), uniform parameters p, cell constants of synthetic.geo11 (snow_cv factors 0).

    Returns per step and cell, bool [T][n]:
      job       the step has a corr_lwc Brent job (its lane evaluates lgamma(a2) in gs_front)
      front     gs_front's opening calc_snow_state evaluates a new lgamma (no carry from the step before)
      job_new   the job's lgamma(a2) is a new evaluation
      back      gs_back's final calc_snow_state evaluates a new lgamma: the shapes the queue is for
      again     such a shape was set in gs_back (melt update or reset), after gs_front's snowfall update or not
      melt, reset_shape, cold   what made a `back` shape new: the melt update, the reset value 1 / snow_cv^2 met
                later, or a shape unchanged in the step that the cache does not hold (the first step)
      uses      gs_back's final calc_snow_state uses lgamma at all (cache hits included)
    and the tallies per workgroup-step [T][ceil(n / block)]: n_job, n_back."""
    ss = np.asarray(state_series)
    nT, n = ss.shape[1] - 1, ss.shape[2]
    tx, max_water, ibgf, p_corr, wed = p[4], p[6], p[21], p[16], int(p[22])
    cv2 = p[14] * p[14]
    inv_cv2_param = 1.0 / cv2

    def uses(shape, smm, lam, lwd):
        with np.errstate(all="ignore"):
            scale = smm / shape
            early = (lam > 0.0) & (lam / scale > 1.3 * shape + 20.0)
            first = (lam > 0.0) & ~early
            second = ~early & (lwd > 0.0) & ~(lwd > shape * scale)
        return first | second

    names = ("job", "front", "job_new", "back", "again", "melt", "reset_shape", "cold", "uses")
    ev = {k: np.zeros((nT, n), dtype=bool) for k in names}
    key = np.full(n, -1.0)
    carry_ok = np.zeros(n, dtype=bool)
    for i in range(nT):
        alpha, smm, acc = ss[4, i], ss[5, i], ss[6, i].copy()
        lwc = ss[2, i] / SSF
        if ((hour0 + i) // 24) % 365 + 1 == wed:   # start_melt
            acc[:] = 0.0
            carry_ok[:] = False
        prec = (prec_mm_h[i] * p_corr * 3600000000.0) / 3600000000.0
        snow = np.where(temp[i] < tx, prec, 0.0)
        done = (snow < GS_TOL) & (smm < GS_TOL) & (acc < 0.0)
        # gs_front's opening calc_snow_state
        f = ~done & ~carry_ok & uses(alpha, smm, acc, lwc) & (key != alpha)
        ev["front"][i] = f
        key = np.where(f, alpha, key)
        # the snowfall update and the Brent job
        upd = ~done & (acc < 0.0) & ~(snow < GS_TOL)
        sdc_snow = snow / (1.0 - ibgf)
        with np.errstate(all="ignore"):
            a2 = np.where(upd, (smm * alpha + sdc_snow / cv2) / (sdc_snow + smm), alpha)
        smm_front = np.where(upd, smm + sdc_snow, smm)
        job = upd & (lwc > 0.0) & (sdc_snow > 0.01 * smm)
        ev["job"][i] = job
        ev["job_new"][i] = job & (key != a2)
        key = np.where(job, a2, key)
        # gs_back's final calc_snow_state
        alpha1, smm1, acc1 = ss[4, i + 1], ss[5, i + 1], ss[6, i + 1]
        u = ~done & uses(alpha1, smm1, acc1, ss[2, i + 1] / SSF)
        b = u & (key != alpha1)
        changed = ~done & (smm1 != smm_front)   # the melt update or a reset moved sdc_melt_mean in gs_back
        ev["uses"][i] = u
        ev["back"][i] = b
        ev["again"][i] = b & changed
        ev["reset_shape"][i] = b & (alpha1 == inv_cv2_param)
        ev["melt"][i] = b & changed & ~ev["reset_shape"][i]
        ev["cold"][i] = b & ~changed & ~upd & ~ev["reset_shape"][i]
        key = np.where(u, alpha1, key)
        carry_ok = ~done
    nwg = (n + block - 1) // block
    pad = nwg * block - n
    for k in ("job", "back"):
        ev["n_" + k] = np.pad(ev[k], ((0, 0), (0, pad))).reshape(nT, nwg, block).sum(axis=2)
    return ev


@functools.lru_cache(maxsize=None)
def _events(window):
    f = _forcing(window)
    return lgamma_events(_oracle(window)["state_series"], f[0], f[1], synthetic.default_ptgsk_parameters(),
                         hour0=WINDOWS[window])


@functools.lru_cache(maxsize=None)
def _hip(window, collect, state_series=False, cids=None, override=False, delay=0, step0=0):
    """{'series' [2 | 4 | 8][T][N], 'state' [N][9], 'state_series' [9][T+1][N] or None} of one run of the 256-lane
    instance."""
    from shyft_amd.region import HipRegion, PT_GS_K, KNOB_PTGSK_INSTANCE, KNOB_BRENT_READ_DELAY
    p, ix = _params(override)
    f = _forcing(window)
    r = HipRegion(PT_GS_K, N, device=0)
    try:
        r.set_geo(_geo())
        r.set_parameters(p, ix)
        r.set_time_axis(_t0(window), synthetic.HOUR_US, T)
        r.set_collection(collect, state_series)
        r.set_state(synthetic.default_ptgsk_state(N))
        if cids is not None:
            r.set_catchment_filter(list(cids))
        r.set_test_knob(KNOB_PTGSK_INSTANCE, 4)
        r.set_test_knob(KNOB_BRENT_READ_DELAY, delay)
        for v in range(5):
            r.set_forcing(v, 0, f[v])
        r.run_cells(0, step0, T - step0)
        ns = (2, 4, 8)[collect]
        return {"series": np.stack([r.get_series(k, 0, T) for k in range(ns)]), "state": r.get_state(),
                "state_series": np.stack([r.get_state_series(k, 0, T + 1) for k in range(9)]) if state_series else None}
    finally:
        r.close()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _check_oracle(g, o, step0=0, on=slice(None)):
    ns = g["series"].shape[0]
    assert _same(g["series"][:, step0:, on], o["full"][:ns, step0:, on])
    assert np.array_equal(g["state"][on], o["state"][on])
    if g["state_series"] is not None:
        assert _same(g["state_series"][:, step0:, on], o["state_series"][:, step0:, on])


def _kinds(ev):
    nb, nj = ev["n_back"], ev["n_job"]
    return {"with_brent": int(((nb > 0) & (nj > 0)).sum()), "without_brent": int(((nb > 0) & (nj == 0)).sum()),
            "over_64": int((nb > 64).sum()), "again": int(ev["again"].sum())}


@functools.lru_cache(maxsize=None)
def _assert_windows():
    """From the oracle alone: the two windows together contain workgroup-steps with new shapes and Brent jobs, with
    new shapes and no Brent job, with more than 64 new shapes (more than one helper pass of a wavefront), and shapes
    that gs_back changed again after gs_front's snowfall update (melt, reset); each window has new shapes at all."""
    k = {w: _kinds(_events(w)) for w in WINDOWS}
    print(k)
    for w in WINDOWS:
        assert k[w]["with_brent"] + k[w]["without_brent"] > 0
    for kind in ("with_brent", "without_brent", "over_64", "again"):
        assert sum(k[w][kind] for w in WINDOWS) > 0, kind
    # the autumn window: packs form, melt out and reset
    ss = _oracle("autumn")["state_series"]
    formed = (ss[5] > 0).any(axis=0)
    assert (formed & (ss[5, -1] == 0.0)).any()
    # shapes changed in gs_back in a step that also had the snowfall update and a Brent job: the job lane's cache
    # holds lgamma(a2) and the step's final shape is another one
    assert sum(int((_events(w)["again"] & _events(w)["job"]).sum()) for w in WINDOWS) > 0


@pytest.fixture(scope="module", autouse=True)
def windows_checked():
    """Before any GPU result is compared: the windows exercise what the tests are about."""
    _assert_windows()


def test_windows_hold_every_kind_of_workgroup_step():
    _assert_windows()


@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_lean_instance_equals_oracle(window):
    """collect 0: the lean 256-lane instance."""
    _check_oracle(_hip(window, 0), _oracle(window))


@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_general_instance_with_state_series_equals_oracle(window):
    """collect 2 and the state series: the general 256-lane instance."""
    g = _hip(window, 2, True)
    _check_oracle(g, _oracle(window))
    assert (g["series"][3] > 0).any()   # a snow pack


@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_odd_first_step(window):
    """step0 odd: the first step uses the second of the double-buffered counters (Brent jobs and shapes)."""
    o = _oracle(window, step0=ODD_STEP0)
    _check_oracle(_hip(window, 0, step0=ODD_STEP0), o, ODD_STEP0)
    _check_oracle(_hip(window, 2, True, step0=ODD_STEP0), o, ODD_STEP0)


@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_catchment_filter_part_of_a_wavefront(window):
    """Catchments 1 and 3 only: lanes 50-99 and 200-249 are off, inside the first, second and fourth wavefronts. They
    queue nothing and receive nothing (they still help), and their state stays as it was set."""
    on = np.isin(_geo()[:, 4], (1, 3))
    assert 0 < on[:64].sum() < 64 and 0 < on[64:128].sum() < 64
    for g in (_hip(window, 0, cids=(1, 3)), _hip(window, 2, True, cids=(1, 3))):
        _check_oracle(g, _oracle(window), on=on)
        assert np.array_equal(g["state"][~on], synthetic.default_ptgsk_state(N)[~on])


@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_catchment_parameter_override(window):
    """A second parameter set for catchment 2: the per-cell parameter instances, lean and general."""
    o = _oracle(window, override=True)
    _check_oracle(_hip(window, 0, override=True), o)
    _check_oracle(_hip(window, 2, True, override=True), o)
    assert not _same(o["full"][0], _oracle(window)["full"][0])   # the override changes the discharge


@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_late_readers(window):
    """read_delay 3 (general instance): three wavefronts read their Brent results and cache slots late, while the
    first is already queueing the next step's jobs and shapes."""
    _check_oracle(_hip(window, 0, delay=3), _oracle(window))
    _check_oracle(_hip(window, 2, True, delay=3), _oracle(window))
