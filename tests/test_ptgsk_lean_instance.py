"""The lean (discharge-only) instance of the pt_gs_k run kernel against the general one and the oracle.

launch_ptgsk_run (kernels/ptgsk.hip) sends a launch with collect == 0, no state series and read_delay == 0 to an
instance compiled without the code and pointers for response series 2-7, the state series and the delay knob (the
256-lane 4-wave kernel and the 64-lane small-region kernel each have one, for uniform and for per-cell parameters);
every other combination takes the general instance. Both run the same step, so every case here is bit-for-bit the
oracle's, and the discharge-only runs equal the same series of the collect-all run.

The region is 300 cells of the synthetic 1M-cell region: one full 256-lane workgroup and one with 212 out-of-range
lanes. 720 hourly steps from Jan 1 use the Brent job queue, the carry and the lgamma cache. The catchment ids are
rewritten in runs of 50 cells, so that a catchment filter or a parameter override covers part of a wavefront."""
import functools

import numpy as np
import pytest

from shyft_amd import synthetic

pytestmark = pytest.mark.gpu

N, T = 300, 720
ODD_STEP0 = 1


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


@functools.lru_cache(maxsize=None)
def _oracle(override=False, step0=0):
    from tests import oracle_lib
    p, ix = _params(override)
    return oracle_lib.ptgsk_run(_geo(), p, synthetic.default_ptgsk_state(N), synthetic.T0_2015_US, synthetic.HOUR_US,
                                synthetic.forcing(N, 0, T), start_step=step0, n_steps=T - step0, set_ix=ix, full=True,
                                collect_state=True)


@functools.lru_cache(maxsize=None)
def _hip(collect, state_series=False, cids=None, override=False, delay=0, step0=0, instance=4):
    """{'series' [2 | 4 | 8][T][N], 'state' [N][9], 'state_series' [9][T+1][N] or None} of one run."""
    from shyft_amd.region import HipRegion, PT_GS_K, KNOB_PTGSK_INSTANCE, KNOB_BRENT_READ_DELAY
    p, ix = _params(override)
    f = synthetic.forcing(N, 0, T)
    r = HipRegion(PT_GS_K, N, device=0)
    try:
        r.set_geo(_geo())
        r.set_parameters(p, ix)
        r.set_time_axis(synthetic.T0_2015_US, synthetic.HOUR_US, T)
        r.set_collection(collect, state_series)
        r.set_state(synthetic.default_ptgsk_state(N))
        if cids is not None:
            r.set_catchment_filter(list(cids))
        r.set_test_knob(KNOB_PTGSK_INSTANCE, instance)
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


def _check_lean_vs_general(lean, general, step0=0, on=slice(None)):
    assert _same(lean["series"][:, step0:, on], general["series"][:2, step0:, on])
    assert np.array_equal(lean["state"][on], general["state"][on])


@pytest.mark.parametrize("state_series", [False, True])
@pytest.mark.parametrize("collect", [0, 1, 2])
def test_collect_modes_equal_oracle(collect, state_series):
    g = _hip(collect, state_series)
    _check_oracle(g, _oracle())
    if collect == 2:
        assert (g["series"][3] > 0).any()   # a snow pack: the window has Brent jobs


@pytest.mark.parametrize("state_series", [False, True])
def test_discharge_only_equals_collect_all(state_series):
    _check_lean_vs_general(_hip(0, state_series), _hip(2, state_series))
    _check_lean_vs_general(_hip(0, False), _hip(2, True))


def test_odd_first_step():
    """step0 odd: the first step uses the second of the double-buffered job counters."""
    lean, general = _hip(0, step0=ODD_STEP0), _hip(2, step0=ODD_STEP0)
    o = _oracle(step0=ODD_STEP0)
    _check_oracle(lean, o, ODD_STEP0)
    _check_oracle(general, o, ODD_STEP0)
    _check_lean_vs_general(lean, general, ODD_STEP0)


def test_catchment_filter_part_of_a_wavefront():
    """Catchments 1 and 3 only: lanes 50-99, 200-249 are off, inside the first, second and fourth wavefronts."""
    on = np.isin(_geo()[:, 4], (1, 3))
    assert 0 < on[:64].sum() < 64 and 0 < on[64:128].sum() < 64
    lean, general = _hip(0, cids=(1, 3)), _hip(2, cids=(1, 3))
    _check_oracle(lean, _oracle(), on=on)
    _check_oracle(general, _oracle(), on=on)
    _check_lean_vs_general(lean, general, on=on)
    # the cells switched off keep their state
    assert np.array_equal(lean["state"][~on], synthetic.default_ptgsk_state(N)[~on])
    assert np.array_equal(general["state"][~on], synthetic.default_ptgsk_state(N)[~on])


def test_catchment_parameter_override():
    """A second parameter set for catchment 2: the per-cell parameter instances, lean and general."""
    lean, general = _hip(0, override=True), _hip(2, override=True)
    o = _oracle(override=True)
    _check_oracle(lean, o)
    _check_oracle(general, o)
    _check_lean_vs_general(lean, general)
    assert not _same(o["full"][0], _oracle()["full"][0])   # the override changes the discharge


def test_read_delay_takes_the_general_instance_and_agrees():
    """read_delay 3 with collect == 0 is not a lean launch (the lean instance has no knob code); same bits."""
    g = _hip(0, delay=3)
    _check_oracle(g, _oracle())
    _check_lean_vs_general(g, _hip(2))
    _check_lean_vs_general(_hip(0), g)


def test_small_region_instance():
    """The 64-lane instance (knob 2) has a lean variant too: discharge-only against collect-all and the oracle."""
    lean, general = _hip(0, instance=2), _hip(2, instance=2)
    _check_oracle(lean, _oracle())
    _check_oracle(general, _oracle())
    _check_lean_vs_general(lean, general)
    lean, general = _hip(0, override=True, instance=2), _hip(2, override=True, instance=2)
    _check_oracle(lean, _oracle(override=True))
    _check_lean_vs_general(lean, general)
