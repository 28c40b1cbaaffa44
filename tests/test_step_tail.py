"""The part of a pt_ss_k / pt_hs_k / pt_hps_k step after the snow routine (glacier melt on the post-step sca,
Priestley-Taylor, actual evapotranspiration, kirchner, total discharge and charge), bit for bit against the oracle.

The case is the smallest that reaches every branch of that tail: 70 cells (a full wavefront and a partial one),
72 hourly steps of the synthetic melt season on a snowpack spun up from January 1st, cells with glacier fraction
0 / 0.3 / 0.9, with a lake and with a reservoir, and two parameter sets that differ in gm.direct_response,
reservoir_direct_response_fraction, dtf and ae_scale. It runs with one set (the kernels' uniform instance) and
with both assigned alternately (the per-lane instance), in each collection mode."""
import functools

import numpy as np
import pytest

from shyft_amd import synthetic
from shyft_amd.region import (COLLECT_ALL, COLLECT_DISCHARGE, COLLECT_DISCHARGE_SNOW, HipRegion, PT_HPS_K, PT_HS_K,
                              PT_SS_K)
from tests import engines, oracle_lib
from tests.test_pthsk import _assert_same

HOUR = synthetic.HOUR_US
N, T = 70, 72
STEP0 = 24 * 130  # May 11th: the highest cells still freeze, the lower ones have lost their snow
A5 = [0.0, 0.25, 0.5, 0.75, 1.0]

# stack: (id, oracle/engine runner, default parameters, default state, row indices of ae_scale, dtf,
#         gm.direct_response (None: behind the reference row) and reservoir_direct_response_fraction, state series)
STACKS = {
    "pt_ss_k": (PT_SS_K, engines.run_ptssk, synthetic.default_ptssk_parameters, synthetic.default_ptssk_state,
                3, 15, 19, 20, 7),
    "pt_hs_k": (PT_HS_K, engines.run_pthsk, synthetic.default_pthsk_parameters, synthetic.default_pthsk_state,
                3, 9, 16, 17, 19),
    "pt_hps_k": (PT_HPS_K, engines.run_pthpsk, synthetic.default_pthpsk_parameters, synthetic.default_pthpsk_state,
                 3, 16, None, 23, 36),
}
GM_DIRECT = [0.0, 0.4]


def _geo():
    rows = []
    for i in range(N):
        glacier = (0.0, 0.3, 0.9)[i % 3]
        lake = 0.2 if i % 4 == 1 and glacier < 0.9 else 0.0
        reservoir = 0.2 if i % 4 == 2 and glacier < 0.9 else 0.0
        rows.append(engines.geo_row(x=500.0 + 1000.0 * i, z=400.0 + 35.0 * i, cid=1 + i // 35, glacier=glacier,
                                    lake=lake, reservoir=reservoir))
    return np.stack(rows)


def _params(name):
    _, _, defaults, _, k_ae, k_dtf, k_gm, k_rsv, _ = STACKS[name]
    p = np.stack([defaults(), defaults()])
    p[0, k_rsv], p[1, k_rsv] = 1.0, 0.5
    p[0, k_dtf], p[1, k_dtf] = 6.0, 4.0
    p[0, k_ae], p[1, k_ae] = 1.5, 1.2
    if k_gm is not None:
        p[:, k_gm] = GM_DIRECT
    return p


@functools.lru_cache(maxsize=None)
def _case(name):
    """geo, parameters [2][ref], set_ix, the melt-season forcing and the state the oracle reaches at its start"""
    _, run, _, state0, *_ = STACKS[name]
    geo = _geo()
    p = _params(name)
    ix = (np.arange(N) % 2).astype(np.int32)
    kw = dict(gm_direct=GM_DIRECT) if name == "pt_hps_k" else {}
    spin = run("oracle", geo, p, state0(N), synthetic.T0_2015_US, HOUR, synthetic.forcing(N, 0, STEP0, z=geo[:, 2]),
               set_ix=ix, full=False, **kw)
    f = synthetic.forcing(N, STEP0, T, z=geo[:, 2])
    return geo, p, ix, f, spin["state"]


@functools.lru_cache(maxsize=None)
def _reference(name, n_sets):
    """the oracle's result, every series and the state series; one set: the second (non-default) set alone"""
    _, run, *_ = STACKS[name]
    geo, p, ix, f, st = _case(name)
    kw = {}
    if name == "pt_hps_k":
        kw["gm_direct"] = GM_DIRECT if n_sets == 2 else GM_DIRECT[1:]
    t0 = synthetic.T0_2015_US + STEP0 * HOUR
    if n_sets == 2:
        return run("oracle", geo, p, st, t0, HOUR, f, set_ix=ix, full=True, collect_state=True, **kw)
    return run("oracle", geo, p[1], st, t0, HOUR, f, full=True, collect_state=True, **kw)


def _device_rows(name, p, gm):
    """the rows handed to the C ABI: pt_hps_k's carry gm.direct_response and the snow distribution behind the 24"""
    if name != "pt_hps_k":
        return p
    d = np.tile(oracle_lib.hbv_dist_row([1.0] * 5, A5), (p.shape[0], 1))
    return np.concatenate([p, np.asarray(gm, dtype=np.float64).reshape(-1, 1), d], axis=1)


def _run_hip(name, n_sets, collect, collect_state):
    sid, *_, n_state_series = STACKS[name]
    geo, p, ix, f, st = _case(name)
    rows = _device_rows(name, p, GM_DIRECT) if n_sets == 2 else _device_rows(name, p[1:], GM_DIRECT[1:])
    r = HipRegion(sid, N)
    try:
        r.set_geo(geo)
        r.set_parameters(rows, ix if n_sets == 2 else None)
        r.set_time_axis(synthetic.T0_2015_US + STEP0 * HOUR, HOUR, T)
        r.set_collection(collect, collect_state)
        r.set_state(st)
        for v in range(5):
            r.set_forcing(v, 0, f[v])
        r.run_cells()
        out = {"state": r.get_state(),
               "series": np.stack([r.get_series(k, 0, T) for k in range((2, 4, 8)[collect])])}
        if collect_state:
            out["state_series"] = np.stack([r.get_state_series(k, 0, T + 1) for k in range(n_state_series)])
        return out
    finally:
        r.close()


def _assert_not_vacuous(name, n_sets):
    """the oracle's result has glacier melt and none of it on glaciated cells, both signs of prec - ae, snow-covered
    and bare cells, and temperatures on both sides of 0 C"""
    geo, _, _, f, _ = _case(name)
    full = _reference(name, n_sets)["full"]
    sca, glacier_melt, ae = full[2], full[5], full[6]
    has_glacier = np.broadcast_to(geo[:, 6] > 0.0, glacier_melt.shape)
    assert (glacier_melt > 0.0).any()
    assert ((glacier_melt == 0.0) & has_glacier).any()
    assert (glacier_melt[:, geo[:, 6] == 0.0] == 0.0).all()
    assert (f[1] - ae < 0.0).any() and (f[1] - ae > 0.0).any()  # p_corr is 1: prec is the forcing's
    # snow-covered and bare cell-steps (the default, flat hbv_snow distribution has nothing in between)
    assert (sca < 1.0).any() and (sca > 0.0).any()
    assert (f[0] > 0.0).any() and (f[0] <= 0.0).any()
    assert np.isfinite(full).all()


@pytest.mark.parametrize("name", list(STACKS))
def test_oracle_case_reaches_every_branch_of_the_tail(name):
    for n_sets in (1, 2):
        _assert_not_vacuous(name, n_sets)


@pytest.mark.gpu
@pytest.mark.parametrize("collect", [COLLECT_DISCHARGE, COLLECT_DISCHARGE_SNOW, COLLECT_ALL],
                         ids=["discharge", "discharge_snow", "all"])
@pytest.mark.parametrize("name", list(STACKS))
def test_step_tail_bitexact(name, collect):
    collect_state = collect == COLLECT_ALL
    for n_sets in (1, 2):
        _assert_not_vacuous(name, n_sets)
        ref = _reference(name, n_sets)
        want = {"state": ref["state"], "series": ref["full"][:(2, 4, 8)[collect]]}
        keys = ["series", "state"]
        if collect_state:
            want["state_series"] = ref["state_series"]
            keys.append("state_series")
        _assert_same(_run_hip(name, n_sets, collect, collect_state), want, keys)
