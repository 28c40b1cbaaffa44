"""hbv_stack, pt_hs_k and pt_hps_k on the device against the oracle, bit for bit, on the single-step jobs and the
scripted sequences of tests/snow_cases.py: every branch of hbv_snow_step, hbv_distribute, hbv_integrate0 and hps_step
(the labels test_snow_steps_host.py counts) at time steps of 1 h, 3 h and 24 h, every launch instance of
launch_hbv_run, launch_pthsk_run and launch_pthpsk_run by the condition that selects it, and the "Negative outflow"
failure next to the mass-balance clamp that must not fail. A job is one cell of a region with T = 1; the product's own
HipRegion runs it. No comparison here has a tolerance."""
import functools
import re

import numpy as np
import pytest

from tests import snow_cases as sc

pytestmark = pytest.mark.gpu

N_SERIES = {"hbv_stack": 9, "pt_hs_k": 8, "pt_hps_k": 8}
N_STATE_SERIES = {"hbv_stack": 22, "pt_hs_k": 19, "pt_hps_k": 36}
DISCHARGE, DISCHARGE_SNOW, ALL = 0, 1, 2          # region.COLLECT_*
N_COLLECTED = (2, 4, None)
# the state columns of bins 5..7 (sp, sw and, for pt_hps_k, albedo and iso_pot_energy)
UPPER_BINS = {"hbv_stack": [6 + b * 8 + i for b in range(2) for i in (5, 6, 7)],
              "pt_hs_k": [3 + b * 8 + i for b in range(2) for i in (5, 6, 7)]}
SET = {name: k for k, name in enumerate(sc.set_names())}
DT_NAMES = list(sc.DTS)


def _stack_id(stack):
    from shyft_amd import region
    return {"hbv_stack": region.HBV_STACK, "pt_hs_k": region.PT_HS_K, "pt_hps_k": region.PT_HPS_K}[stack]


def _device_rows(stack, case, k):
    """the C-ABI parameter rows: the reference row, pt_hps_k's gm.direct_response, the snow distribution; every set
    (k None) or set k alone"""
    sel = slice(None) if k is None else slice(k, k + 1)
    cols = [case["params"][sel]]
    if stack == "pt_hps_k":
        cols.append(np.asarray(case["gm_direct"], dtype=np.float64)[sel].reshape(-1, 1))
    cols.append(case["dist"][sel])
    return np.concatenate(cols, axis=1)


def _of_set(case, k):
    """the cells of a case that belong to set k (one more, so that the count is no multiple of 64)"""
    idx = np.flatnonzero(case["set_ix"] == k)
    if len(idx) % 64 == 0:
        idx = np.append(idx, idx[0])
    out = dict(case)
    out.update(geo=case["geo"][idx], state=case["state"][idx], forcing=np.ascontiguousarray(case["forcing"][:, :, idx]),
               set_ix=case["set_ix"][idx])
    if "jobs" in case:
        out["jobs"] = case["jobs"][idx]
    return out


def _run_hip(stack, case, k=None, collect=ALL, collect_state=True, catchments=None, stepwise=False):
    """run a case on the device with every set assigned per lane (k None) or with set k alone (the uniform launch);
    dict series [n][T][N], state [N][.], state_series [.][T + 1][N]"""
    from shyft_amd.region import HipRegion
    n, T = case["geo"].shape[0], case["forcing"].shape[1]
    r = HipRegion(_stack_id(stack), n)
    try:
        r.set_geo(case["geo"])
        r.set_parameters(_device_rows(stack, case, k), case["set_ix"] if k is None else None)
        r.set_time_axis(0, case["dt_us"], T)
        r.set_collection(collect, collect_state)
        r.set_state(case["state"])
        for v in range(5):
            r.set_forcing(v, 0, case["forcing"][v])
        if catchments is not None:
            r.set_catchment_filter(catchments)
        if stepwise:
            for t in range(T):
                r.run_cells(0, t, 1)
        else:
            r.run_cells()
        ns = N_COLLECTED[collect] or N_SERIES[stack]
        out = {"series": np.stack([r.get_series(s, 0, T) for s in range(ns)]), "state": r.get_state()}
        if collect_state:
            out["state_series"] = np.stack([r.get_state_series(s, 0, T + 1) for s in range(N_STATE_SERIES[stack])])
        return out
    finally:
        r.close()


def _oracle(stack, case, k=None):
    if k is None:
        return sc.run_oracle_region(stack, case)
    gm = case["gm_direct"][k:k + 1]
    return sc.run_oracle_region(stack, case, set_ix=None, params=case["params"][k], dist=case["dist"][k:k + 1],
                                gm_direct=gm)


def _same(x, y):
    return (x.view(np.int64) == y.view(np.int64)) | (np.isnan(x) & np.isnan(y))   # NaN as NaN, zeros by sign


def _assert_cells_same(stack, dt_name, got, ref, collect, collect_state, case, cells=None):
    """every collected response series, both rows of the state series and the final state, bit for bit; a failure
    names the first differing job, its labels and its inputs"""
    ns = N_COLLECTED[collect] or N_SERIES[stack]
    pairs = [("series", got["series"], ref["full"][:ns], -1), ("state", got["state"], ref["state"], 0)]
    if collect_state:
        pairs.append(("state_series", got["state_series"], ref["state_series"], -1))
    bad = {}
    for name, x, y, axis in pairs:
        assert x.shape == y.shape, (name, x.shape, y.shape)
        same = np.moveaxis(_same(np.ascontiguousarray(x), np.ascontiguousarray(y)), axis, 0)
        if cells is not None:
            same = same[cells]
        wrong = np.flatnonzero(~same.reshape(same.shape[0], -1).all(axis=1))
        if wrong.size:
            c = int(wrong[0] if cells is None else np.arange(x.shape[axis])[cells][wrong[0]])
            bad[name] = (c, wrong.size)
    if not bad:
        return
    c = min(v[0] for v in bad.values())
    msg = [f"{stack} {dt_name}: {bad} differ (first cell, cells); first differing cell {c}"]
    if "jobs" in case:
        jobs = sc.stack_jobs(stack, dt_name)
        i = int(case["jobs"][c])
        msg.append(f"job {i} ({jobs['tag'][i]}), set {sc.set_names()[int(jobs['k'][i])]}, labels {sorted(jobs['labels'][i])}")
    msg.append(f"state in {case['state'][c].tolist()}")
    msg.append(f"forcing (temp prec wind rh rad per step) {case['forcing'][:, :, c].T.tolist()}")
    msg.append(f"state out {got['state'][c].tolist()}\n   oracle {ref['state'][c].tolist()}")
    for s in range(got["series"].shape[0]):
        if not _same(got["series"][s, :, c], ref["full"][s, :, c]).all():
            msg.append(f"series {s}: {got['series'][s, :, c].tolist()} oracle {ref['full'][s, :, c].tolist()}")
    raise AssertionError("\n".join(msg))


@functools.lru_cache(maxsize=None)
def _clean(stack, dt_name):
    """the clean jobs of a stack as a region and the oracle's run of it with every set assigned per lane"""
    case = sc.region_case(stack, dt_name)
    n = case["geo"].shape[0]
    assert n < 3000 and n % 64 != 0 and n % 256 != 0
    assert len(set(case["set_ix"].tolist())) == len(sc.set_names())
    return case, sc.run_oracle_region(stack, case)


@functools.lru_cache(maxsize=None)
def _clean_of_set(stack, dt_name, name):
    case = _of_set(_clean(stack, dt_name)[0], SET[name])
    return case, _oracle(stack, case, SET[name])


# ---- job runs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("stack", sc.STACKS)
def test_jobs_bit_for_bit(stack, dt_name):
    """Every clean job as one cell, sets of 2, 3, 5 and 8 bins assigned per lane: hbv_run_kernel<false, 8>,
    pthsk_run_kernel<false, 8>, pthpsk_run_kernel<false> (more than one parameter set: uniform_params is 0)."""
    case, ref = _clean(stack, dt_name)
    got = _run_hip(stack, case)
    _assert_cells_same(stack, dt_name, got, ref, ALL, True, case)


@pytest.mark.parametrize("stack", sc.STACKS)
def test_jobs_through_a_catchment_filter(stack):
    """The 3 h jobs with catchment 1 selected: its cells equal the oracle, a filtered-out cell's state row comes back
    as it went in (stale bin slots included) and its series rows are never written."""
    case, ref = _clean(stack, "3h")
    got = _run_hip(stack, case, catchments=[1])
    sel = case["geo"][:, 4] == 1
    assert 0 < sel.sum() < sel.size
    _assert_cells_same(stack, "3h", got, ref, ALL, True, case, cells=sel)
    assert _same(got["state"][~sel], case["state"][~sel]).all()
    assert np.isnan(got["series"][:, :, ~sel]).all() and np.isnan(got["state_series"][:, :, ~sel]).all()


# ---- launch instances ------------------------------------------------------------------------------------------------
def _check_uniform(stack, dt_name, name, collect, collect_state, five_bin_kernel):
    case, ref = _clean_of_set(stack, dt_name, name)
    got = _run_hip(stack, case, k=SET[name], collect=collect, collect_state=collect_state)
    _assert_cells_same(stack, dt_name, got, ref, collect, collect_state, case)
    if five_bin_kernel:   # bins 5..7 of the state come back as zeros whatever the input held
        cols = UPPER_BINS[stack]
        assert (case["state"][:, cols] != 0.0).any(), "no job of this set hands in stale upper bins"
        assert (got["state"][:, cols].view(np.int64) == 0).all()


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("name", ["flat5", "skew5", "zero5"])
def test_hbv_uniform_exact_five_bins_lean(name, dt_name):
    """hbv_run_kernel<true, 5, true, true>: one parameter set (uniform_params), nb_max == 5, no state series and the
    discharge collector only (collect == 0). The bin count is the compile-time 5."""
    _check_uniform("hbv_stack", dt_name, name, DISCHARGE, False, True)


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("name", ["three", "two"])
def test_hbv_uniform_fewer_than_five_bins_lean(name, dt_name):
    """hbv_run_kernel<true, 5, true>: one set of 3 bins, and one of 2: nb_max <= 5 but not 5, no state series,
    collect == 0. Capacity 5 with a runtime bin count: every i < nb guard is live."""
    _check_uniform("hbv_stack", dt_name, name, DISCHARGE, False, True)


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("collect", [DISCHARGE_SNOW, ALL])
@pytest.mark.parametrize("name", ["three", "skew5"])
def test_hbv_uniform_five_bin_capacity_with_collectors(name, collect, dt_name):
    """hbv_run_kernel<true, 5>: one set of at most 5 bins and no state series, but collection 1 or 2, which the lean
    instances do not serve."""
    _check_uniform("hbv_stack", dt_name, name, collect, False, True)


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("name,collect,collect_state", [("eight", DISCHARGE, False), ("flat5", ALL, True)])
def test_hbv_uniform_eight_bin_capacity(name, collect, collect_state, dt_name):
    """hbv_run_kernel<true, 8>: one set, and either nb_max == 8 (the 8-bin set, discharge only) or a state series is
    collected (the 5-bin set with the state series), either of which rules the capacity-5 instances out."""
    _check_uniform("hbv_stack", dt_name, name, collect, collect_state, False)


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("stack", sc.STACKS)
def test_per_lane_instance_discharge_only(stack, dt_name):
    """hbv_run_kernel<false, 8>, pthsk_run_kernel<false, 8>, pthpsk_run_kernel<false>: six sets of 2, 3, 5 and 8 bins
    assigned per lane select the per-lane instance whatever is collected; here the discharge collector alone and no
    state series, the conditions under which one set would pick a lean instance."""
    case, ref = _clean(stack, dt_name)
    got = _run_hip(stack, case, collect=DISCHARGE, collect_state=False)
    _assert_cells_same(stack, dt_name, got, ref, DISCHARGE, False, case)


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("name", ["flat5", "skew5"])
def test_pthsk_uniform_exact_five_bins(name, dt_name):
    """pthsk_run_kernel<true, 5, true>: one set, nb_max == 5, no state series (any collection)."""
    _check_uniform("pt_hs_k", dt_name, name, ALL, False, True)


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("name", ["three", "two"])
def test_pthsk_uniform_fewer_than_five_bins(name, dt_name):
    """pthsk_run_kernel<true, 5>: one set of 3 bins, and one of 2 (nb_max <= 5 but not 5), no state series: capacity
    5 with a runtime bin count, every i < nb guard live."""
    _check_uniform("pt_hs_k", dt_name, name, DISCHARGE, False, True)


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("name,collect,collect_state", [("eight", DISCHARGE, False), ("zero5", ALL, True)])
def test_pthsk_uniform_eight_bin_capacity(name, collect, collect_state, dt_name):
    """pthsk_run_kernel<true, 8>: one set with nb_max == 8, or a 5-bin set with the state series collected."""
    _check_uniform("pt_hs_k", dt_name, name, collect, collect_state, False)


@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("name", ["three", "eight", "two", "skew5"])
def test_pthpsk_uniform(name, dt_name):
    """pthpsk_run_kernel<true>: one parameter set (uniform_params); its bin capacity is always 8, here with a 3-bin
    and an 8-bin set (and 2 and 5 bins), all series and the state series."""
    _check_uniform("pt_hps_k", dt_name, name, ALL, True, False)


# ---- scripted sequences ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("stack", sc.STACKS)
def test_scripted_sequences_whole_and_stepwise(stack, dt_name):
    """A dozen cells over 11 steps in which one branch's output is the next step's input (the events
    test_snow_steps_host.py asserts), run once as a whole and once with run_cells per step: both equal the oracle."""
    case = sc.sequence_case(stack, dt_name)
    ref = sc.run_oracle_region(stack, case)
    for stepwise in (False, True):
        got = _run_hip(stack, case, stepwise=stepwise)
        _assert_cells_same(stack, dt_name, got, ref, ALL, True, case)


# ---- raising jobs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt_name", DT_NAMES)
@pytest.mark.parametrize("stack", sc.STACKS)
def test_raising_jobs_fail_the_run_and_clamped_jobs_do_not(stack, dt_name):
    """Per cause (the branch that left more water in the bins than came in): 40 clean jobs mixed with that cause's
    raising jobs fail with "Negative outflow" and name a cell whose job raises on the oracle; the same region without
    them passes bit for bit; a region of only clamp-branch jobs (-tolerance <= total_water - swe < 0) does not fail."""
    from shyft_amd._native import ShyftHipError
    jobs = sc.stack_jobs(stack, dt_name)
    clean_ix = np.flatnonzero(~jobs["raises"])[::max(1, int((~jobs["raises"]).sum()) // 40)][:40]
    causes = {}
    for i in np.flatnonzero(jobs["raises"]):
        causes.setdefault(sc._cause(jobs["labels"][i]), []).append(int(i))
    assert len(causes) >= 2
    for cause, raising in causes.items():
        order = np.sort(np.concatenate([clean_ix, raising]))
        case = sc.region_case(stack, dt_name, select=order)
        with pytest.raises(RuntimeError, match="Negative outflow"):
            sc.run_oracle_region(stack, case)
        with pytest.raises(ShyftHipError, match="Negative outflow") as e:
            _run_hip(stack, case)
        cell = int(re.search(r"cell (\d+)", str(e.value)).group(1))
        assert jobs["raises"][order[cell]], (cause, cell, int(order[cell]))
    case = sc.region_case(stack, dt_name, select=clean_ix)
    _assert_cells_same(stack, dt_name, _run_hip(stack, case), sc.run_oracle_region(stack, case), ALL, True, case)
    clamp = np.array([i for i, (L, r) in enumerate(zip(jobs["labels"], jobs["raises"])) if "clamp" in L and not r])
    assert clamp.size >= 8
    case = sc.region_case(stack, dt_name, select=clamp)
    _assert_cells_same(stack, dt_name, _run_hip(stack, case), sc.run_oracle_region(stack, case), ALL, True, case)
