"""Bayesian temperature kriging at its edges (kernels/btk.hip, the region entry, the sharded entry).

CPU: every case of tests/btk_cases.py meets its admission conditions (oracle against an independent numpy statement
below 1e-10; neighbouring destinations and steps more than 1e-6 apart), and the oracle's error texts for a reduced
step with a single valid source and for two coincident sources.

GPU: the device against oracle_btk at the tolerance of tests/test_btk.py (TOL = 1e-9 degC), on
  the stateless entry: destination and source counts around the thread block and the wavefront, every placement of a
      pattern's steps (direct at row 0, direct at a row offset, scatter, blocks of 1, 2 and 7 steps), coincident
      and far destinations, zscale 0, the 200 km range, and a pattern of more than 65535 non-contiguous steps;
  the region entry: a sub-window of a sentinel-filled window with and without a catchment filter, where everything
      outside the window and the filter must keep the sentinel bit for bit; the cache hit and every way its key
      can go stale, error recovery included;
  sharded regions on one device and two regions driven from two threads (one rocBLAS handle per device).
"""
import threading

import numpy as np
import pytest

from tests import btk_cases as bc
from tests.test_btk import TOL, oracle_btk

N, T, W0, W = bc.REGION_N, bc.REGION_T, bc.REGION_W0, bc.REGION_W
SENTINEL = 77.0
SINGULAR = r"inv\(\): matrix is singular"


def _err(got, ref, what):
    assert got.shape == ref.shape
    e = float(np.max(np.abs(got - ref)))  # NaN if either side has one: fails every bound below
    print(f"btk-edge {what}: max|device - oracle| = {e:.3e}")
    return e


# ---- error cases (host and device) ----------------------------------------------------------------------------------
ERR_SRC = np.array([[0.0, 0.0, 0.0], [1000.0, 0.0, 300.0], [0.0, 1000.0, 700.0]])
ERR_VALS = 10.0 + np.arange(9.0).reshape(3, 3)
ERR_PRIOR = [-0.006] * 3
ERR_DST = np.array([[100.0, 200.0, 50.0], [500.0, 500.0, 400.0], [900.0, 100.0, 650.0], [50.0, 950.0, 20.0]])


def _error_cases():
    """(name, src, vals): a reduced step whose only valid source is source 0, at sea level (H^-1 exactly singular)
    and at 37 m (singular after rounding); two coincident sources (two equal rows of K)."""
    alone = bc.single_valid(ERR_VALS, 1, 0)
    at37 = ERR_SRC.copy()
    at37[0, 2] = 37.0
    twin = ERR_SRC.copy()
    twin[2] = twin[1]
    return [("single-valid-z0", ERR_SRC, alone), ("single-valid-z37", at37, alone), ("coincident-sources", twin, ERR_VALS)]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bc.BUILDERS))
def test_case_is_admitted(name):
    case, ref = bc.case_and_oracle(name)
    assert np.isfinite(ref).all()
    # long_alternating: numpy_btk on the first and last 512 steps (both patterns, the same distribution of values)
    steps = np.r_[0:512, ref.shape[0] - 512:ref.shape[0]] if ref.shape[0] > 4096 else None
    cond, by_dst, by_step = bc.admission(case, ref, steps)
    assert cond < bc.COND, cond
    assert by_dst > bc.SENS and by_step > bc.SENS, (by_dst, by_step)


@pytest.mark.parametrize("layout", ["contiguous", "alternating", "full", "reduced", "cache"])
def test_region_case_is_admitted(layout):
    case = bc.cache_case() if layout == "cache" else bc.region_case(layout)
    cond, by_dst, by_step = bc.admission(case)
    assert cond < bc.COND and by_dst > bc.SENS and by_step > bc.SENS, (cond, by_dst, by_step)


def test_pattern_layout_has_every_placement():
    seq = bc.pattern_layout()
    steps = {}
    for t, p in enumerate(seq):
        steps.setdefault(p, []).append(t)
    runs = {p: np.split(np.array(s), np.where(np.diff(s) != 1)[0] + 1) for p, s in steps.items()}
    assert seq[0] == () and seq[-1] == () and len(runs[()]) == 2            # the full set first and last
    assert any(len(r) == 1 and len(r[0]) >= 8 and r[0][0] > 0 for p, r in runs.items() if p)  # one run at an offset
    assert sum(1 for r in runs.values() if len(r) >= 5 and all(len(x) == 1 for x in r)) == 2  # two alternating
    assert any(len(r) == 2 and all(len(x) == 2 for x in r) for r in runs.values())            # returns after a gap
    assert sum(1 for s in steps.values() if len(s) == 1) >= 20                              # distinct single steps
    vals = bc.patterns()[1]
    assert np.isposinf(vals).any() and np.isneginf(vals).any() and np.isnan(vals).any()
    assert np.isfinite(vals[:, :2]).all()


def test_oracle_takes_infinities_as_missing():
    case, ref = bc.case_and_oracle("patterns")
    assert np.array_equal(ref, oracle_btk(*bc.nan_only(case)))


def test_oracle_returns_a_valid_source_at_its_own_place():
    (src, vals, _, _, _), ref = bc.case_and_oracle("coincident")
    ok = np.isfinite(vals)
    assert (~ok).any() and np.max(np.abs(ref[:, :len(src)] - vals)[ok]) < 1e-13


def test_far_destinations_lose_the_covariance():
    src, vals, prior, prm, dst = bc.case_and_oracle("far")[0]
    d = np.sqrt(((dst[:, None, :2] - src[None, :, :2]) ** 2).sum(-1) + ((dst[:, None, 2] - src[None, :, 2]) * prm[4]) ** 2)
    sweep = d[bc.FAR_AWAY:] / prm[3]
    # the network is 2 km across: 690 .. 760 to within 2, over exp's gradual underflow (-708.4 .. -745.13)
    assert 688 < sweep.min() < 692 and 758 < sweep.max() < 762
    assert np.exp(-d[:bc.FAR_AWAY] / prm[3]).max() == 0.0       # only the trend remains at 1e6 m


def test_long_alternating_has_two_patterns_beyond_one_scatter_launch():
    vals = bc.case_and_oracle("long_alternating")[0][1]
    odd = np.isnan(vals[:, 2])
    assert odd[1::2].all() and not odd[0::2].any() and np.isfinite(vals[:, :2]).all()
    assert odd.sum() == 65537 and (~odd).sum() == 65537


@pytest.mark.parametrize("name,src,vals", _error_cases(), ids=[c[0] for c in _error_cases()])
def test_oracle_error_texts_of_singular_sets(name, src, vals):
    with pytest.raises(RuntimeError, match=SINGULAR):
        oracle_btk(src, vals, ERR_PRIOR, bc.PRM, ERR_DST)


def test_call_after_an_error_is_well_conditioned():
    assert bc.admission((ERR_SRC, ERR_VALS, ERR_PRIOR, bc.PRM, ERR_DST))[0] < bc.COND


def test_cache_case_error_step_is_singular_in_the_oracle():
    src, vals, prior, prm, dst = bc.cache_case()
    with pytest.raises(RuntimeError, match=SINGULAR):
        oracle_btk(src, bc.single_valid(vals, 25, bc.LEVEL_SOURCE), prior, prm, dst[:4])


# ---- GPU: the stateless entry -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(bc.BUILDERS))
def test_device_matches_oracle(name):
    from shyft_amd.region import btk
    case, ref = bc.case_and_oracle(name)
    got = btk(*case)
    assert _err(got, ref, name) < TOL
    if name == "coincident":  # a valid source is returned at its own place, full and reduced patterns alike
        src, vals = case[0], case[1]
        ok = np.isfinite(vals)
        assert np.max(np.abs(got[:, :len(src)] - vals)[ok]) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("block_steps", [1, 2, 7])
def test_device_step_blocks_match_oracle(block_steps):
    from shyft_amd.region import btk
    case, ref = bc.case_and_oracle("patterns")
    assert _err(btk(*case, block_steps=block_steps), ref, f"patterns block_steps={block_steps}") < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name,src,vals", _error_cases(), ids=[c[0] for c in _error_cases()])
def test_device_raises_as_the_oracle_and_recovers(name, src, vals):
    from shyft_amd.region import btk
    with pytest.raises(RuntimeError, match=SINGULAR):
        btk(src, vals, ERR_PRIOR, bc.PRM, ERR_DST)
    got = btk(ERR_SRC, ERR_VALS, ERR_PRIOR, bc.PRM, ERR_DST)
    assert _err(got, oracle_btk(ERR_SRC, ERR_VALS, ERR_PRIOR, bc.PRM, ERR_DST), f"after {name}") < TOL


# ---- GPU: the region entry --------------------------------------------------------------------------------------------------
CATCHMENT = 1 + np.arange(N) // 200
_REGION_ORACLE = {}


def _oracle_all_cells(key, case):
    """The oracle of a region case at all 600 cells (each destination is computed on its own, so a filter's result
    is the selected columns), computed once per key."""
    if key not in _REGION_ORACLE:
        ref = oracle_btk(*case)
        ref.setflags(write=False)
        _REGION_ORACLE[key] = ref
    return _REGION_ORACLE[key]


def _fill(r, value=SENTINEL):
    """The whole temperature window := value, through the one-source copy without a filter."""
    r.set_catchment_filter([])
    r.interpolate_btk(ERR_SRC[:1], np.full((T, 1), value), 0, bc.PRM)


def _region(devices=None, geo=None):
    from shyft_amd import synthetic
    from shyft_amd.region import HipRegion, PT_GS_K
    r = HipRegion(PT_GS_K, N) if devices is None else HipRegion(PT_GS_K, N, devices=devices)
    try:
        r.set_geo(bc.region_geo() if geo is None else geo)
        r.set_parameters(synthetic.default_ptgsk_parameters())
        r.set_time_axis(synthetic.T0_2015_US, synthetic.HOUR_US, T)
        _fill(r)
    except Exception:
        r.close()
        raise
    return r


def _active(filt):
    return np.isin(CATCHMENT, filt) if filt else np.ones(N, dtype=bool)


def _run_window(r, case):
    src, vals, prior, prm, _ = case
    r.interpolate_btk(src, vals, W0, prm, prior)


def _window_and_rest(r, active):
    """(the written block [W][active cells], True where everything else still holds the sentinel bit for bit)."""
    from shyft_amd.region import TEMPERATURE
    got = r.get_forcing(TEMPERATURE, 0, T)
    written = np.zeros((T, N), dtype=bool)
    written[W0:W0 + W, active] = True
    return got[W0:W0 + W][:, active], bool(np.all(got[~written] == SENTINEL))


@pytest.mark.gpu
@pytest.mark.parametrize("layout,filt", [("contiguous", None), ("contiguous", [1, 3]), ("alternating", [1, 3])],
                         ids=["contiguous-all", "contiguous-filter", "alternating-filter"])
def test_region_writes_its_window_and_filter_only(layout, filt):
    case = bc.region_case(layout)
    active = _active(filt)
    r = _region()
    try:
        r.set_catchment_filter(filt or [])
        _run_window(r, case)
        got, rest_untouched = _window_and_rest(r, active)
    finally:
        r.close()
    assert _err(got, _oracle_all_cells(layout, case)[:, active], f"region {layout} filter={filt}") < TOL
    assert rest_untouched


@pytest.mark.gpu
def test_region_single_source_copy_respects_the_filter():
    from shyft_amd.region import TEMPERATURE
    r = _region()
    try:
        r.set_catchment_filter([1, 3])
        r.interpolate_btk(ERR_SRC[:1], np.array([[55.0], [56.0], [57.0]]), 5, bc.PRM)
        got = r.get_forcing(TEMPERATURE, 0, T)
    finally:
        r.close()
    exp = np.full((T, N), SENTINEL)
    exp[5:8, _active([1, 3])] = np.array([55.0, 56.0, 57.0])[:, None]
    assert np.array_equal(got, exp)


def _cache_sequence():
    """[(what, src, vals, prm, filter, dz of the cell heights)]: the calls of the cache test on one region, each
    differing from the one before it in exactly one thing."""
    src, vals, _, prm, _ = bc.cache_case()
    seq = [("first call", src, vals, list(prm), [1, 3], 0.0)]

    def then(what, **change):
        last = dict(zip(("src", "vals", "prm", "filt", "dz"), seq[-1][1:]))
        last.update(change)
        seq.append((what, last["src"], last["vals"], last["prm"], last["filt"], last["dz"]))

    def with_prm(ix, value):
        p = list(seq[-1][3])
        p[ix] = value
        return p

    then("second call (hit)")
    then("range", prm=with_prm(3, 15000.0))
    then("zscale", prm=with_prm(4, 10.0))
    then("gradient_sd", prm=with_prm(0, 0.004))
    then("sill", prm=with_prm(1, 16.0))
    moved = src.copy()
    moved[3, 2] += 40.0
    then("one source's z", src=moved)
    then("source values only (hit)", vals=bc.cache_case(seed=12)[1])
    then("filter [1, 3] -> [1, 2]", filt=[1, 2])           # as many destinations, other cells
    then("set_geo with other heights", dz=35.0)
    then("only reduced patterns", vals=bc.cache_case("reduced")[1])   # the full set is factorised, never placed
    then("full set after only reduced patterns", vals=bc.cache_case("full")[1])
    then("before the errors", vals=vals)
    return seq


def test_cache_sequence_is_admitted():
    prior = bc.cache_case()[2]
    seen = []
    for what, src, vals, prm, filt, dz in _cache_sequence():
        if any(src is s and vals is v and prm == p and dz == z for s, v, p, z in seen):
            continue  # a hit or another filter: the same case at all cells
        seen.append((src, vals, prm, dz))
        cond, by_dst, by_step = bc.admission((src, vals, prior, prm, bc.region_geo(dz)[:, :3]))
        assert cond < bc.COND and by_dst > bc.SENS and by_step > bc.SENS, (what, cond, by_dst, by_step)


@pytest.mark.gpu
def test_region_cache_hit_and_every_stale_key():
    prior = bc.cache_case()[2]
    other = bc.cache_case(seed=12)[1]
    r = _region()
    now = {"filt": None, "dz": 0.0}

    def call_and_check(what, src, vals, prm, filt, dz):
        if dz != now["dz"]:
            r.set_geo(bc.region_geo(dz))
        if filt != now["filt"]:
            _fill(r)  # cells of the last filter back to the sentinel: no BTK call, so the cache stays as it is
            r.set_catchment_filter(filt)
        now.update(filt=filt, dz=dz)
        r.interpolate_btk(src, vals, W0, prm, prior)
        active = _active(filt)
        got, rest_untouched = _window_and_rest(r, active)
        ref = oracle_btk(src, vals, prior, prm, bc.region_geo(dz)[active, :3])
        assert _err(got, ref, f"cache {what}") < TOL, what
        assert rest_untouched, what
        return got

    try:
        results = {}
        for step in _cache_sequence():
            results[step[0]] = call_and_check(*step)
        assert np.array_equal(results["first call"], results["second call (hit)"])
        _, src, vals, prm, filt, dz = step
        # each call after an error has other temperatures than the call before it: nothing left over can pass
        with pytest.raises(RuntimeError, match=SINGULAR):  # raised after the full-set steps before it were placed
            r.interpolate_btk(src, bc.single_valid(vals, 25, bc.LEVEL_SOURCE), W0, prm, prior)
        call_and_check("after a singular reduced pattern", src, other, prm, filt, dz)
        nothing = vals.copy()
        nothing[7] = np.nan
        with pytest.raises(RuntimeError, match="No valid sources for time period"):
            r.interpolate_btk(src, nothing, W0, prm, prior)
        call_and_check("after a step without sources", src, vals, prm, filt, dz)
    finally:
        r.close()


# ---- GPU: shards on one device, regions on two threads ----------------------------------------------------------------------
SHARD_FILTERS = {"all": None, "first-shard-idle": [3]}
_UNSHARDED = {}


def _unsharded_window(filt_name):
    """The unsharded region's result of the shard case, computed once per filter."""
    if filt_name not in _UNSHARDED:
        filt = SHARD_FILTERS[filt_name]
        r = _region()
        try:
            r.set_catchment_filter(filt or [])
            _run_window(r, bc.region_case("contiguous"))
            _UNSHARDED[filt_name] = _window_and_rest(r, _active(filt))
        finally:
            r.close()
    return _UNSHARDED[filt_name]


@pytest.mark.gpu
@pytest.mark.parametrize("filt_name", list(SHARD_FILTERS))
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["two-shards", "three-shards"])
def test_shards_on_one_device_match_oracle_and_unsharded(devices, filt_name):
    filt = SHARD_FILTERS[filt_name]
    case = bc.region_case("contiguous")
    active = _active(filt)
    one, one_rest_untouched = _unsharded_window(filt_name)
    sh = _region(devices=devices)
    try:
        _, c0, nc = sh.shards()[0]
        assert (filt is not None) == (not active[c0:c0 + nc].any())   # the filter idles the first shard
        sh.set_catchment_filter(filt or [])
        _run_window(sh, case)
        got, rest_untouched = _window_and_rest(sh, active)
    finally:
        sh.close()
    ref = _oracle_all_cells("contiguous", case)[:, active]
    what = f"{len(devices)} shards filter={filt}"
    assert _err(one, ref, f"unsharded filter={filt}") < TOL and one_rest_untouched
    assert _err(got, ref, what) < TOL
    assert _err(got, one, what + " against unsharded") < 2 * TOL   # rocBLAS may pick another kernel for another D
    assert rest_untouched                                         # idle shards and filtered-out cells


@pytest.mark.gpu
def test_two_regions_on_two_threads_match_oracle():
    cases = [bc.region_case("contiguous"), bc.region_case("alternating", seed=12)]
    regions = [_region(), _region()]
    start = threading.Barrier(2, timeout=60)
    errors = [None, None]

    def drive(k):
        try:
            start.wait()
            _run_window(regions[k], cases[k])
        except Exception as e:  # reported below, on the test's thread
            errors[k] = e

    try:
        threads = [threading.Thread(target=drive, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert errors == [None, None], errors
        results = [_window_and_rest(r, _active(None)) for r in regions]
    finally:
        for r in regions:
            r.close()
    for k, (got, rest_untouched) in enumerate(results):
        assert _err(got, oracle_btk(*cases[k]), f"thread {k}") < TOL
        assert rest_untouched
