"""Inverse-distance interpolation at its edges: every gather instance launch_idw_gather can pick (register tier 8 /
12 / 20 / 32 x model x wavefront-union / LDS row tiles / global-memory rows) and the neighbour selection's corner
cases -- fewer candidates than max_members, none at all, exact weight ties at the cut, the weight clamp, stations
exactly at max_distance -- on the inputs of tests/idw_cases.py.

CPU: the inputs have the properties the device tests rely on, and the oracle agrees with a plain numpy restatement
of the reference's rules. GPU: the kernels against the oracle, bit for bit, with the gather that ran asserted on
every call."""
import contextlib

import numpy as np
import pytest

from tests import idw_cases as ic

HOUR = 3600 * 10**6
POISON = -777.0     # written over the forcing rows before a run: a cell the kernel skips shows up


# ------------------------------------------------------------------------------------------------------------- CPU

def _counts(which, pset):
    w, cand = ic.np_weights(ic.stations(which), ic.cells(), ic.param(pset, 1))
    return w, cand, cand.sum(1)


def test_edge_inputs_have_the_classes_they_claim(capsys):
    """"near": for every max_members up to 21 there are cells with fewer, exactly as many and more candidates, and a
    cell whose K-th and (K+1)-th weights are equal (the tie decides who is kept); some weights are clamped to 1
    (cells on top of a station), a station lies exactly at max_distance, and some cells have no candidate. "far":
    wavefronts 0-3 have at least 32 candidates in every cell (exactly max_members kept, whatever max_members),
    wavefront 4 is mixed and wavefront 5 has none."""
    w, cand, cnt = _counts("edge", "near")
    sorted_w = -np.sort(-np.where(cand, w, -1.0), axis=1)
    lines = []
    for K in ic.K_VALUES:
        if K > 21:
            continue
        below, at, above = int((cnt < K).sum()), int((cnt == K).sum()), int((cnt > K).sum())
        ties = int(((cnt > K) & (sorted_w[:, K - 1] == sorted_w[:, K])).sum())
        lines.append(f"near K={K}: {below} cells below / {at} at / {above} above max_members, {ties} with a tie at the cut")
        assert below > 0 and at > 0 and above > 0 and ties > 0, lines[-1]
    clamped = int((w == 1.0).sum())
    min_w = 1.0 / (2500.0 * 2500.0)
    lines.append(f"near: {clamped} weights clamped to 1, {int((cnt == 0).sum())} cells without a candidate, "
                 f"{int((w == min_w).sum())} weights exactly at the minimum")
    with capsys.disabled():     # the class counts are part of the test's report
        print("\n" + "\n".join(lines))
    assert clamped > 0 and (cnt == 0).any() and (w == min_w).any()
    assert (cnt[-ic.N_FAR_CELLS:] == 0).all()
    _, _, cnt = _counts("edge", "far")
    assert ic.N_CELLS == 5 * 64 + 13 == 256 + 77
    assert (cnt[:256] >= 32).all()
    assert (cnt[256:320] >= 32).any() and (cnt[256:320] == 0).any()
    assert (cnt[320:] == 0).all()


def test_large_station_set_has_the_same_kinds_of_counts():
    """S = 4100: rows too long for the 32 KB tile budget of any model, candidate counts below, at and above
    max_members = 20 for "near", and "far" as on the small set."""
    xyz = ic.stations("large")
    assert xyz.shape == (4100, 3) and 8 * xyz.shape[0] > 32 * 1024
    assert ic.rows("large").shape == (5, 4100) and np.isnan(ic.rows("large")).any(axis=1).sum() == 1
    _, _, cnt = _counts("large", "near")
    print(f"large near K=20: {(cnt < 20).sum()} / {(cnt == 20).sum()} / {(cnt > 20).sum()}; max {cnt.max()}")
    assert (cnt < 20).any() and (cnt == 20).any() and (cnt > 20).any()
    assert (cnt > 12).sum() == ic.N_CELLS - ic.N_FAR_CELLS and cnt.max() < 32
    _, _, cnt = _counts("large", "far")
    assert (cnt[:256] >= 32).all() and (cnt[320:] == 0).all()


def test_edge_rows_are_what_they_claim():
    v = ic.rows()
    assert v.shape == (ic.T_ROWS, 49)
    bad = np.flatnonzero(~np.isfinite(v).all(axis=1))
    assert list(bad) == [1, 3, 5, 64, 66] and ic.ROW_HUGE == 63     # the 1e300 row is finite
    assert np.isnan(v[ic.ROW_ALL_NAN]).all() and np.isnan(v[ic.ROW_ALL_NAN_2]).all()
    for r in (ic.ROW_SOME_NAN, ic.ROW_SOME_NAN_2):
        assert 0 < np.isnan(v[r]).sum() < 49
    assert np.isposinf(v[ic.ROW_INF]).sum() == 1 and np.isneginf(v[ic.ROW_INF]).sum() == 1
    assert (v[ic.ROW_HUGE] == ic.HUGE).sum() == 1


def test_oracle_against_numpy_restatement():
    """The oracle's run_interpolation against tests/idw_cases.np_idw (stable descending sort with ties to the lower
    source index above max_members, source order otherwise; the min/max gradient scan with dz > 50; the cofactor
    3 x 3 solve with its fallback on a non-finite solution; the per-model transforms; NaN without a finite
    neighbour), all models, max_members 1, 8, 13, 32, near and far: the same NaN pattern, and values within 1e-12
    relative to max(|x|, 1) -- the room for detmath's pow against numpy's (<= 2 ulp each) in the weights and the
    precipitation factor, summed over <= 32 terms. Measured worst: 5.3e-15 (temperature_eq, far).

    The by-equation runs must take the overflow fallback somewhere (usable determinant, non-finite solution)."""
    geo, xyz, vals = ic.cells(), ic.stations(), ic.rows()
    worst, overflowed = 0.0, 0
    for model in ic.MODELS:
        for K in (1, 8, 13, 32):
            for pset in ("near", "far"):
                got, ovf = ic.np_idw(model, ic.param(pset, K, ic.MODELS[model][2]), xyz, vals, geo)
                exp = ic.expected(model, K, pset)
                overflowed += ovf
                assert np.array_equal(np.isnan(got), np.isnan(exp)), (model, K, pset)
                assert np.isnan(exp[ic.ROW_ALL_NAN]).all() and np.isnan(exp[:, -ic.N_FAR_CELLS:]).all()
                ok = ~np.isnan(exp)
                rel = float(np.max(np.abs(got[ok] - exp[ok]) / np.maximum(np.abs(exp[ok]), 1.0)))
                worst = max(worst, rel)
                assert rel <= 1e-12, (model, K, pset, rel)
    print(f"oracle vs numpy restatement: worst relative difference {worst:.3g}; "
          f"{overflowed} by-equation solves fell back on overflow")
    assert overflowed > 0


@pytest.mark.parametrize("K", [1, 8, 12, 20, 21])
def test_the_tie_rule_decides_results(K):
    """Ties at the cut go to the lower source index (the reference's partial_sort leaves them unspecified). With the
    other order the restatement keeps different stations in the tied cells and leaves the oracle by far more than
    the rounding bound, so the device comparison on these inputs does check the rule."""
    geo, xyz, vals = ic.cells(), ic.stations(), ic.rows()
    exp = ic.expected("wind_speed", K, "near")
    other, _ = ic.np_idw("wind_speed", ic.param("near", K), xyz, vals, geo, ties_to_lower=False)
    ok = ~np.isnan(exp) & ~np.isnan(other)    # (another station can also be missing where the kept one is not)
    rel = np.abs(other[ok] - exp[ok]) / np.maximum(np.abs(exp[ok]), 1.0)
    assert (rel > 1e-6).any(), rel.max()


def _cache_steps(pset):
    """The calls of the table-cache test, each differing from the one before in one input:
    (what, model, stations, cells, parameters)."""
    geo, xyz = ic.cells(), ic.stations()
    moved = xyz.copy()
    moved[ic.NEAR_PLANE_STATION] += (300.0, -200.0, 50.0)
    geo2 = geo.copy()
    geo2[:, 2] += 37.5
    eq = ic.param(pset, 12, True, default_gradient=-0.01)
    return [
        ("first call", "temperature", xyz, geo, ic.param(pset, 12)),
        ("default_gradient changed", "temperature", xyz, geo, ic.param(pset, 12, default_gradient=-0.01)),
        ("by_equation on", "temperature_eq", xyz, geo, eq),
        ("one station moved", "temperature_eq", moved, geo, eq),
        ("set_geo, cells 37.5 m higher", "temperature_eq", moved, geo2, eq),
        ("by_equation off", "temperature", moved, geo2, ic.param(pset, 12, default_gradient=-0.01)),
    ]


def test_table_cache_steps_each_change_the_answer(pset="near"):
    """Every step of the device's table-cache test changes the oracle's result, so a stale table, stale station
    coordinates or a stale parameter cannot pass there ("near": cells with one neighbour, or neighbours all at
    z = 100, use default_gradient; with "far" no cell does)."""
    previous = None
    for what, model, x, g, prm in _cache_steps(pset):
        exp = ic.oracle(model, prm, x, ic.rows(), g)
        if previous is not None:
            changed = ~((exp == previous) | (np.isnan(exp) & np.isnan(previous)))
            print(f"{pset}: {what}: {int(changed.sum())} of {changed.size} values change")
            assert changed.any(), what
        previous = exp


# ------------------------------------------------------------------------------------------------------------- GPU

@contextlib.contextmanager
def _region(geo, T, window=0, devices=None):
    from shyft_amd import synthetic
    from shyft_amd.region import HipRegion, PT_GS_K
    N = geo.shape[0]
    r = HipRegion(PT_GS_K, N, devices=devices) if devices is not None else HipRegion(PT_GS_K, N)
    try:
        r.set_geo(geo)
        r.set_parameters(synthetic.default_ptgsk_parameters())
        r.set_time_axis(synthetic.T0_2015_US, HOUR, T, window)
        yield r
    finally:
        r.close()


def _set_path(monkeypatch, path):
    if path == "tile":
        monkeypatch.setenv("SHYFT_IDW_TILE", "1")
    else:
        monkeypatch.delenv("SHYFT_IDW_TILE", raising=False)


def _run(r, model, xyz, vals, step0, prm, path, what):
    """One interpolate call; `path` is the gather it must report (a tuple: any of them). Returns the path."""
    var = ic.MODELS[model][0]
    r.interpolate(var, xyz, vals, step0, prm)
    ran = r.interpolation_path(var)
    allowed = path if isinstance(path, tuple) else (path,)
    assert ran in allowed, f"{what}: rows [{step0}, {step0 + len(vals)}) ran the {ran} gather, expected {path}"
    return ran


def _assert_bits(got, exp, what):
    """Bit for bit, NaN equal to NaN."""
    exp = np.ascontiguousarray(exp)
    got = np.ascontiguousarray(got)
    assert got.shape == exp.shape, f"{what}: shape {got.shape} != {exp.shape}"
    same = (got.view(np.int64) == exp.view(np.int64)) | (np.isnan(got) & np.isnan(exp))
    if not same.all():
        row, cell = (int(i) for i in np.argwhere(~same)[0])
        pytest.fail(f"{what}: {(~same).sum()} of {same.size} differ, first at row {row} cell {cell}: "
                    f"got {got[row, cell]!r}, oracle {exp[row, cell]!r}")


def _poison(r, var, step0, n):
    r.set_forcing(var, step0, np.full((n, r.n), POISON))


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["wave", "tile"])
@pytest.mark.parametrize("model", list(ic.MODELS))
def test_every_tier_and_model_bitexact(model, path, monkeypatch):
    """The full matrix on the S = 49 geometry: 9 max_members (all four register tiers, each at, below and above its
    size) x near / far, on the wavefront-union gather and the LDS row tiles. The 67 rows go in two calls, [0, 30)
    and [30, 67) (the second reuses the neighbour table), then once more in one call (two LDS tiles, the non-finite
    rows 63 | 64 on their boundary, a 3-row remainder)."""
    _set_path(monkeypatch, path)
    var, _, by_eq = ic.MODELS[model]
    xyz, vals, T = ic.stations(), ic.rows(), ic.T_ROWS
    with _region(ic.cells(), T) as r:
        for K in ic.K_VALUES:
            for pset in ("near", "far"):
                prm = ic.param(pset, K, by_eq)
                exp = ic.expected(model, K, pset)
                what = f"{model} K={K} {pset} {path}"
                _poison(r, var, 0, T)
                _run(r, model, xyz, vals[:30], 0, prm, path, what)
                _run(r, model, xyz, vals[30:], 30, prm, path, what)
                _assert_bits(r.get_forcing(var, 0, T), exp, what + " (two calls)")
                _poison(r, var, 0, T)
                _run(r, model, xyz, vals, 0, prm, path, what)
                _assert_bits(r.get_forcing(var, 0, T), exp, what + " (one call)")


@pytest.mark.gpu
@pytest.mark.parametrize("model", list(ic.MODELS))
def test_global_memory_rows_bitexact(model, monkeypatch):
    """S = 4100: a row does not fit the tile budget, so the tile kernel reads rows and coordinates from global memory
    (lds_rows == 0), every model at every register tier. Without SHYFT_IDW_TILE the launch picks its own gather
    (the wavefront unions where they fit 64 stations) and must match too."""
    var, _, by_eq = ic.MODELS[model]
    xyz, vals = ic.stations("large"), ic.rows("large")
    T = vals.shape[0]
    with _region(ic.cells(), T) as r:
        for K in (8, 12, 20, 32):
            for pset in ("near", "far"):
                prm = ic.param(pset, K, by_eq)
                exp = ic.expected(model, K, pset, "large")
                for path in ("tile", ("wave", "tile")):
                    _set_path(monkeypatch, path)
                    _poison(r, var, 0, T)
                    ran = _run(r, model, xyz, vals, 0, prm, path, f"{model} K={K} {pset} S=4100")
                    _assert_bits(r.get_forcing(var, 0, T), exp, f"{model} K={K} {pset} S=4100 {ran}")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["wave", "tile"])
@pytest.mark.parametrize("model", ["temperature", "temperature_eq", "precipitation"])
def test_short_calls_and_moved_window_bitexact(model, path, monkeypatch):
    """Calls of 1, 2, 3 and 5 rows (fewer than the wavefront gather's 4 prefetched rows, odd pairs), at step 0, 1, 3
    and 6 of the whole axis, and through an 11-row window moved to step 56: 5, 2 and 3 rows and a call whose only
    row is the all-NaN row 66."""
    _set_path(monkeypatch, path)
    var, _, by_eq = ic.MODELS[model]
    xyz, vals, T = ic.stations(), ic.rows(), ic.T_ROWS
    assert ic.ROW_ALL_NAN_2 == 66
    with _region(ic.cells(), T) as whole, _region(ic.cells(), T, window=11) as win:
        win.move_window(56, 1)
        for K in (8, 32):
            for pset in ("near", "far"):
                prm = ic.param(pset, K, by_eq)
                exp = ic.expected(model, K, pset)
                what = f"{model} K={K} {pset} {path}"
                _poison(whole, var, 0, 11)
                for step0, n in ((0, 1), (1, 2), (3, 3), (6, 5)):
                    _run(whole, model, xyz, vals[step0:step0 + n], step0, prm, path, what)
                _assert_bits(whole.get_forcing(var, 0, 11), exp[:11], what + " rows [0, 11)")
                _poison(win, var, 56, 11)
                for step0, n in ((66, 1), (56, 5), (63, 3), (61, 2)):
                    _run(win, model, xyz, vals[step0:step0 + n], step0, prm, path, what + " window at 56")
                _assert_bits(win.get_forcing(var, 56, 11), exp[56:], what + " window rows [56, 67)")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["wave", "tile"])
def test_table_cache_follows_every_input(path, monkeypatch, pset="near"):
    """One region, temperature, max_members 12: the neighbour table is cached on the stations and the selection
    parameters, not on default_gradient and gradient_by_equation (the gather reads those per call). Changing only
    one of them, then moving a station, then set_geo with every cell's elevation changed must each give the oracle's
    result for that call's inputs -- a stale table or stale coordinates would not."""
    _set_path(monkeypatch, path)
    vals, T = ic.rows(), ic.T_ROWS
    with _region(ic.cells(), T) as r:
        for what, model, x, g, prm in _cache_steps(pset):
            if what.startswith("set_geo"):
                r.set_geo(g)
            _poison(r, 0, 0, T)
            _run(r, model, x, vals, 0, prm, path, what)
            _assert_bits(r.get_forcing(0, 0, T), ic.oracle(model, prm, x, vals, g), f"{what} ({pset}, {path})")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["wave", "tile"])
def test_catchment_filter_bitexact(path, monkeypatch):
    """Unsharded interpolation under set_catchment_filter([1, 3]): catchment ids cycle 1, 2, 3 over the cells, so
    the filter's edge runs through every wavefront. Calculated cells equal the oracle, the others keep the NaN the
    window was filled with."""
    _set_path(monkeypatch, path)
    geo, xyz, vals, T = ic.cells(), ic.stations(), ic.rows(), ic.T_ROWS
    on = np.isin(geo[:, 4], [1, 3])
    assert 0 < on.sum() < ic.N_CELLS and all(0 < on[b:b + 64].sum() < on[b:b + 64].size for b in range(0, ic.N_CELLS, 64))
    with _region(geo, T) as r:
        r.set_catchment_filter([1, 3])
        for model in ("temperature", "radiation"):
            var = ic.MODELS[model][0]
            for K in (9, 32):
                for pset in ("near", "far"):
                    exp = np.where(on[None, :], ic.expected(model, K, pset), np.nan)
                    what = f"{model} K={K} {pset} {path} filter [1, 3]"
                    r.move_window(0, 1)     # NaN fill of the forcing window
                    _run(r, model, xyz, vals[:30], 0, ic.param(pset, K), path, what)
                    _run(r, model, xyz, vals[30:], 30, ic.param(pset, K), path, what)
                    _assert_bits(r.get_forcing(var, 0, T), exp, what)
        r.set_catchment_filter([])          # filter off again: every cell is calculated
        _poison(r, 0, 0, T)
        _run(r, "temperature", xyz, vals, 0, ic.param("near", 9), path, "filter removed")
        _assert_bits(r.get_forcing(0, 0, T), ic.expected("temperature", 9, "near"), f"filter removed ({path})")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["wave", "tile"])
def test_single_source(path, monkeypatch):
    """One station: temperature is a clean copy of its row to every calculated cell, whatever the distance (path
    "copy"; region_model.h:470-481), with or without gradient_by_equation; under a catchment filter the other cells
    stay NaN. The same single station for precipitation takes the normal gather and equals the oracle (cells out of
    its reach: NaN)."""
    _set_path(monkeypatch, path)
    geo = ic.cells()
    xyz = ic.stations()[8:9]
    vals = np.array([[3.25], [-1.5], [np.nan], [0.0], [7.125]])
    T = vals.shape[0]
    copied = np.repeat(vals, ic.N_CELLS, axis=1)
    on = np.isin(geo[:, 4], [1, 3])
    with _region(geo, T) as r:
        for model in ("temperature", "temperature_eq"):
            _poison(r, 0, 0, T)
            _run(r, model, xyz, vals, 0, ic.param("near", 8, ic.MODELS[model][2]), "copy", model + " single source")
            _assert_bits(r.get_forcing(0, 0, T), copied, model + " single source")
        for K, pset in ((8, "near"), (32, "far"), (1, "near")):
            prm = ic.param(pset, K)
            exp = ic.oracle("precipitation", prm, xyz, vals, geo)
            assert np.isfinite(exp[0]).any() and np.isnan(exp[0]).any()
            _poison(r, 1, 0, T)
            _run(r, "precipitation", xyz, vals, 0, prm, path, "precipitation single source")
            _assert_bits(r.get_forcing(1, 0, T), exp, f"precipitation single source K={K} {pset} {path}")
        r.set_catchment_filter([1, 3])
        r.move_window(0, 1)
        _run(r, "temperature", xyz, vals, 0, ic.param("near", 8), "copy", "single source, filter")
        _assert_bits(r.get_forcing(0, 0, T), np.where(on[None, :], copied, np.nan), "single source, filter [1, 3]")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["wave", "tile"])
def test_two_shards_on_one_device_bitexact(path, monkeypatch):
    """HipRegion(devices=[0, 0]): two shards of the edge cells, far, max_members 32 -- each shard builds its own
    neighbour table and wavefront unions over its cells. Equal to the unsharded region and to the oracle."""
    _set_path(monkeypatch, path)
    geo, xyz, vals, T = ic.cells(), ic.stations(), ic.rows(), ic.T_ROWS
    with _region(geo, T) as one, _region(geo, T, devices=[0, 0]) as two:
        assert len(two.shards()) == 2 and len(one.shards()) == 1
        for model in ("temperature", "precipitation"):
            var = ic.MODELS[model][0]
            prm = ic.param("far", 32)
            got = []
            for r in (one, two):
                _poison(r, var, 0, T)
                _run(r, model, xyz, vals[:30], 0, prm, path, f"{model} {len(r.shards())} shard(s)")
                _run(r, model, xyz, vals[30:], 30, prm, path, f"{model} {len(r.shards())} shard(s)")
                got.append(r.get_forcing(var, 0, T))
            _assert_bits(got[0], ic.expected(model, 32, "far"), f"{model} unsharded {path}")
            _assert_bits(got[1], ic.expected(model, 32, "far"), f"{model} two shards {path}")
            _assert_bits(got[1], got[0], f"{model} two shards against unsharded {path}")
