"""Cell percentiles on the GPU (shyft_hip_percentiles / shyft_hip_catchment_percentiles, kernels/percentiles.hip;
calculate_percentiles, core/time_series_statistics.h:112-246) against the host restatement
shyft_hip_percentiles_host, which tests/test_percentiles_host.py pins to the reference's rules.

Crafted values are written into a forcing series, so no model run is needed. Every entry but AVERAGE must be
bit-identical to the host (zeros compared numerically: +0.0 and -0.0 are equal in a sort). AVERAGE sums the same
finite samples in another order, so |device - host| <= 2 n 2^-53 sum|x_i| (each order is within (n-1) u sum|x| of
the exact sum); the bound is computed from the data of each step."""
import numpy as np
import pytest

from shyft_amd import synthetic
from shyft_amd._native import ShyftHipError
from shyft_amd.region import (KNOB_PERCENTILES_PATH, PERCENTILES_LDS_MAX, PERCENTILES_MAX, SCOPE_CATCHMENT,
                              SCOPE_CELL_IX, SERIES_FORCING, percentiles_host)

pytestmark = pytest.mark.gpu

N, T = 20480, 304
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 20011]
PCTS = [-1000, 0, 1, 10, 50, -1, 70, 99, 100, 1000, 101, -5, 50, 0]  # the list of the host test
AUTO, LDS, RADIX = 0, 1, 2
KINDS = 8


def crafted(n_steps, n, seed):
    """[n_steps][n]: the value sets a radix select goes wrong on, one kind per step (t % KINDS)."""
    rng = np.random.default_rng(seed)
    v = np.empty((n_steps, n))
    for t in range(n_steps):
        k = t % KINDS
        if k == 0:    # wide range of magnitudes, both signs
            v[t] = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, size=n)
        elif k == 1:  # all equal
            v[t] = 2.5 + t
        elif k == 2:  # three distinct values
            v[t] = rng.choice([-1.5, 0.25, 7.0], n)
        elif k == 3:  # equal in the top 56 bits, differing in the last byte only
            bits = np.uint64(0x400921FB54442D00) | rng.integers(0, 256, size=n).astype(np.uint64)
            v[t] = bits.view(np.float64)
        elif k == 4:  # mixed signs with subnormals and +-0
            x = rng.normal(size=n)
            x[rng.random(n) < 0.3] = 0.0
            x[rng.random(n) < 0.2] = -0.0
            sub = rng.random(n) < 0.3
            x[sub] = rng.integers(-1000, 1000, size=int(sub.sum())) * 5e-324
            v[t] = x
        elif k == 5:  # +-inf and NaN sprinkled in
            x = rng.normal(size=n) * 100.0
            x[rng.random(n) < 0.2] = np.nan
            x[rng.random(n) < 0.1] = np.inf
            x[rng.random(n) < 0.1] = -np.inf
            v[t] = x
        elif k == 6:  # an all-NaN step among finite ones
            v[t] = np.nan
        else:         # exactly one finite sample (cell 0 is in every selection of these tests)
            v[t] = np.nan
            v[t, 0] = -3.75
            v[t, 1::7] = np.inf
    return v


def make_region(n, geo):
    from shyft_amd.region import HipRegion, PT_GS_K
    r = HipRegion(PT_GS_K, n)
    r.set_geo(geo)
    r.set_time_axis(synthetic.T0_2015_US, synthetic.HOUR_US, T)
    return r


@pytest.fixture(scope="module")
def region():
    geo = synthetic.geo11(N, n_catchments=5)
    geo[:, 4] = 1 + (np.arange(N) * 5) // N  # five contiguous catchments, cell 0 in catchment 1
    r = make_region(N, geo)
    values = crafted(T, N, 1)
    r.set_forcing(0, 0, values)
    yield r, geo, values
    r.close()


def check(got, rows, pcts):
    """got [n_pct][n] against the host restatement of rows [n][n_samples]"""
    want = percentiles_host(rows, pcts)
    assert got.shape == want.shape
    fin = np.isfinite(rows)
    absum = np.where(fin, np.abs(np.where(fin, rows, 0.0)), 0.0).sum(axis=1)
    bound = 2.0 * fin.sum(axis=1) * 2.0 ** -53 * absum
    for k, p in enumerate(pcts):
        g, w = got[k], want[k]
        if p == -1:
            both_nan = np.isnan(g) & np.isnan(w)
            d = np.abs(np.where(both_nan, 0.0, g - w))
            print(f"AVERAGE: max |device - host| {np.nanmax(d):.3e}, max bound {bound.max():.3e}")
            assert np.all(both_nan | (d <= bound)), (k, p, g, w, bound)
        else:
            same = (g.view(np.int64) == w.view(np.int64)) | ((g == 0) & (w == 0)) | (np.isnan(g) & np.isnan(w))
            assert np.all(same), (k, p, np.flatnonzero(~same)[:5], g[~same][:5], w[~same][:5])


def strided(size):
    return (np.arange(size) * (N // size if size * 2 <= N else 1)).astype(np.int64)  # non-identity, starts at cell 0


@pytest.mark.parametrize("knob", [AUTO, LDS, RADIX])
@pytest.mark.parametrize("size", SIZES)
def test_selection_sizes_and_paths(region, size, knob):
    r, _, values = region
    sel = strided(size)
    if size == 20011:  # no stride fits: drop a spread of cells instead (still not the identity)
        sel = np.delete(np.arange(N), np.arange(1, N, 43)[:N - size]).astype(np.int64)
    assert sel.size == size and sel[0] == 0
    fits = size <= PERCENTILES_LDS_MAX
    r.set_test_knob(KNOB_PERCENTILES_PATH, knob)
    try:
        if knob == LDS and not fits:
            with pytest.raises(ShyftHipError, match="LDS sort path is forced"):
                r.percentiles(SERIES_FORCING + 0, PCTS, sel, SCOPE_CELL_IX, 0, 3)
            return
        got = r.percentiles(SERIES_FORCING + 0, PCTS, sel, SCOPE_CELL_IX, 0, 300)
        assert r.percentiles_path() == ("radix" if knob == RADIX or (knob == AUTO and not fits) else "lds_sort")
    finally:
        r.set_test_knob(KNOB_PERCENTILES_PATH, AUTO)
    check(got, values[:300][:, sel], PCTS)


@pytest.mark.parametrize("knob", [AUTO, RADIX])
@pytest.mark.parametrize("step0,n", [(0, 1), (5, 3), (3, 1)])
def test_step_windows(region, step0, n, knob):
    r, _, values = region
    r.set_test_knob(KNOB_PERCENTILES_PATH, knob)
    try:
        for size in (257, 4097):
            sel = strided(size)
            got = r.percentiles(SERIES_FORCING + 0, PCTS, sel, SCOPE_CELL_IX, step0, n)
            check(got, values[step0:step0 + n][:, sel], PCTS)
    finally:
        r.set_test_knob(KNOB_PERCENTILES_PATH, AUTO)


@pytest.mark.parametrize("knob", [AUTO, RADIX])
def test_catchment_scope_and_all_cells(region, knob):
    r, geo, values = region
    r.set_test_knob(KNOB_PERCENTILES_PATH, knob)
    try:
        got = r.percentiles(SERIES_FORCING + 0, PCTS, [1, 4], SCOPE_CATCHMENT, 0, 24)  # two of five catchments
        assert r.percentiles_path() == "radix"
        check(got, values[:24][:, np.isin(geo[:, 4], [1, 4])], PCTS)
        got = r.percentiles(SERIES_FORCING + 0, PCTS, [], SCOPE_CATCHMENT, 0, 24)      # all cells: the identity
        check(got, values[:24], PCTS)
    finally:
        r.set_test_knob(KNOB_PERCENTILES_PATH, AUTO)


def test_percentile_lists(region):
    r, _, values = region
    sel = strided(1025)
    at_cap = [0, 3, 5, 10, 20, 25, 33, 50, -1, 66, 75, 90, 95, 100, -1000, 1000]
    assert len(at_cap) == PERCENTILES_MAX
    for knob in (AUTO, RADIX):
        r.set_test_knob(KNOB_PERCENTILES_PATH, knob)
        try:
            check(r.percentiles(SERIES_FORCING + 0, at_cap, sel, SCOPE_CELL_IX, 0, 16), values[:16][:, sel], at_cap)
            check(r.percentiles(SERIES_FORCING + 0, [-1], sel, SCOPE_CELL_IX, 0, 16), values[:16][:, sel], [-1])
            with pytest.raises(ShyftHipError, match="the maximum is 16"):
                r.percentiles(SERIES_FORCING + 0, at_cap + [1], sel, SCOPE_CELL_IX, 0, 16)
            assert r.percentiles(SERIES_FORCING + 0, [], sel, SCOPE_CELL_IX, 0, 16).shape == (0, 16)
        finally:
            r.set_test_knob(KNOB_PERCENTILES_PATH, AUTO)
    with pytest.raises(ShyftHipError, match="the maximum is 16"):
        r.catchment_percentiles(SERIES_FORCING + 0, at_cap + [1], 0, 4)
    assert r.catchment_percentiles(SERIES_FORCING + 0, [], 0, 4).shape == (5, 0, 4)


def test_errors_as_statistics(region):
    r, _, _ = region
    with pytest.raises(ShyftHipError, match="one or more supplied catchment_indexes does not exist:9"):
        r.percentiles(SERIES_FORCING + 0, [50], [1, 9], SCOPE_CATCHMENT, 0, 4)
    with pytest.raises(ShyftHipError, match="is ouside valid range"):
        r.percentiles(SERIES_FORCING + 0, [50], [N + 5], SCOPE_CELL_IX, 0, 4)
    with pytest.raises(ShyftHipError, match="outside the resident window"):
        r.percentiles(SERIES_FORCING + 0, [50], [0], SCOPE_CELL_IX, T - 2, 4)
    with pytest.raises(ShyftHipError, match="percentiles path must be"):
        r.set_test_knob(KNOB_PERCENTILES_PATH, 3)


def test_sharded_region_is_refused():
    from shyft_amd.region import HipRegion, PT_GS_K
    n = 64
    r = HipRegion(PT_GS_K, n, devices=[0, 0])
    try:
        r.set_geo(synthetic.geo11(n, n_catchments=2))
        r.set_time_axis(synthetic.T0_2015_US, synthetic.HOUR_US, 4)
        with pytest.raises(ShyftHipError, match="percentiles: not available for a sharded region"):
            r.percentiles(SERIES_FORCING + 0, [50], [], SCOPE_CATCHMENT, 0, 4)
        with pytest.raises(ShyftHipError, match="percentiles: not available for a sharded region"):
            r.catchment_percentiles(SERIES_FORCING + 0, [50], 0, 4)
    finally:
        r.close()


@pytest.fixture(scope="module", params=["contiguous", "interleaved"])
def catchments(request):
    n = 9001
    geo = synthetic.geo11(n, n_catchments=4)
    if request.param == "contiguous":
        cid = 1 + (np.arange(n) * 3) // (n - 1)   # three contiguous ranges, then catchment 4 = the last cell alone
    else:
        cid = np.random.default_rng(5).choice([3, 1, 2], n)
        cid[0] = 3
        cid[4321] = 4                              # a catchment of one cell
    geo[:, 4] = cid
    r = make_region(n, geo)
    values = crafted(T, n, 2)
    r.set_forcing(1, 0, values)
    yield r, cid, values
    r.close()


@pytest.mark.parametrize("knob", [AUTO, LDS, RADIX])
def test_catchment_percentiles(catchments, knob):
    import torch
    r, cid, values = catchments
    series, n = SERIES_FORCING + 1, 40
    pcts = [0, 25, 50, -1, 75, 100, -1000, 1000]
    cids = [int(c) for c in r.catchment_ids()]
    assert len(cids) == 4 and int((cid == 4).sum()) == 1
    r.set_test_knob(KNOB_PERCENTILES_PATH, knob)
    try:
        got = r.catchment_percentiles(series, pcts, 8, n)
        assert r.percentiles_path() == ("radix" if knob == RADIX else "lds_sort")
        dev = torch.full((len(cids), len(pcts), n), 7.0, dtype=torch.float64, device="cuda")
        r.catchment_percentiles_device(series, pcts, 8, n, dev.data_ptr())
        assert np.array_equal(dev.cpu().numpy().view(np.int64), got.view(np.int64))  # dst_on_device both ways
        for k, c in enumerate(cids):
            one = r.percentiles(series, pcts, [c], SCOPE_CATCHMENT, 8, n)
            # same segment, same order: bitwise, AVERAGE included
            assert np.array_equal(one.view(np.int64), got[k].view(np.int64)), (c, one, got[k])
            check(got[k], values[8:8 + n][:, cid == c], pcts)
    finally:
        r.set_test_knob(KNOB_PERCENTILES_PATH, AUTO)


def test_model_statistics_percentiles():
    """pt_gs_k 20 x 240 (tests/golden/pt_gs_k_20x240.npz) through shyft_amd.api: statistics.<name>_percentiles
    against the host restatement of the cells' series; a state series has T + 1 points."""
    import os
    from shyft_amd import api
    from shyft_amd.api import pt_gs_k
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pt_gs_k_20x240.npz"))
    geo, forcing = g["geo"], g["forcing"]
    n, steps = geo.shape[0], forcing.shape[1]
    gcds = api.GeoCellDataVector()
    for row in geo:
        ltf = api.LandTypeFractions(row[6], row[7], row[8], row[9], row[10])
        gcds.append(api.GeoCellData(api.GeoPoint(row[0], row[1], row[2]), row[3], int(row[4]), row[5], ltf))
    p = pt_gs_k.PTGSKParameter()
    p.set(list(g["params"].ravel()[:p.size()]))
    model = pt_gs_k.PTGSKModel(gcds, p)
    ta = api.TimeAxisFixedDeltaT(int(g["t0_us"]) // 1000000, int(g["dt_us"]) // 1000000, steps)
    model.initialize_cell_environment(ta)
    for v in range(5):
        for c in range(n):
            model._set_cell_forcing(v, c, forcing[v][:, c].tolist())
    s0 = pt_gs_k.PTGSKStateVector(pt_gs_k.PTGSKState(row) for row in g["state0"])
    model.set_states(s0)
    model.set_state_collection(-1, True)
    model.run_cells()
    pcts = [0, 25, 50, -1, 75, 100]
    all_cids = [int(c) for c in model.catchment_ids]
    for cids in (all_cids[:2], []):
        cells = [c for c in range(n) if not cids or int(geo[c, 4]) in cids]
        r = model.statistics.discharge_percentiles(api.IntVector(cids), api.IntVector(pcts))
        assert isinstance(r, api.TsVector) and len(r) == len(pcts) and r[0].size() == steps
        rows = np.stack([model._cell_series(0, c) for c in cells], axis=1)
        check(np.array([ts.values for ts in r]), rows, pcts)
    by_cell = model.statistics.temperature_percentiles(api.IntVector([0, 3, 7]), [50], api.stat_scope.cell)
    rows = np.stack([model._cell_series(api.SERIES_FORCING + 0, c) for c in (0, 3, 7)], axis=1)
    check(np.array([ts.values for ts in by_cell]), rows, [50])
    st = model.kirchner_state.discharge_percentiles(api.IntVector(), [0, 50, 100])  # a state series: T + 1 points
    assert st[1].size() == steps + 1
    rows = np.stack([model._cell_series(api.SERIES_STATE + 0, c) for c in range(n)], axis=1)
    check(np.array([ts.values for ts in st]), rows, [0, 50, 100])
    per_catchment = model.catchment_percentiles("avg_discharge", pcts)
    assert len(per_catchment) == len(all_cids)
    for c, tsv in zip(all_cids, per_catchment):
        one = model.statistics.discharge_percentiles(api.IntVector([c]), pcts)
        assert [list(a.values) for a in tsv] == [list(b.values) for b in one]
    with pytest.raises(AttributeError):
        model.actual_evaptranspiration_response.pot_ratio_percentiles
    with pytest.raises(AttributeError):
        model.statistics.total_area_percentiles
