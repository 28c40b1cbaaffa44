"""kernels/stats.hip at its edges: every segment_sum_kernel instance, both select_sum_kernel branches and the
grid-stride tails of nan_scan_kernel and fill_kernel, bit for bit against the plain restatements of
tests/reduce_cases.py, which the CPU tests below hold within a derived bound of the exact sum.

The values are planted as forcing (statistics, catchment_sums and catchment_area_sums accept SERIES_FORCING + v), so
no model runs except where routing group sums need discharge. The segment sizes are reduce_cases.SIZES: the sizes at
which the lane stride, the wavefront butterfly and the four-loads-ahead loop change behaviour, on two layouts
(contiguous catchments: the index array is not read; the same sizes dealt through a permutation: the indexed path).

The bound of the restatement against the exact sum: a term passes ceil(n/256) - 1 adds in its lane, 6 butterfly levels
and 3 wavefront adds, one spare: |got - exact| <= (ceil(n/256) + 9) 2^-53 sum|x|; the weighted form rounds each product
first: + 10, against the exact sum of the exact products. The planted rows stay below 0.13 of it."""
import ctypes as C
import math

import numpy as np
import pytest

from shyft_amd import synthetic
from tests import reduce_cases as rc

T_EDGE = 7
SENTINEL = -12345.0
V_SPECIAL = 3  # the forcing variable whose first rows carry the special values
NAN_CID, INF_NAN_CID, INF_CID = 1, 2, 77  # the 257-, 1025- and 768-cell catchments
V_LANE0, ROW_LANE0, LANE0_CID = 4, 5, 23   # see planted_forcing
LANE0_TERMS = [0, 256, 512, 768]           # lane 0's terms of a 769-cell segment


def planted_forcing(cid):
    """[5][T_EDGE][N_CELLS] planted values; variable V_SPECIAL carries, in the layout given by cid: row 0 a NaN in the
    last cell of the 257-cell catchment, row 1 +inf and -inf in different lanes of one catchment and a lone +inf in
    another, row 2 all -0.0. Row ROW_LANE0 of variable V_LANE0: in the 769-cell catchment only lane 0 enters the
    four-loads-ahead loop, and its partial sum is small next to the others', so the order of its four adds would hide in
    the later roundings; there its terms are 2^60, 1, -2^60, 1, which give 1.0 in order and 0.0 reversed."""
    F = np.stack([rc.planted(T_EDGE, rc.N_CELLS, 300 + v) for v in range(5)])
    F[V_LANE0][ROW_LANE0, np.flatnonzero(cid == LANE0_CID)[LANE0_TERMS]] = [2.0 ** 60, 1.0, -2.0 ** 60, 1.0]
    s = F[V_SPECIAL]
    s[0, np.flatnonzero(cid == NAN_CID)[-1]] = np.nan
    c = np.flatnonzero(cid == INF_NAN_CID)
    s[1, c[3]], s[1, c[70]] = np.inf, -np.inf          # lanes 3 and 70: they meet in the last wavefront add
    s[1, np.flatnonzero(cid == INF_CID)[300]] = np.inf
    s[2, :] = -0.0
    return F


_cases = {}


def case(kind):
    """(cid [N], areas [N], forcing [5][T][N]) of a layout, built once and read-only"""
    if kind not in _cases:
        cid = rc.layout(kind)
        areas = rc.planted_areas(rc.N_CELLS)
        F = planted_forcing(cid)
        for a in (cid, areas, F):
            a.setflags(write=False)
        _cases[kind] = (cid, areas, F)
    return _cases[kind]


def expected_sums(rows, cid, order, areas=None):
    """[catchment][step] restated segment sums of rows [T][N]; order = the catchment ids in output order"""
    out = np.empty((len(order), rows.shape[0]))
    for k, c in enumerate(order):
        cells = np.flatnonzero(cid == c)  # segment order: cell order
        out[k] = rc.device_order_sum(rows[:, cells], None if areas is None else areas[cells])
    return out


def same_bits(a, b):
    """equal values (NaN equal to NaN) and, where zero, the same sign"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and \
        np.array_equal(np.signbit(a[a == 0]), np.signbit(b[b == 0]))


# ---------------------------------------------------------------- CPU: the restatements themselves

@pytest.mark.parametrize("kind", rc.LAYOUTS)
@pytest.mark.parametrize("size", rc.SIZES)
def test_restated_sum_within_bound_of_exact(size, kind):
    cid, areas, F = case(kind)
    cells = np.flatnonzero(cid == rc.CIDS[rc.SIZES.index(size)])
    assert cells.size == size
    rows = F[0][:, cells]
    got, got_w = rc.device_order_sum(rows), rc.device_order_sum(rows, areas[cells])
    worst = 0.0
    for t in range(T_EDGE):
        exact, mag = rc.exact_sum(rows[t])
        bound = (math.ceil(size / 256) + 9) * rc.U * mag
        assert abs(got[t] - exact) <= bound
        exact_w, mag_w = rc.exact_sum(rows[t], areas[cells])
        bound_w = (math.ceil(size / 256) + 10) * rc.U * mag_w
        assert abs(got_w[t] - exact_w) <= bound_w
        worst = max(worst, abs(got[t] - exact) / bound, abs(got_w[t] - exact_w) / bound_w)
    print(f"n={size} {kind}: largest |error| / bound = {worst:.3f}")


@pytest.mark.parametrize("kind", rc.LAYOUTS)
@pytest.mark.parametrize("size", [s for s in rc.SIZES if s >= 63])
def test_planted_rows_tell_device_order_from_sequential_order(size, kind):
    """at least one of the T planted rows differs in bits between the device order and a left-to-right sum, so a
    bit-exact match pins the order and not just the value"""
    cid, areas, F = case(kind)
    cells = np.flatnonzero(cid == rc.CIDS[rc.SIZES.index(size)])
    rows = F[0][:, cells]
    dev, dev_w = rc.device_order_sum(rows), rc.device_order_sum(rows, areas[cells])
    assert any(dev[t] != rc.sequential_sum(rows[t]) for t in range(T_EDGE))
    assert any(dev_w[t] != rc.sequential_sum(rows[t] * areas[cells]) for t in range(T_EDGE))


def test_restated_sum_of_the_old_form_is_unchanged():
    """device_order_sum term by term, as tests/test_segment_sums.py stated it before it moved"""
    vals = rc.planted(1, 1300, 9)[0]
    acc = [0.0] * rc.RB
    for k, v in enumerate(vals.tolist()):
        acc[k % rc.RB] += v
    w = np.array(acc).reshape(rc.RB // 64, 64)
    lanes = np.arange(64)
    off = 32
    while off:
        w = w + w[:, lanes ^ off]
        off >>= 1
    r = w[0, 0]
    for p in w[1:, 0]:
        r = r + p
    assert rc.device_order_sum(vals) == r


@pytest.mark.parametrize("kind", rc.LAYOUTS)
def test_planted_row_tells_the_order_of_lane_0_at_769_cells(kind):
    cid, _, F = case(kind)
    assert rc.size_of_cid(LANE0_CID) == 769
    vals = F[V_LANE0][ROW_LANE0, np.flatnonzero(cid == LANE0_CID)]
    backwards = vals.copy()
    backwards[LANE0_TERMS] = vals[LANE0_TERMS[::-1]]       # lane 0 adding its four loads last to first
    assert rc.device_order_sum(vals) - rc.device_order_sum(backwards) == 1.0


def selections(k):
    """{name: cell indices} that select k cells: a prefix, a strided set, an unordered list with duplicates"""
    rng = np.random.default_rng(1000 + k)
    pick = rng.permutation(rng.choice(rc.N_CELLS, k, replace=False))
    return {"prefix": np.arange(k), "strided": 3 + 5 * np.arange(k),
            "unordered": np.concatenate([pick, pick[: max(1, k // 3)], pick[:1]])}


SELECTION_SIZES = [1, 255, 256, 257, 1025]


@pytest.mark.parametrize("k", SELECTION_SIZES)
def test_strided_selection_tells_position_weights_from_cell_weights(k):
    """select_sum_kernel weights by selection position (w[k], gathered on the host), the segment kernel by cell
    (w[i]): on the strided selection, weighting by the first k cells' areas instead gives other bits."""
    _, areas, F = case("contiguous")
    sel = selections(k)["strided"]
    right = rc.select_order_sum(F[1], sel, areas)
    confused = rc.device_order_sum(F[1][:, sel], areas[:k])
    assert np.all(right != confused)
    assert len(np.unique(selections(k)["unordered"])) == k


# ---------------------------------------------------------------- GPU

def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def seg_sums(r, entry, series, step0, n, rows):
    """a raw [rows][n] segment-sum entry on a sentinel-filled host array"""
    out = np.full((rows, n), SENTINEL)
    r._chk(getattr(r._L, entry)(r.h, series, step0, n, _ptr(out), 0))
    return out


def group_sums(r, step0, n):
    out = np.full((r.n_route_groups, n), SENTINEL)
    r._chk(r._L.shyft_hip_routing_group_sums(r.h, step0, n, _ptr(out), 0))
    return out


def stat(r, series, ids, scope, weighted, step0=0, n=T_EDGE):
    i = np.ascontiguousarray(list(ids), dtype=np.int64)
    out = np.full(n, SENTINEL)
    r._chk(r._L.shyft_hip_statistics(r.h, series, _ptr(i) if i.size else None, i.size, scope, int(weighted), step0, n,
                                     _ptr(out)))
    return out


def forcing_ok(r):
    ok = C.c_int(-1)
    r._chk(r._L.shyft_hip_forcing_ok(r.h, C.byref(ok)))
    assert ok.value in (0, 1)
    return bool(ok.value)


def new_region(n, T, geo, collect):
    from shyft_amd.region import HipRegion, PT_GS_K
    r = HipRegion(PT_GS_K, n)
    r.set_geo(geo)
    r.set_parameters(synthetic.default_ptgsk_parameters())
    r.set_collection(collect)
    r.set_time_axis(synthetic.T0_2015_US, synthetic.HOUR_US, T)
    return r


@pytest.fixture(scope="module", params=rc.LAYOUTS)
def edge(request):
    """a region of reduce_cases.N_CELLS cells in the layout, the planted values as its forcing; no model run"""
    from shyft_amd.region import COLLECT_DISCHARGE
    cid, areas, F = case(request.param)
    geo = synthetic.geo11(rc.N_CELLS, n_catchments=3)
    geo[:, 4] = cid
    geo[:, 3] = areas
    r = new_region(rc.N_CELLS, T_EDGE, geo, COLLECT_DISCHARGE)
    for v in range(5):
        r.set_forcing(v, 0, F[v])
    yield r, cid, areas, F, [int(c) for c in r.catchment_ids()]
    r.close()


@pytest.mark.gpu
def test_catchment_sums_every_size_class(edge):
    from shyft_amd.region import SERIES_FORCING
    r, cid, _, F, order = edge
    assert sorted(order) == sorted(rc.CIDS)
    for v in (0, 4):
        got = seg_sums(r, "shyft_hip_catchment_sums", SERIES_FORCING + v, 0, T_EDGE, len(order))
        assert np.array_equal(got, expected_sums(F[v], cid, order))
        got = seg_sums(r, "shyft_hip_catchment_sums", SERIES_FORCING + v, 2, 3, len(order))
        assert np.array_equal(got, expected_sums(F[v][2:5], cid, order))
    assert np.array_equal(r.catchment_sums(SERIES_FORCING + 1, 0, T_EDGE), expected_sums(F[1], cid, order))


@pytest.mark.gpu
def test_catchment_area_sums_every_size_class(edge):
    """the two weighted segment_sum_kernel instances: value times the cell's own area (geo[:, 3] unchanged), rounded,
    then the same reduction"""
    from shyft_amd.region import SERIES_FORCING
    r, cid, areas, F, order = edge
    for v in (1, 2):
        got = seg_sums(r, "shyft_hip_catchment_area_sums", SERIES_FORCING + v, 0, T_EDGE, len(order))
        assert np.array_equal(got, expected_sums(F[v], cid, order, areas))
    got = seg_sums(r, "shyft_hip_catchment_area_sums", SERIES_FORCING + 2, 2, 3, len(order))
    assert np.array_equal(got, expected_sums(F[2][2:5], cid, order, areas))


@pytest.mark.gpu
def test_statistics_catchment_scope(edge):
    from shyft_amd.region import SERIES_FORCING, SCOPE_CATCHMENT, SCOPE_CELL_IX
    r, cid, areas, F, _ = edge
    for ids in ([], [42], [7], [1, 31], [31, 7, 42], list(rc.CIDS), [2, 2, 64]):
        sel = np.flatnonzero(np.isin(cid, ids)) if ids else np.arange(rc.N_CELLS)
        got = stat(r, SERIES_FORCING + 0, ids, SCOPE_CATCHMENT, False)
        assert np.array_equal(got, rc.select_order_sum(F[0], sel)), ids
        got = stat(r, SERIES_FORCING + 1, ids, SCOPE_CATCHMENT, True)
        want = rc.select_order_sum(F[1], sel, areas) * (1 / rc.sequential_sum(areas[sel]))
        assert np.array_equal(got, want), ids
    assert np.array_equal(stat(r, SERIES_FORCING + 2, [], SCOPE_CELL_IX, False), rc.select_order_sum(F[2]))   # [] = all
    got = stat(r, SERIES_FORCING + 4, [11, 3], SCOPE_CATCHMENT, False, step0=2, n=3)
    assert np.array_equal(got, rc.select_order_sum(F[4][2:5], np.flatnonzero(np.isin(cid, [11, 3]))))


@pytest.mark.gpu
@pytest.mark.parametrize("k", SELECTION_SIZES)
def test_statistics_cell_index_selections(edge, k):
    from shyft_amd.region import SERIES_FORCING, SCOPE_CELL_IX
    r, _, areas, F, _ = edge
    for name, ids in selections(k).items():
        sel = np.unique(ids)
        assert sel.size == k
        got = stat(r, SERIES_FORCING + 0, ids, SCOPE_CELL_IX, False)
        assert np.array_equal(got, rc.select_order_sum(F[0], ids)), name
        got = stat(r, SERIES_FORCING + 1, ids, SCOPE_CELL_IX, True)
        want = rc.select_order_sum(F[1], ids, areas) * (1 / rc.sequential_sum(areas[sel]))
        assert np.array_equal(got, want), name


@pytest.mark.gpu
def test_statistics_cell_index_n_is_accepted_like_the_reference(edge):
    """cell_statistics::verify_cids_exist (core/cell_model.h:202) refuses an index only when it is above the number of
    cells, so n itself passes and matches no cell: the sum is over the other indices (0.0 when there are none, where
    the reference returns an empty series), the average over nothing is NaN."""
    from shyft_amd._native import ShyftHipError
    from shyft_amd.region import SERIES_FORCING, SCOPE_CELL_IX
    r, _, areas, F, _ = edge
    n = rc.N_CELLS
    got = stat(r, SERIES_FORCING + 0, [n], SCOPE_CELL_IX, False)
    assert np.all(got == 0.0) and not np.signbit(got).any()
    assert np.isnan(stat(r, SERIES_FORCING + 0, [n], SCOPE_CELL_IX, True)).all()
    assert np.array_equal(stat(r, SERIES_FORCING + 0, [5, n, n - 1], SCOPE_CELL_IX, False),
                          rc.select_order_sum(F[0], [5, n - 1]))
    assert np.array_equal(stat(r, SERIES_FORCING + 1, [n, 5], SCOPE_CELL_IX, True),
                          rc.select_order_sum(F[1], [5], areas) * (1 / areas[5]))
    with pytest.raises(ShyftHipError, match="is ouside valid range"):
        stat(r, SERIES_FORCING + 0, [n + 1], SCOPE_CELL_IX, False)
    with pytest.raises(ShyftHipError, match="is ouside valid range"):
        stat(r, SERIES_FORCING + 0, [-1], SCOPE_CELL_IX, False)


@pytest.mark.gpu
def test_special_values_stay_in_their_catchment(edge):
    from shyft_amd.region import SERIES_FORCING, SCOPE_CATCHMENT
    r, cid, areas, F, order = edge
    clean = rc.planted(T_EDGE, rc.N_CELLS, 300 + V_SPECIAL)   # the variable before the special values went in
    for entry, w in (("shyft_hip_catchment_sums", None), ("shyft_hip_catchment_area_sums", areas)):
        got = seg_sums(r, entry, SERIES_FORCING + V_SPECIAL, 0, T_EDGE, len(order))
        assert same_bits(got, expected_sums(F[V_SPECIAL], cid, order, w)), entry
        by_cid = dict(zip(order, got))
        assert np.isnan(by_cid[NAN_CID][0]) and np.isnan(by_cid[INF_NAN_CID][1]) and by_cid[INF_CID][1] == np.inf
        assert np.all(got[:, 2] == 0.0) and not np.signbit(got[:, 2]).any()   # lanes start at +0.0: -0.0 sums to +0.0
        others = expected_sums(clean, cid, order, w)
        for k, c in enumerate(order):
            rows = [t for t in range(T_EDGE) if t != 2 and (c, t) not in ((NAN_CID, 0), (INF_NAN_CID, 1), (INF_CID, 1))]
            assert np.array_equal(got[k, rows], others[k, rows]), (entry, c)
    got = stat(r, SERIES_FORCING + V_SPECIAL, [NAN_CID, 42], SCOPE_CATCHMENT, False)
    assert same_bits(got, rc.select_order_sum(F[V_SPECIAL], np.flatnonzero(np.isin(cid, [NAN_CID, 42]))))
    assert np.isnan(got[0]) and got[2] == 0.0 and not np.signbit(got[2])
    got = stat(r, SERIES_FORCING + V_SPECIAL, [INF_CID], SCOPE_CATCHMENT, True)
    sel = np.flatnonzero(cid == INF_CID)
    assert same_bits(got, rc.select_order_sum(F[V_SPECIAL], sel, areas) * (1 / rc.sequential_sum(areas[sel])))
    assert got[1] == np.inf


@pytest.mark.gpu
def test_catchment_sums_into_device_memory(edge):
    import torch
    from shyft_amd.region import SERIES_FORCING
    r, _, _, _, order = edge
    host = seg_sums(r, "shyft_hip_catchment_sums", SERIES_FORCING + 0, 1, 5, len(order))
    dev = torch.full((len(order), 5), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    r.catchment_sums_device(SERIES_FORCING + 0, 1, 5, dev.data_ptr())
    assert np.array_equal(dev.cpu().numpy(), host)


# ---------------------------------------------------------------- routing group sums on run discharge

N_RUN, T_RUN = rc.N_CELLS + 37, 6


@pytest.fixture(scope="module")
def ran():
    """a short pt_gs_k run: (region, discharge [T_RUN][N_RUN])"""
    from shyft_amd.region import COLLECT_DISCHARGE
    r = new_region(N_RUN, T_RUN, synthetic.geo11(N_RUN, n_catchments=3), COLLECT_DISCHARGE)
    r.set_state(synthetic.default_ptgsk_state(N_RUN))
    r.synthetic_forcing(synthetic.SEED, 0, T_RUN)
    r.run_cells()
    q = r.get_series(0, 0, T_RUN)
    q.setflags(write=False)
    assert np.isfinite(q).all() and len(np.unique(q[-1])) > N_RUN // 10
    yield r, q
    r.close()


def expected_groups(q, group_of, n_groups):
    out = np.empty((n_groups, q.shape[0]))
    for g in range(n_groups):
        cells = np.flatnonzero(group_of == g)
        out[g] = rc.device_order_sum(q[:, cells]) if cells.size else 0.0
    return out


def _group_layouts():
    """{name: (group of each cell, n_groups)}; groups 0 and the last are empty where the name says so"""
    sizes = np.repeat(np.arange(1, len(rc.SIZES) + 1), rc.SIZES)        # groups 1..14 in the size classes
    dealt = np.full(N_RUN, -1)
    dealt[np.random.default_rng(21).permutation(N_RUN)[: rc.N_CELLS]] = sizes   # 37 cells routed nowhere
    blocks = np.full(N_RUN, -1)
    blocks[: rc.N_CELLS] = sizes
    ident = (np.arange(N_RUN) * 5) // N_RUN                               # every cell, in order: the identity
    one_out = ident.copy()
    one_out[N_RUN // 2] = -1
    swapped = ident.copy()
    b = int(np.flatnonzero(ident == 1)[0])                                # the first cell of group 1
    swapped[b - 1], swapped[b] = 1, 0
    return {"dealt, empty first and last": (dealt, len(rc.SIZES) + 2),
            "blocks, empty first and last": (blocks, len(rc.SIZES) + 2),
            "identity": (ident, 5), "identity but one cell unrouted": (one_out, 5),
            "identity but an adjacent pair swapped": (swapped, 5)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_group_layouts()))
def test_routing_group_sums_size_classes_and_near_identity(ran, name):
    r, q = ran
    group_of, n_groups = _group_layouts()[name]
    r.set_routing_groups(group_of, n_groups)
    got = group_sums(r, 0, T_RUN)
    want = expected_groups(q, group_of, n_groups)
    assert same_bits(got, want)
    if "empty" in name:
        assert np.all(got[[0, -1]] == 0.0) and not np.signbit(got[[0, -1]]).any()
    got = group_sums(r, 2, 3)
    assert same_bits(got, want[:, 2:5])
    if name.startswith("identity but"):     # reading cells 0..n-1 in order instead would give other bits
        ident, _ = _group_layouts()["identity"]
        assert not np.array_equal(want, expected_groups(q, ident, n_groups))


@pytest.mark.gpu
def test_routing_group_sums_into_device_memory(ran):
    import torch
    r, q = ran
    group_of, n_groups = _group_layouts()["dealt, empty first and last"]
    r.set_routing_groups(group_of, n_groups)
    host = group_sums(r, 1, 4)
    dev = torch.full((n_groups, 4), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    r.routing_group_sums_device(1, 4, dev.data_ptr())
    assert same_bits(dev.cpu().numpy(), host)


# ---------------------------------------------------------------- grid-stride tails: forcing_ok and the NaN fill

N_BIG, T_BIG = 4099, 120
STRIDE = 8192 * 256     # the elements one pass of the capped grid covers


def big_region():
    """5 * 120 * 4099 = 2,459,400 forcing values and 8 * 120 * 4099 response values: both above STRIDE"""
    from shyft_amd.region import COLLECT_ALL
    geo = synthetic.geo11(N_BIG, n_catchments=3)
    geo[:, 4] = np.random.default_rng(4).choice([5, 9, 2], N_BIG)
    geo[-1, 4] = 9      # the last cell is in catchment 9
    return new_region(N_BIG, T_BIG, geo, COLLECT_ALL), geo[:, 4].astype(int)


@pytest.mark.gpu
def test_fresh_region_is_nan_to_the_last_element():
    """launch_fill past its 8,192-block cap: the forcing (2,459,400 values) and the response buffer of COLLECT_ALL
    (3,935,040 values) are both longer than one pass of the grid"""
    from shyft_amd.region import PTGSK_SERIES
    assert 5 * T_BIG * N_BIG > STRIDE and len(PTGSK_SERIES) * T_BIG * N_BIG > STRIDE
    r, _ = big_region()
    try:
        assert np.isnan(r.get_forcing(4, T_BIG - 1, 1)).all()
        assert np.isnan(r.get_forcing(4, T_BIG - 20, 20)).all() and np.isnan(r.get_forcing(0, 0, 1)).all()
        last = len(PTGSK_SERIES) - 1
        assert np.isnan(r.get_series(last, T_BIG - 1, 1)).all()
        assert np.isnan(r.get_series(last, T_BIG - 20, 20)).all() and np.isnan(r.get_series(0, 0, 1)).all()
    finally:
        r.close()


@pytest.mark.gpu
def test_forcing_ok_sees_every_element_and_only_active_cells():
    r, cid = big_region()
    try:
        assert not forcing_ok(r)                       # fresh: NaN-filled
        F = rc.planted(5 * T_BIG, N_BIG, 8).reshape(5, T_BIG, N_BIG)
        for v in range(4):
            r.set_forcing(v, 0, F[v])
        assert not forcing_ok(r)                       # one variable still unset
        r.set_forcing(4, 0, F[4])
        assert forcing_ok(r)

        def poke(v, t, c, value):
            """ok with F[v][t][c] = value, the row restored afterwards"""
            row = F[v, t].copy()
            row[c] = value
            r.set_forcing(v, t, row)
            ok = forcing_ok(r)
            r.set_forcing(v, t, F[v, t])
            return ok

        flat = lambda v, t, c: (v * T_BIG + t) * N_BIG + c  # noqa: E731
        tail = (4, 50, 7)
        assert flat(*tail) >= STRIDE and flat(4, T_BIG - 1, N_BIG - 1) == 5 * T_BIG * N_BIG - 1
        assert not poke(0, 0, 0, np.nan)                       # flat index 0
        assert not poke(4, T_BIG - 1, N_BIG - 1, np.nan)       # the last element
        assert not poke(*tail, np.nan)                         # the grid-stride tail
        assert not poke(2, 60, 1000, np.nan)
        for where in ((0, 0, 0), (4, T_BIG - 1, N_BIG - 1), tail):
            assert poke(*where, np.inf) and poke(*where, -np.inf)
        assert forcing_ok(r)

        r.set_catchment_filter([5, 9])                         # catchment 2 is not calculated
        out_cells, in_cells = np.flatnonzero(cid == 2), np.flatnonzero(cid != 2)
        assert in_cells[-1] == N_BIG - 1
        assert forcing_ok(r)
        rows = [(0, 0), (4, 50), (4, T_BIG - 1)]               # first row, a row in the tail, the last row
        assert flat(4, 50, 0) >= STRIDE
        for v, t in rows:
            row = F[v, t].copy()
            row[out_cells] = np.nan
            r.set_forcing(v, t, row)
        assert forcing_ok(r)                                   # NaN only in cells that are filtered out
        for v, t in rows:
            for c in (in_cells[0], in_cells[len(in_cells) // 2], in_cells[-1]):
                row = F[v, t].copy()
                row[out_cells] = np.nan
                row[c] = np.nan
                r.set_forcing(v, t, row)
                assert not forcing_ok(r), (v, t, c)
                row[c] = F[v, t, c]
                r.set_forcing(v, t, row)
        assert forcing_ok(r)
        r.set_catchment_filter([])
        assert not forcing_ok(r)                               # without the filter the same NaNs count
    finally:
        r.close()


# ---------------------------------------------------------------- more segments than one launch's grid.y takes

@pytest.mark.gpu
def test_seventy_thousand_routing_groups():
    """70,000 groups of one cell each (a few empty): the segments go in the launch's grid.y, and the MI355X reports
    maxGridSize[1] = 65,536. launch_segment_sums launches them in slices of 65,535, each with its own seg_off and out
    rows: every segment, those next to the slice boundary and above it included, gets its sum."""
    from shyft_amd.region import COLLECT_DISCHARGE
    n, T = 70_000, 2
    r = new_region(n, T, synthetic.geo11(n, n_catchments=3), COLLECT_DISCHARGE)
    try:
        r.set_state(synthetic.default_ptgsk_state(n))
        r.synthetic_forcing(synthetic.SEED, 0, T)
        r.run_cells()
        q = r.get_series(0, 0, T)
        group_of = np.arange(n)
        empty = [0, 4097, 65_534, 65_535, 65_536, n - 1]
        group_of[empty] = -1
        r.set_routing_groups(group_of, n)
        got = group_sums(r, 0, T)
        want = (0.0 + q.T).copy()
        want[empty] = 0.0
        assert same_bits(got, want)
        assert np.count_nonzero(want) > n        # the run produced discharge
    finally:
        r.close()
