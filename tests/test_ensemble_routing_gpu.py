"""Ensemble routing on the device: per-member routing-group sums of an ensemble run
(shyft_hip_ensemble_group_sums), the river network for all members at once (shyft_hip_route_members,
kernels/routing_members.hip), and the host class and Python layers on top (region_model::ensemble_routed,
model.ensemble_river_output_flow_m3s).

Every comparison is bit for bit (np.array_equal): a member's group sums against shyft_hip_routing_group_sums after
a sequential run with the member's parameters, the device routing against its _host twin and against
shyft_hip_route called member by member, and the api method against set_region_parameter + run_cells +
river_output_flow_m3s."""
import numpy as np
import pytest

from shyft_amd import region, synthetic
from shyft_amd.region import COLLECT_DISCHARGE, PT_GS_K, HipRegion
from tests import route_members_cases as rc

pytestmark = pytest.mark.gpu

HOUR = synthetic.HOUR_US
VELOCITIES = (1.0, 5.0, 0.3)


# ---- group sums --------------------------------------------------------------------------------------------------------
N_CELLS, N_STEPS, N_CATCH = 2000, 30, 10


def _cells():
    """Catchments 1..8 (80 % of the cells) route to river 1, catchment 9 to rivers 2 and 3, catchment 10 to river
    4; river 3 has exactly one cell 12 km away, which is a group of its own at every velocity."""
    geo = synthetic.geo11(N_CELLS, n_catchments=N_CATCH)
    cid = geo[:, 4].astype(np.int64)
    i = np.arange(N_CELLS)
    rid = np.where(cid <= 8, 1, np.where(cid == 9, 2 + i % 2, 4))
    rng = np.random.default_rng(23)
    dist = rng.choice(rc.DISTANCES, N_CELLS)
    r3 = np.flatnonzero(rid == 3)
    dist[r3] = rng.choice(rc.DISTANCES[:3], r3.size)
    dist[r3[7]] = 12000.0
    rid[5] = 0  # one cell that is not routed
    return geo, cid, rid, dist


def _member_groups(rid, dist, members, rivers=None):
    from shyft_amd.api import _api as A
    group_of, row = [], [0]
    for p in members:
        g, grid, _ = A.routing_groups(list(rid), list(dist), rc.HOUR_S, p[25], p[26], p[27], rivers=rivers)
        group_of.append(np.asarray(g, np.int32))
        row.append(row[-1] + len(grid))
    return np.stack(group_of), np.asarray(row, np.int64)


def _members():
    base = synthetic.default_ptgsk_parameters()
    p = np.tile(base, (len(VELOCITIES), 1))
    p[:, 25] = VELOCITIES
    p[:, 0] = (-2.439, -2.2, -2.7)  # kirchner c1
    return p


def _group_sum_region(filt=None):
    geo, cid, rid, dist = _cells()
    r = HipRegion(PT_GS_K, N_CELLS)
    r.set_geo(geo)
    r.set_parameters(synthetic.default_ptgsk_parameters()[None, :])
    r.set_time_axis(synthetic.T0_2015_US, HOUR, N_STEPS)
    r.set_collection(COLLECT_DISCHARGE)
    r.set_state(synthetic.default_ptgsk_state(N_CELLS))
    r.synthetic_forcing(synthetic.SEED, 0, N_STEPS)
    if filt is not None:
        r.set_catchment_filter(filt)
    return r, cid, rid, dist


def _check_group_sums(filt, rivers):
    r, cid, rid, dist = _group_sum_region(filt)
    try:
        members = _members()
        group_of, row = _member_groups(rid, dist, members, rivers)
        if filt is not None:
            assert np.all(group_of[:, ~np.isin(cid, filt)] == -1)  # the left-out catchment routes outside `rivers`
        sizes = [np.bincount(g[g >= 0]) for g in group_of]
        assert max(sizes[1]) > 1024  # the four-loads-ahead loop of the segment sum
        assert all(1 in s for s in sizes)  # and a group of a single cell
        assert len({len(s) for s in sizes}) == 3  # the members partition the cells differently
        s0 = r.get_state().copy()
        r.ensemble_run(members)
        got = r.ensemble_group_sums(group_of, row, 0, N_STEPS)
        assert got.shape == (row[-1], N_STEPS)
        assert np.array_equal(r.get_state(), s0)
        for m in range(len(members)):
            r.set_parameters(members[m:m + 1])
            r.set_state(s0)
            r.run_cells()
            r.set_routing_groups(group_of[m], int(row[m + 1] - row[m]))
            ref = r.routing_group_sums(0, N_STEPS)
            assert np.array_equal(got[row[m]:row[m + 1]], ref), f"member {m}"
            assert np.all(np.isfinite(ref)) and ref.sum() > 0
        assert not np.array_equal(got[row[0]], got[row[2]])
        # a window of the run's steps
        part = r.ensemble_group_sums(group_of, row, 7, 11)
        assert np.array_equal(part, got[:, 7:18])
    finally:
        r.close()


def test_member_group_sums_equal_the_sequential_runs():
    _check_group_sums(None, None)


def test_member_group_sums_with_a_catchment_left_out():
    _check_group_sums(list(range(1, 10)), [1, 2, 3])


def test_group_sum_refusals():
    r, cid, rid, dist = _group_sum_region(list(range(1, 10)))
    try:
        members = _members()
        group_of, row = _member_groups(rid, dist, members, [1, 2, 3])
        with pytest.raises(RuntimeError, match="ensemble_group_sums: no ensemble run"):
            r.ensemble_group_sums(group_of, row, 0, N_STEPS)
        r.ensemble_run(members)
        with pytest.raises(RuntimeError, match="n_members differs from the last ensemble run's 3"):
            r.ensemble_group_sums(group_of[:2], row[:3], 0, N_STEPS)
        bad = group_of.copy()
        bad[1, 100] = row[2] - row[1]  # one past member 1's last group
        with pytest.raises(RuntimeError, match="ensemble_group_sums: group index out of range"):
            r.ensemble_group_sums(bad, row, 0, N_STEPS)
        bad = group_of.copy()
        bad[2, 7] = -2
        with pytest.raises(RuntimeError, match="ensemble_group_sums: group index out of range"):
            r.ensemble_group_sums(bad, row, 0, N_STEPS)
        bad = group_of.copy()
        cell = int(np.flatnonzero(cid == 10)[3])  # catchment 10 is filtered out
        bad[0, cell] = 0
        with pytest.raises(RuntimeError, match=f"cell {cell} has a group but was not a calculated cell"):
            r.ensemble_group_sums(bad, row, 0, N_STEPS)
        with pytest.raises(RuntimeError, match="steps outside the last ensemble run"):
            r.ensemble_group_sums(group_of, row, 20, N_STEPS)
        with pytest.raises(RuntimeError, match="group_row must not decrease"):
            r.ensemble_group_sums(group_of, [0, 5, 3, 9], 0, N_STEPS)
        assert r.ensemble_group_sums(group_of, row, 0, N_STEPS).shape == (row[-1], N_STEPS)  # still usable
    finally:
        r.close()


def test_group_sums_of_a_sharded_region_are_refused_as_out_of_scope():
    n = 64
    r = HipRegion(PT_GS_K, n, devices=[0, 0])
    try:
        r.set_geo(synthetic.geo11(n, n_catchments=4))
        with pytest.raises(RuntimeError, match="sharded regions are out of scope"):
            r.ensemble_group_sums(np.zeros((2, n), np.int32), [0, 1, 2], 0, 1)
    finally:
        r.close()


# ---- routing -----------------------------------------------------------------------------------------------------------
def _check_routing(case):
    row = case[0]
    dev = region.route_members(*case)
    host = region.route_members(*case, host=True)
    for name, d, h in zip(("local", "upstream", "output"), dev, host):
        assert d.shape == h.shape
        assert np.array_equal(d, h), name
    for m in range(len(row) - 1):
        if row[m + 1] == row[m]:
            assert all(np.all(d[m] == 0.0) for d in dev)  # a member without groups
            continue
        _, sums, uhgs, river, ruhgs, down = rc.member_slice(case, m)
        one = region.route(sums, uhgs, river, ruhgs, down)
        for name, d, o in zip(("local", "upstream", "output"), dev, one):
            assert np.array_equal(d[m], o), (name, m)
    assert np.all(np.isfinite(dev[2])) and np.any(dev[2] != 0.0)
    assert region.route_members_last_ms() > 0.0


def test_device_routing_equals_the_host_twin_and_route_member_by_member():
    # T = 300 is not a multiple of the 256-step tile; 256 / 257 sit on the staged chunk's edge and 333 is longer than
    # both T and one chunk, so the j <= t edge and the chunk boundary meet in one convolution
    _check_routing(rc.random_case((5, 0, 9, 1), 300, [1, 2, 256, 257, 333], seed=41, river_lengths=[3, 257, 1, 333]))


def test_device_routing_of_one_step():
    _check_routing(rc.random_case((5, 0, 9, 1), 1, [1, 2, 256, 257, 333], seed=43))


# ---- host class and Python ---------------------------------------------------------------------------------------------
def _routed_model(n=40, T=72):
    from shyft_amd import api
    from shyft_amd.api import pt_gs_k
    from tests.test_api_region_model import build_model, dummy_env
    from tests.test_routing import RIVERS
    model = build_model(pt_gs_k.PTGSKModel, pt_gs_k.PTGSKParameter, n, num_catchments=4)
    ta = api.TimeAxisFixedDeltaT(api.Calendar().time(2015, 1, 1, 0, 0, 0), api.deltahours(1), T)
    model.initialize_cell_environment(ta)
    model.interpolate(api.InterpolationParameter(), dummy_env(ta, model.get_cells()[n // 2].geo.mid_point()))
    s0 = pt_gs_k.PTGSKStateVector()
    for i in range(n):
        si = pt_gs_k.PTGSKState()
        si.kirchner.q = 20.0 + i
        s0.append(si)
    model.set_states(s0)
    for rid, ds, d, v, a, b in RIVERS:
        model.river_network.add(api.River(rid, api.RoutingInfo(ds, d), api.UHGParameter(v, a, b)))
    for i in range(n):
        model._set_cell_routing(i, 1 + i % 4, rc.DISTANCES[(i * 7 + i // 5) % 4])  # catchment c routes to river c
    ps = []
    for c1, v, a in [(-2.439, 1.0, 7.0), (-2.2, 5.0, 3.0), (-2.7, 0.3, 5.0), (-2.5, 0.7, 7.0), (-2.3, 2.0, 2.5)]:
        p = pt_gs_k.PTGSKParameter(model.get_region_parameter())
        p.kirchner.c1, p.routing.velocity, p.routing.alpha = c1, v, a
        ps.append(p)
    return api, pt_gs_k, model, s0, ps


def test_api_ensemble_river_output_flow_equals_the_sequential_evaluations():
    api, pt_gs_k, model, s0, ps = _routed_model()
    rids = [4, 1, 3, 2]
    state_before = [list(s) for s in model._get_states()]
    param_before = list(model.get_region_parameter().to_vector())
    got = model.ensemble_river_output_flow_m3s(ps, rids)
    sub = model.ensemble_river_output_flow_m3s(ps, [2])  # evaluates rivers 2 and 4 only
    assert [list(s) for s in model._get_states()] == state_before
    assert list(model.get_region_parameter().to_vector()) == param_before
    assert list(model._get_region_parameter()) == param_before
    assert len(got) == len(ps) and all(len(g) == len(rids) for g in got)
    outs = []
    for m, p in enumerate(ps):
        model.set_region_parameter(p)
        model.set_states(s0)
        model.run_cells()
        for q, rid in enumerate(rids):
            ref = model.river_output_flow_m3s(rid).values.to_numpy()
            assert np.array_equal(got[m][q].values.to_numpy(), ref), (m, rid)
            assert np.all(np.isfinite(ref)) and ref.sum() > 0
        assert np.array_equal(sub[m][0].values.to_numpy(), got[m][3].values.to_numpy())
        outs.append(got[m][1].values.to_numpy())
    assert all(not np.array_equal(outs[0], o) for o in outs[1:])


def test_api_ensemble_routing_refuses_a_local_parameter_on_a_feeding_catchment():
    api, pt_gs_k, model, s0, ps = _routed_model()
    local = pt_gs_k.PTGSKParameter(model.get_region_parameter())
    local.kirchner.c1 = -2.0
    model.set_catchment_parameter(4, local)  # catchment 4 -> river 4 -> river 2 -> river 1
    with pytest.raises(RuntimeError, match="catchment 4 feeding river 4 has a catchment-specific parameter"):
        model.ensemble_river_output_flow_m3s(ps, [1])
    assert len(model.ensemble_river_output_flow_m3s(ps, [3])) == len(ps)  # river 3 has nothing upstream of it


def test_api_ensemble_routing_refuses_an_uncalculated_feeding_cell_and_gives_zeros_without_routing():
    api, pt_gs_k, model, s0, ps = _routed_model()
    model.set_catchment_calculation_filter(api.IntVector([1, 2, 3]))
    with pytest.raises(RuntimeError, match="routes to river 4 but is not calculated"):
        model.ensemble_river_output_flow_m3s(ps, [2])
    assert len(model.ensemble_river_output_flow_m3s(ps, [3])) == len(ps)
    model.set_catchment_calculation_filter(api.IntVector())
    for i in range(model.size()):
        model._set_cell_routing(i, 0, 0.0)
    zeros = model.ensemble_river_output_flow_m3s(ps[:2], [1, 2])
    assert all(np.all(ts.values.to_numpy() == 0.0) for member in zeros for ts in member)
