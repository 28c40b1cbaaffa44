"""River routing for parameter ensembles on the host (shyft_hip_route_members_host through
region.route_members(host=True), and the factored routing-group construction of csrc/host/routing.hpp).

The host twin is the literal loops in the reference's order and is what the device entry is compared with bit for
bit (test_ensemble_routing_gpu.py). Here it is checked against the oracle's per-cell convolution (1e-12 relative and
absolute, test_routing.py's tolerance for the same reason: the same terms in another order), against itself member by
member, at its edges, and the refusals of both entries are compared: each is made before the device is touched, so
the device entry refuses with the same text on a machine without a device."""
import numpy as np
import pytest

from shyft_amd import region, synthetic
from shyft_amd._native import ShyftHipError
from tests import oracle_lib
from tests import route_members_cases as rc
from tests.test_routing import RIVERS

HOUR = synthetic.HOUR_US
MEMBERS = [(1.0, 7.0, 0.0), (5.0, 3.0, 0.0), (0.3, 5.0, 0.001)]  # routing velocity, alpha, beta


def _groups(cell_rid, cell_dist, vab, rivers=None):
    from shyft_amd.api import _api as A
    group_of, rid, w = A.routing_groups(list(cell_rid), list(cell_dist), rc.HOUR_S, *vab, rivers=rivers)
    return np.asarray(group_of, np.int32), list(rid), [np.asarray(x) for x in w]


def test_host_twin_matches_the_oracles_per_cell_convolution():
    n, T = 40, 60
    rng = np.random.default_rng(17)
    q = rng.uniform(0.0, 4.0, (T, n))
    cell_rid = 1 + np.arange(n) % 4
    cell_rid[[3, 22]] = 0  # not routed
    cell_dist = rng.choice(rc.DISTANCES, n)
    row, sums, uhgs, river = [0], [], [], []
    for vab in MEMBERS:
        group_of, rid, w = _groups(cell_rid, cell_dist, vab)
        assert np.all((group_of >= 0) == (cell_rid > 0))
        for g in range(len(rid)):
            sums.append(q[:, group_of == g].sum(axis=1))
        uhgs += w
        river += [r - 1 for r in rid]
        row.append(len(uhgs))
    counts = np.diff(row)
    assert len(set(counts)) == 3, counts  # the members partition the cells differently
    local, up, out = region.route_members(row, np.array(sums), uhgs, river, rc.river_uhgs(), rc.RIVER_DOWN, host=True)
    assert out.shape == (3, 4, T)
    for m, vab in enumerate(MEMBERS):
        for k, (rid, *_rest) in enumerate(RIVERS):
            ol, ou, oo = oracle_lib.route(q, HOUR, cell_rid, cell_dist, np.tile(vab, (n, 1)), RIVERS, rid)
            assert np.allclose(local[m, k], ol, rtol=1e-12, atol=1e-12), (m, rid)
            assert np.allclose(up[m, k], ou, rtol=1e-12, atol=1e-12), (m, rid)
            assert np.allclose(out[m, k], oo, rtol=1e-12, atol=1e-12), (m, rid)
    assert out[:, 0].sum() > 0 and up[:, 0].sum() > 0
    assert not np.array_equal(out[0], out[1])


def test_host_twin_all_members_equal_member_by_member():
    counts = (5, 0, 9, 1)
    case = rc.random_case(counts, 70, [1, 2, 9, 80], seed=3)
    local, up, out = region.route_members(*case, host=True)
    for m in range(4):
        l1, u1, o1 = region.route_members(*rc.member_slice(case, m), host=True)
        assert np.array_equal(local[m], l1[0]) and np.array_equal(up[m], u1[0]) and np.array_equal(out[m], o1[0])
    assert np.all(out[1] == 0.0) and np.all(local[1] == 0.0)  # the member without groups
    assert np.any(out[0] != 0.0) and np.any(out[3] != 0.0)


def test_a_river_without_groups_or_upstream_rivers_is_zero_and_one_step_works():
    row, sums, uhgs, river, ruhgs, down = rc.random_case((4, 3), 1, [1, 3], seed=5)
    river[:] = np.where(river == 3, 0, river)  # river 3 (index) is a source: nothing routes to it
    local, up, out = region.route_members(row, sums, uhgs, river, ruhgs, down, host=True)
    assert out.shape == (2, 4, 1)
    assert np.all(local[:, 3] == 0.0) and np.all(up[:, 3] == 0.0) and np.all(out[:, 3] == 0.0)
    for m in range(2):
        for r in range(4):  # T = 1: only tap 0 of every UHG takes part
            mine = [g for g in range(int(row[m]), int(row[m + 1])) if river[g] == r]
            acc = 0.0
            for g in mine:
                acc += uhgs[g][0] * sums[g, 0]
            assert local[m, r, 0] == acc
    assert np.array_equal(up[:, 0], out[:, 1] + out[:, 2])  # rivers 2 and 3 (ids) flow into river 1


# ---- refusals: the device entry, before it touches the device, and its _host twin say the same -------------------------
def _refused(expected, max_len=None, **change):
    texts = []
    for host in (False, True):
        row, sums, uhgs, river, ruhgs, down = rc.random_case((2, 3), 8, [1, 3], seed=7)
        a = dict(group_row=row, group_sums=sums, group_uhgs=uhgs, group_river=river, river_uhgs=ruhgs,
                 river_downstream=list(down))
        a.update(change)
        with pytest.raises(ShyftHipError) as e:
            region.route_members(host=host, max_len=max_len, **a)
        texts.append(str(e.value))
    assert texts == [expected, expected]


def test_the_well_formed_case_is_accepted_by_the_host_twin():
    out = region.route_members(*rc.random_case((2, 3), 8, [1, 3], seed=7), host=True)[2]
    assert out.shape == (2, 4, 8) and np.all(np.isfinite(out))


def test_a_group_row_that_does_not_start_at_zero_is_refused():
    _refused("route_members: group_row must start at 0", group_row=[1, 2, 5])


def test_a_decreasing_group_row_is_refused():
    _refused("route_members: group_row must not decrease", group_row=[0, 6, 5])


def test_a_group_river_out_of_range_is_refused():
    _refused("route_members: group river out of range", group_river=[0, 1, 4, 0, 0])
    _refused("route_members: group river out of range", group_river=[0, 1, -1, 0, 0])


def test_a_uhg_length_of_zero_or_above_max_len_is_refused():
    uhgs = rc.random_case((2, 3), 8, [1, 3], seed=7)[2]
    _refused("route_members: group UHG length", group_uhgs=uhgs[:2] + [np.zeros(0)] + uhgs[3:])
    _refused("route_members: group UHG length", max_len=2)  # groups of 3 taps, rivers of up to 5
    _refused("route_members: river UHG length", river_uhgs=[np.ones(1), np.zeros(0), np.ones(1), np.ones(2)])
    _refused("route_members: river UHG length", group_uhgs=[np.ones(1)] * 5, max_len=4)


def test_a_river_that_is_its_own_downstream_is_refused():
    _refused("route_members: invalid downstream river", river_downstream=[-1, 1, 0, 1])
    _refused("route_members: invalid downstream river", river_downstream=[-1, 0, 0, 4])


def test_a_cycle_in_the_network_is_refused():
    _refused("route_members: the river network has a cycle", river_downstream=[-1, 2, 1, 0])


# ---- the factored group construction ------------------------------------------------------------------------------
def _distance_cells():
    n = 40
    cell_rid = 1 + (np.arange(n) // 2) % 4
    cell_dist = np.array([rc.DISTANCES[(i * 7 + i // 5) % 4] for i in range(n)])
    assert all(set(cell_dist[cell_rid == r]) == set(rc.DISTANCES) for r in range(1, 5))
    return cell_rid, cell_dist


@pytest.mark.parametrize("velocity, classes", [(5.0, [[0.0, 1500.0, 5000.0], [12000.0]]),
                                               (1.0, [[0.0, 1500.0], [5000.0], [12000.0]]),
                                               (0.3, [[0.0], [1500.0], [5000.0], [12000.0]])])
def test_cells_share_a_group_by_their_whole_uhg_steps(velocity, classes):
    cell_rid, cell_dist = _distance_cells()
    group_of, rid, w = _groups(cell_rid, cell_dist, (velocity, 7.0, 0.0))
    assert len(rid) == 4 * len(classes)
    for r in range(1, 5):
        for cls in classes:
            sel = (cell_rid == r) & np.isin(cell_dist, cls)
            g = set(group_of[sel])
            assert len(g) == 1  # one group per (river, class)
            g = g.pop()
            assert rid[g] == r
            assert np.array_equal(np.flatnonzero(group_of == g), np.flatnonzero(sel))  # and nothing else in it
            steps = int(cls[0] / velocity / rc.HOUR_S + 0.5)
            assert len(w[g]) == max(1, steps)
    # numbered by first appearance in cell order
    first = [int(np.flatnonzero(group_of == g)[0]) for g in range(len(rid))]
    assert first == sorted(first)


def test_a_river_subset_keeps_each_rivers_relative_group_order():
    cell_rid, cell_dist = _distance_cells()
    vab = (0.3, 7.0, 0.0)
    all_of, all_rid, all_w = _groups(cell_rid, cell_dist, vab)
    sub_of, sub_rid, sub_w = _groups(cell_rid, cell_dist, vab, rivers=[2, 4])
    assert set(sub_rid) == {2, 4} and len(sub_rid) == 8
    assert np.all(sub_of[~np.isin(cell_rid, [2, 4])] == -1)
    for r in (2, 4):
        mine_all = [g for g in range(len(all_rid)) if all_rid[g] == r]
        mine_sub = [g for g in range(len(sub_rid)) if sub_rid[g] == r]
        assert len(mine_all) == len(mine_sub) == 4
        for ga, gs in zip(mine_all, mine_sub):  # the k-th group of the river is the same cells with the same UHG
            assert np.array_equal(np.flatnonzero(all_of == ga), np.flatnonzero(sub_of == gs))
            assert np.array_equal(all_w[ga], sub_w[gs])
