"""Calibration against routed discharge in device ensembles: the optimizer batches ROUTED_DISCHARGE targets like
every other target (one ensemble run and one ensemble routing per slice of vectors), and a batched member's goal
value is bit-identical to the sequential evaluation of the same vector, although routing.velocity and
routing.alpha are part of the vector and so every member has its own routing groups and unit hydrographs.

The scenario is test_calibration._opt_scenario plus a two-river network (river 2 flows into river 1) and nonzero
cell routing distances."""
import numpy as np
import pytest

from tests import route_members_cases as rc
from tests.test_calibration import _opt_scenario

pytestmark = pytest.mark.gpu


def _routed_scenario():
    api, pt_gs_k, model, opt_model, tsa, cids = _opt_scenario()
    opt_model.river_network.add(api.River(1, api.RoutingInfo(0, 8000.0), api.UHGParameter(1.0, 3.0, 0.0)))
    opt_model.river_network.add(api.River(2, api.RoutingInfo(1, 20000.0), api.UHGParameter(1.5, 7.0, 0.0)))
    for i in range(opt_model.size()):
        opt_model._set_cell_routing(i, 1 + i % 2, rc.DISTANCES[(i // 2 + i // 7) % 4])
    return api, pt_gs_k, model, opt_model, tsa, cids


def _bounds(pt_gs_k, model):
    lo = pt_gs_k.PTGSKParameter(model.get_region_parameter())
    hi = pt_gs_k.PTGSKParameter(model.get_region_parameter())
    lo.kirchner.c1, hi.kirchner.c1 = -3.0, -1.9
    lo.kirchner.c2, hi.kirchner.c2 = 0.8, 0.99
    lo.routing.velocity, hi.routing.velocity = 0.3, 5.0
    lo.routing.alpha, hi.routing.alpha = 2.0, 8.0
    return lo, hi


def test_batched_routed_goal_functions_are_bit_identical_to_sequential():
    api, pt_gs_k, model, opt_model, tsa, cids = _routed_scenario()
    targets = api.TargetSpecificationVector()
    targets.append(api.TargetSpecificationPts(tsa, 1, 1.0, api.NASH_SUTCLIFFE, 1.0, 1.0, 1.0, "routed_ns"))
    targets.append(api.TargetSpecificationPts(tsa, 2, 0.5, api.KLING_GUPTA, 1.0, 2.0, 0.5, "routed_kg_upstream"))
    targets.append(api.TargetSpecificationPts(tsa, cids, 0.25, api.NASH_SUTCLIFFE, 1.0, 1.0, 1.0, api.DISCHARGE))
    lo, hi = _bounds(pt_gs_k, model)
    o = pt_gs_k.PTGSKOptimizer(opt_model)
    o.set_target_specification(targets, lo, hi)
    assert o.n_batched_evaluations == 0 and o.n_sequential_evaluations == 0
    rng = np.random.default_rng(5)
    ps = []
    for _ in range(9):
        p = pt_gs_k.PTGSKParameter(model.get_region_parameter())
        p.kirchner.c1 = rng.uniform(-3.0, -1.9)
        p.kirchner.c2 = rng.uniform(0.8, 0.99)
        p.routing.velocity = rng.uniform(0.3, 5.0)
        p.routing.alpha = rng.uniform(2.0, 8.0)
        ps.append(p)
    batched = o.calculate_goal_functions(ps)
    assert o.n_batched_evaluations == 9 and o.n_sequential_evaluations == 0
    assert o.trace_size == 9
    sequential = [o.calculate_goal_function(p) for p in ps]
    assert o.n_batched_evaluations == 9 and o.n_sequential_evaluations == 9
    assert batched == sequential  # bit-identical
    assert all(np.isfinite(batched))
    assert len(set(batched)) == 9  # the vectors differ, and so do their goals
    # a vector that differs in the routing velocity alone changes the goal: routing is part of what is scored
    q = pt_gs_k.PTGSKParameter(ps[0])
    q.routing.velocity = 0.31 if ps[0].routing.velocity > 1.0 else 4.9
    two = o.calculate_goal_functions([ps[0], q])
    assert two[0] == batched[0] and two[1] != two[0]


def test_sceua_with_a_routed_target_batched_equals_sequential():
    api, pt_gs_k, model, opt_model, tsa, cids = _routed_scenario()
    targets = api.TargetSpecificationVector()
    targets.append(api.TargetSpecificationPts(tsa, 1, 1.0, api.NASH_SUTCLIFFE, 1.0, 1.0, 1.0, "routed_ns"))
    lo, hi = _bounds(pt_gs_k, model)
    p0 = pt_gs_k.PTGSKParameter(model.get_region_parameter())
    p0.kirchner.c1, p0.kirchner.c2 = -2.2, 0.85
    p0.routing.velocity, p0.routing.alpha = 2.0, 4.0
    runs = []
    for batch in (True, False):
        o = pt_gs_k.PTGSKOptimizer(opt_model)
        o.batch_evaluation = batch
        o.set_target_specification(targets, lo, hi)
        p = o.optimize_sceua(p0, 120, 1e-4, 1e-6)
        runs.append((p.to_vector(), o.trace_goal_function_values))
        if batch:
            assert o.n_batched_evaluations > 0
        else:
            assert o.n_batched_evaluations == 0 and o.n_sequential_evaluations == len(runs[-1][1])
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1]
    assert len(runs[0][1]) > 9
