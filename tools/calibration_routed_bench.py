#!/usr/bin/env python3
"""Routed-target calibration measurement (not part of bench.py): prints one JSON line per timed call and a summary.

calculate_goal_functions of --vectors (64) pt_gs_k parameter vectors that vary kirchner c1/c2, routing.velocity and
routing.alpha, one ROUTED_DISCHARGE target on river 1 of the four-river network, a region of --cells (100,000) cells in
16 catchments over --steps (8,760) hourly steps, with batch_evaluation on (device ensembles of --batch members: one
ensemble run, one ensemble routing per slice) and off (one run_cells and one river evaluation per vector, the path the
batched one must equal), alternating, --repeats times each after one warm-up of each. Wall time around the call (it
ends in device synchronises), and beside it the HIP-event milliseconds of the last ensemble launch and of the last
ensemble routing. The goal values of the two paths must be equal. --plain then times the batched call against a plain
DISCHARGE target of every catchment, the batched path without routing. There is no pass mark.

  python tools/calibration_routed_bench.py
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RIVERS = [(1, 0, 8000.0, 1.0, 3.0, 0.0), (2, 1, 20000.0, 1.5, 7.0, 0.0), (3, 1, 3000.0, 0.5, 5.0, 0.001),
          (4, 2, 6000.0, 2.0, 2.0, 0.0)]
DISTANCES = (0.0, 1500.0, 5000.0, 12000.0)
N_CATCHMENTS = 16


def constant_source(api, src_t, gp, period, value):
    ts = api.TsFactory().create_time_point_ts(period, api.UtcTimeVector([period.start]), api.DoubleVector([value]),
                                              api.POINT_AVERAGE_VALUE)
    return src_t(gp, ts)


def build(api, pt_gs_k, n, steps):
    gcds = api.GeoCellDataVector()
    for i in range(n):
        gp = api.GeoPoint(500 + 100.0 * (i % 300), 500.0 + 100.0 * (i // 300), 500.0 * i / n)  # within the IDW reach
        g = api.GeoCellData(gp, 1000 * 1000, 1 + (i * N_CATCHMENTS) // n, 0.9, api.LandTypeFractions(0.01, 0.05, 0.19, 0.3, 0.45))
        gcds.append(g)
    model = pt_gs_k.PTGSKOptModel(gcds, pt_gs_k.PTGSKParameter())
    ta = api.TimeAxisFixedDeltaT(api.Calendar().time(2015, 1, 1, 0, 0, 0), api.deltahours(1), steps)
    model.initialize_cell_environment(ta)
    period = api.UtcPeriod(*ta.total_period())
    gp = model.get_cells()[n // 2].geo.mid_point()
    env = api.ARegionEnvironment()
    env.precipitation.append(constant_source(api, api.PrecipitationSource, gp, period, 5.0))
    env.temperature.append(constant_source(api, api.TemperatureSource, gp, period, 10.0))
    env.wind_speed.append(constant_source(api, api.WindSpeedSource, gp, period, 2.0))
    env.rel_hum.append(constant_source(api, api.RelHumSource, gp, period, 0.7))
    env.radiation = api.RadiationSourceVector()
    env.radiation.append(constant_source(api, api.RadiationSource, gp, period, 300.0))
    model.interpolate(api.InterpolationParameter(), env)
    s0 = pt_gs_k.PTGSKStateVector()
    for i in range(n):
        si = pt_gs_k.PTGSKState()
        si.kirchner.q = 0.5 + (i % 7) * 0.1
        s0.append(si)
    model.set_states(s0)
    model.initial_state = s0
    for rid, ds, d, v, a, b in RIVERS:
        model.river_network.add(api.River(rid, api.RoutingInfo(ds, d), api.UHGParameter(v, a, b)))
    for i in range(n):
        cid = 1 + (i * N_CATCHMENTS) // n
        model._set_cell_routing(i, 1 + (cid - 1) % 4, DISTANCES[(i * 7 + i // 5) % 4])
    return model, ta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=8760)
    ap.add_argument("--vectors", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8, help="members per ensemble launch (device memory: members x cells x steps)")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--plain", action="store_true", help="then time the batched call against a plain DISCHARGE target")
    a = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("calibration_routed_bench: needs a GPU")
    from shyft_amd import api, region
    from shyft_amd.api import pt_gs_k

    t_build = time.perf_counter()
    model, ta = build(api, pt_gs_k, a.cells, a.steps)
    model.run_cells()
    observed = model.river_output_flow_m3s(1)
    model.revert_to_initial_state()
    targets = api.TargetSpecificationVector()
    targets.append(api.TargetSpecificationPts(observed, 1, 1.0, api.NASH_SUTCLIFFE, 1.0, 1.0, 1.0, "routed"))
    lo = pt_gs_k.PTGSKParameter(model.get_region_parameter())
    hi = pt_gs_k.PTGSKParameter(model.get_region_parameter())
    lo.kirchner.c1, hi.kirchner.c1 = -3.0, -1.9
    lo.kirchner.c2, hi.kirchner.c2 = 0.8, 0.99
    lo.routing.velocity, hi.routing.velocity = 0.3, 5.0
    lo.routing.alpha, hi.routing.alpha = 2.0, 8.0
    rng = np.random.default_rng(5)
    ps = []
    for _ in range(a.vectors):
        p = pt_gs_k.PTGSKParameter(model.get_region_parameter())
        p.kirchner.c1, p.kirchner.c2 = rng.uniform(-3.0, -1.9), rng.uniform(0.8, 0.99)
        p.routing.velocity, p.routing.alpha = rng.uniform(0.3, 5.0), rng.uniform(2.0, 8.0)
        ps.append(p)
    o = pt_gs_k.PTGSKOptimizer(model)
    o._o.max_batch_members = a.batch
    o.set_target_specification(targets, lo, hi)
    print(json.dumps({"what": "setup", "cells": a.cells, "steps": a.steps, "vectors": a.vectors, "batch": a.batch,
                      "seconds": round(time.perf_counter() - t_build, 3)}), flush=True)

    def timed(batch, vectors):
        o.batch_evaluation = batch
        t0 = time.perf_counter()
        g = o.calculate_goal_functions(vectors)
        dt = time.perf_counter() - t0
        rec = {"what": "batched" if batch else "sequential", "vectors": len(vectors), "seconds": round(dt, 4)}
        if batch:
            rec["ensemble_last_ms"] = round(model._ensemble_last_ms(), 3)
            rec["route_members_last_ms"] = round(region.route_members_last_ms(), 3)
        print(json.dumps(rec), flush=True)
        return g, dt

    timed(True, ps[:a.batch])  # warm-up of every shape of the timed calls: one full slice, and one sequential vector
    timed(False, ps[:2])
    on, off, goals = [], [], []
    for _ in range(a.repeats):
        g1, t1 = timed(True, ps)
        g0, t0 = timed(False, ps)
        on.append(t1)
        off.append(t0)
        goals.append(g1 == g0)
    print(json.dumps({"what": "summary", "cells": a.cells, "steps": a.steps, "vectors": a.vectors, "batch": a.batch,
                      "batched_seconds_best": round(min(on), 4), "sequential_seconds_best": round(min(off), 4),
                      "sequential_over_batched": round(min(off) / min(on), 3),
                      "batched_seconds_all": [round(x, 4) for x in on],
                      "sequential_seconds_all": [round(x, 4) for x in off],
                      "goals_bit_identical": all(goals), "n_batched_evaluations": o.n_batched_evaluations,
                      "n_sequential_evaluations": o.n_sequential_evaluations}), flush=True)
    if a.plain:
        # the same vectors against a plain DISCHARGE target of every catchment: the batched path without any routing,
        # so the difference to the routed call above is what the group sums and the routing cost
        plain = api.TargetSpecificationVector()
        plain.append(api.TargetSpecificationPts(observed, api.IntVector(list(range(1, N_CATCHMENTS + 1))), 1.0,
                                                api.NASH_SUTCLIFFE, 1.0, 1.0, 1.0, api.DISCHARGE, "plain"))
        o.set_target_specification(plain, lo, hi)
        o.batch_evaluation = True
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            o.calculate_goal_functions(ps)
            print(json.dumps({"what": "batched, plain DISCHARGE target", "vectors": len(ps),
                              "seconds": round(time.perf_counter() - t0, 4),
                              "ensemble_last_ms": round(model._ensemble_last_ms(), 3)}), flush=True)


if __name__ == "__main__":
    main()
