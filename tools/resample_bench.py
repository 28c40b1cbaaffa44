#!/usr/bin/env python3
"""Resampling measurement (not part of bench.py): prints one JSON line.

shyft_hip_resample on three shapes:
  a  the region's own: 500 series of 3-hourly instant points over a year (2,920 points each) onto 8,760 hourly steps;
  b  10,000 hourly average-value series over a year onto 365 daily steps;
  c  shape a with about 20 % NaN and irregular point times.
Per shape, mode and launch shape (DIRECT: one lane per job; TILED: 16 series x 64 intervals per workgroup through
LDS): the kernels' HIP-event milliseconds (shyft_hip_resample_last_ms; --warmup calls, then --reps: best, and the
spread), the wall time of the whole call minus the kernels (allocation and copies), and the wall time of
shyft_hip_resample_host on one thread of the same machine (best of --reps). There is no pass mark.

--run-interpolation CELLS also times model.run_interpolation (pt_gs_k, IDW for all five variables) with 500 sources
of shape a per variable on CELLS cells: wall milliseconds of --reps calls after --warmup. The same option works on a
checkout without shyft_hip_resample (--shapes ""), which is how the parent commit is timed; --merge FILE copies that
run's "run_interpolation" entry into this one's as "run_interpolation_parent".

  python tools/resample_bench.py --run-interpolation 2000 --merge parent.json > profiles/r09/resample_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOUR = 3600 * 10**6
T0 = 1451606400 * 10**6  # 2016-01-01


def shape(np, name):
    """(row, t, v, t_end, fx), (ta_t0, ta_dt, T)"""
    rng = np.random.default_rng(1)
    if name == "b":
        S, n, dt, fx, axis = 10000, 8760, HOUR, 1, (T0, 24 * HOUR, 365)
    else:
        S, n, dt, fx, axis = 500, 2920, 3 * HOUR, 0, (T0, HOUR, 8760)
    t = T0 + dt * np.arange(n, dtype=np.int64)[None, :] + np.zeros((S, 1), dtype=np.int64)
    v = 5.0 + 10.0 * rng.random((S, n))
    t_end = np.full(S, T0 + dt * n, dtype=np.int64)
    if name == "c":
        off = rng.integers(0, dt, (S, n), dtype=np.int64)
        off[:, 0] = 0
        t = t + off
        t_end = t[:, -1] + 1 + rng.integers(0, dt, S, dtype=np.int64)
        v[rng.random((S, n)) < 0.2] = np.nan
    row = n * np.arange(S + 1, dtype=np.int64)
    return (row, t.reshape(-1), v.reshape(-1), t_end, np.full(S, fx, dtype=np.int32)), axis


def run_interpolation(np, cells, warmup, reps):
    from shyft_amd import api
    from shyft_amd.api import pt_gs_k
    rng = np.random.default_rng(2)
    side = int(np.ceil(np.sqrt(cells)))
    gcds = api.GeoCellDataVector()
    for i in range(cells):
        gp = api.GeoPoint(500.0 + 1000.0 * (i % side), 500.0 + 1000.0 * (i // side), 1500.0 * rng.random())
        gcds.append(api.GeoCellData(gp, 1000.0 * 1000.0, 1, 0.9, api.LandTypeFractions(0.01, 0.05, 0.19, 0.3, 0.45)))
    model = pt_gs_k.PTGSKModel(gcds, pt_gs_k.PTGSKParameter())
    src_axis = api.TimeAxis(T0 // 10**6, 3 * 3600, 2920)
    env = api.ARegionEnvironment()
    env.radiation = api.RadiationSourceVector()
    kinds = ((env.temperature, api.TemperatureSource, 5.0, 8.0), (env.precipitation, api.PrecipitationSource, 1.0, 1.0),
             (env.radiation, api.RadiationSource, 200.0, 100.0), (env.wind_speed, api.WindSpeedSource, 3.0, 2.0),
             (env.rel_hum, api.RelHumSource, 0.6, 0.2))
    for vec, src_t, base, span in kinds:
        for _ in range(500):
            gp = api.GeoPoint(1000.0 * side * rng.random(), 1000.0 * side * rng.random(), 1500.0 * rng.random())
            vec.append(src_t(gp, api.TimeSeries(src_axis, base + span * rng.random(2920), api.POINT_INSTANT_VALUE)))
    ip = api.InterpolationParameter()
    ip.use_idw_for_temperature = True
    for p in (ip.temperature_idw, ip.precipitation, ip.radiation, ip.wind_speed, ip.rel_hum):
        p.max_distance = 1e7
    ta = api.TimeAxis(T0 // 10**6, 3600, 8760)
    ms = []
    for i in range(warmup + reps):
        print(f"resample_bench: run_interpolation call {i}", file=sys.stderr, flush=True)
        c0 = time.perf_counter()
        ok = model.run_interpolation(ip, ta, env)
        c1 = time.perf_counter()
        assert ok
        if i >= warmup:
            ms.append((c1 - c0) * 1e3)
    return {"cells": cells, "sources_per_variable": 500, "source_points": 2920, "steps": 8760, "wall_all_ms": ms,
            "wall_ms": min(ms), "wall_spread": (max(ms) - min(ms)) / min(ms)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", type=str, default="a,b,c")
    ap.add_argument("--run-interpolation", type=int, default=0, metavar="CELLS")
    ap.add_argument("--merge", type=str, default="", metavar="FILE")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch
    from shyft_amd import _native, region

    assert torch.cuda.is_available(), "resample_bench needs a GPU"
    torch.cuda.set_device(0)
    out = {"bench": "resample_bench", "lib_sha256": _native.lib_sha(), "warmup": a.warmup, "reps": a.reps,
           "host_threads": 1, "cases": []}
    shapes = [x for x in a.shapes.split(",") if x]
    if shapes:
        modes = {"AVERAGE": region.RESAMPLE_AVERAGE, "INTEGRAL": region.RESAMPLE_INTEGRAL,
                 "ACCUMULATE": region.RESAMPLE_ACCUMULATE}
        paths = {"DIRECT": region.RESAMPLE_PATH_DIRECT, "TILED": region.RESAMPLE_PATH_TILED}
    for name in shapes:
        batch, (ta_t0, ta_dt, T) = shape(np, name)
        S = batch[0].shape[0] - 1
        for mode_name in ("AVERAGE", "ACCUMULATE") if name != "c" else ("AVERAGE",):
            mode = modes[mode_name]
            host = []
            for i in range(a.reps):
                c0 = time.perf_counter()
                ref = region.resample_csr(*batch, ta_t0, ta_dt, T, mode, host=True)
                host.append((time.perf_counter() - c0) * 1e3)
            for path_name, path in paths.items():
                region.resample_set_path(path)
                ms, wall = [], []
                for i in range(a.warmup + a.reps):
                    print(f"resample_bench: {name} {mode_name} {path_name} call {i}", file=sys.stderr, flush=True)
                    c0 = time.perf_counter()
                    dev = region.resample_csr(*batch, ta_t0, ta_dt, T, mode)
                    c1 = time.perf_counter()
                    if i >= a.warmup:
                        ms.append(region.resample_last_ms())
                        wall.append((c1 - c0) * 1e3)
                nan = np.isnan(ref)
                assert np.array_equal(nan, np.isnan(dev)) and np.array_equal(dev[~nan], ref[~nan]), \
                    "device and host results differ"
                best = min(ms)
                out["cases"].append({
                    "shape": name, "series": S, "points": int(batch[0][-1]), "steps": T, "jobs": S * T,
                    "mode": mode_name, "path": path_name, "kernel_ms": best, "kernel_all_ms": ms,
                    "kernel_spread": (max(ms) - best) / best, "jobs_per_s": S * T / (best * 1e-3),
                    "copy_ms": min(wl - m for wl, m in zip(wall, ms)), "host_ms": min(host), "host_all_ms": host,
                    "host_spread": (max(host) - min(host)) / min(host), "host_over_kernel": min(host) / best,
                    "host_over_device_call": min(host) / min(wall)})
        del batch
    if shapes:
        region.resample_set_path(region.RESAMPLE_PATH_AUTO)
    if a.run_interpolation:
        out["run_interpolation"] = run_interpolation(np, a.run_interpolation, a.warmup, a.reps)
    if a.merge:
        out["run_interpolation_parent"] = json.load(open(a.merge))["run_interpolation"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
