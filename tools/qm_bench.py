#!/usr/bin/env python3
"""Quantile-mapping measurement (not part of bench.py): prints one JSON line.

The shape of the reference's qm_speed (test/qm_test.cpp:514-586): 8 forecast sets of 10 forecasts with weights 3..10,
100 scenarios, 336 hourly steps. Set i covers the first 288 + 6 i steps (the sets start six hours apart and the axis
starts where the last one does), the interpolation period is steps 288..311 and the steps from 312 on keep their
scenarios. shyft_hip_quantile_map runs B = 1 and B = 1024 such problems in one call each. Per case: the kernel's
HIP-event milliseconds (shyft_hip_quantile_map_last_ms; --warmup calls, then --reps: best, and the spread), the wall
time of the whole call minus the kernel (allocation and copies), and the wall time of shyft_hip_quantile_map_host on
one thread of the same machine (best of --reps). There is no pass mark.

  python tools/qm_bench.py > profiles/r08/qm_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SETS, N_FC, N_HIST, T = 8, 10, 100, 336
I_START, I_END = 288, 312


def inputs(np, region, B, seed=1):
    rng = np.random.default_rng(seed)
    F = N_SETS * N_FC
    hours = np.arange(T)
    wave = np.sin(2 * 3.14 / T * hours)

    def series(n):  # a + b sin(w t) per series, as qm_test.cpp:537-548 intends
        a = rng.random((B, 1, n)) * 20 - 10.0
        b = rng.random((B, 1, n)) * 5.0
        return a + b * wave[None, :, None]

    fc, pri = series(F), series(N_HIST)
    for i in range(N_SETS):
        fc[:, I_START + 6 * i:, i * N_FC:(i + 1) * N_FC] = np.nan
    w = np.repeat(np.arange(3.0, 3.0 + N_SETS), N_FC)
    mode = np.full(T, region.QM_QM, dtype=np.int32)
    mode[I_START:I_END] = region.QM_BLEND
    mode[I_END:] = region.QM_PRIOR
    iw = np.zeros(T)
    iw[I_START:I_END] = (hours[I_START:I_END] - I_START) / float(I_END - I_START)
    return fc, w, pri, mode, iw


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--problems", type=str, default="1,1024", help="values of B")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch
    from shyft_amd import _native, region

    assert torch.cuda.is_available(), "qm_bench needs a GPU"
    torch.cuda.set_device(0)
    out = {"bench": "qm_bench", "lib_sha256": _native.lib_sha(), "forecasts": N_SETS * N_FC, "scenarios": N_HIST,
           "steps": T, "warmup": a.warmup, "reps": a.reps, "host_threads": 1, "cases": []}
    for B in (int(v) for v in a.problems.split(",")):
        fc, w, pri, mode, iw = inputs(np, region, B)
        for interpolated in (False, True):
            ms, wall, host = [], [], []
            for i in range(a.warmup + a.reps):
                print(f"qm_bench: B={B} interpolated={interpolated} call {i}", file=sys.stderr, flush=True)
                c0 = time.perf_counter()
                dev = region.quantile_map(fc, w, pri, mode, iw, interpolated=interpolated)
                c1 = time.perf_counter()
                if i >= a.warmup:
                    ms.append(region.quantile_map_last_ms())
                    wall.append((c1 - c0) * 1e3)
            for i in range(a.reps):
                c0 = time.perf_counter()
                ref = region.quantile_map(fc, w, pri, mode, iw, interpolated=interpolated, host=True)
                host.append((time.perf_counter() - c0) * 1e3)
            assert np.array_equal(dev, ref, equal_nan=True), "device and host results differ"
            best = min(ms)
            out["cases"].append({
                "problems": B, "jobs": B * T, "interpolated_quantiles": interpolated,
                "path": {region.QM_PATH_WAVE: "WAVE", region.QM_PATH_GROUP: "GROUP"}[region.quantile_map_last_path()],
                "kernel_ms": best, "kernel_all_ms": ms, "kernel_spread": (max(ms) - best) / best,
                "jobs_per_s": B * T / (best * 1e-3), "copy_ms": min(wl - m for wl, m in zip(wall, ms)),
                "host_ms": min(host), "host_all_ms": host, "host_spread": (max(host) - min(host)) / min(host),
                "host_over_kernel": min(host) / best, "host_over_device_call": min(host) / min(wall)})
        del fc, pri
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
