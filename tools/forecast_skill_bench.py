#!/usr/bin/env python3
"""Forecast-skill measurement (not part of bench.py): prints one JSON line.

shyft_hip_forecast_skill on one lead-time table: --locations (64) locations x --leads (240) hourly lead times, each
cell --forecasts (360) forecasts of 240 hourly average-value points issued 6 h apart against the location's hourly
observation, n = 6 slices of 1 h. A location's forecasts and observation are in the pool once; its 240 problems name
them. The kernel's HIP-event milliseconds (shyft_hip_forecast_skill_last_ms; --warmup calls, then --reps: best, and
the spread), the wall time of the whole call minus the kernel (allocation and copies), and the wall time of
shyft_hip_forecast_skill_host on one thread of the same machine (best of --host-reps), whose scores the device's must
equal bit for bit. There is no pass mark.

  python tools/forecast_skill_bench.py
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
POINTS = 240


def table(np, locations, leads, forecasts):
    """(row, t, v, t_end, fx), (fc_row, fc_ix, obs_ix, t0_offset, dt, n)"""
    rng = np.random.default_rng(1)
    n_obs = 6 * forecasts + 2 * POINTS
    per_loc = forecasts + 1  # the forecasts of a location, then its observation
    lengths = np.tile(np.append(np.full(forecasts, POINTS), n_obs), locations)
    row = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    start = np.tile(np.append(T0 + 6 * HOUR * np.arange(forecasts, dtype=np.int64), T0), locations)
    t = np.concatenate([s + HOUR * np.arange(n, dtype=np.int64) for s, n in zip(start, lengths)])
    hours = (t - T0) // HOUR
    v = np.sin(0.314 + 3.14 * hours / 240.0) + rng.normal(0.0, 0.1, t.shape[0])
    t_end = start + HOUR * lengths
    fx = np.ones(lengths.shape[0], dtype=np.int32)
    P = locations * leads
    loc = np.repeat(np.arange(locations, dtype=np.int64), leads)
    fc_row = forecasts * np.arange(P + 1, dtype=np.int64)
    fc_ix = (loc[:, None] * per_loc + np.arange(forecasts, dtype=np.int64)[None, :]).reshape(-1)
    obs_ix = loc * per_loc + forecasts
    t0_offset = np.tile(HOUR * np.arange(leads, dtype=np.int64), locations)
    return (row, t, v, t_end.astype(np.int64), fx), (fc_row, fc_ix, obs_ix, t0_offset, HOUR, 6)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--locations", type=int, default=64)
    ap.add_argument("--leads", type=int, default=240)
    ap.add_argument("--forecasts", type=int, default=360)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()

    import numpy as np
    import torch
    from shyft_amd import _native, region

    assert torch.cuda.is_available(), "forecast_skill_bench needs a GPU"
    torch.cuda.set_device(0)
    batch, prob = table(np, a.locations, a.leads, a.forecasts)
    P, jobs = a.locations * a.leads, a.locations * a.leads * a.forecasts * 6
    ms, wall = [], []
    for i in range(a.warmup + a.reps):
        print(f"forecast_skill_bench: device call {i}", file=sys.stderr, flush=True)
        c0 = time.perf_counter()
        dev = region.forecast_skill_csr(*batch, *prob)
        c1 = time.perf_counter()
        if i >= a.warmup:
            ms.append(region.forecast_skill_last_ms())
            wall.append((c1 - c0) * 1e3)
    host = []
    for i in range(a.host_reps):
        print(f"forecast_skill_bench: host call {i}", file=sys.stderr, flush=True)
        c0 = time.perf_counter()
        ref = region.forecast_skill_csr(*batch, *prob, host=True)
        host.append((time.perf_counter() - c0) * 1e3)
    if host:
        nan = np.isnan(ref)
        assert np.array_equal(nan, np.isnan(dev)) and np.array_equal(dev[~nan], ref[~nan]), "device and host scores differ"
    best = min(ms)
    out = {"bench": "forecast_skill_bench", "lib_sha256": _native.lib_sha(), "warmup": a.warmup, "reps": a.reps,
           "host_threads": 1, "locations": a.locations, "lead_times": a.leads, "forecasts": a.forecasts,
           "forecast_points": POINTS, "n": 6, "problems": P, "jobs": jobs, "points": int(batch[0][-1]),
           "finite_scores": int(np.isfinite(dev).sum()), "kernel_ms": best, "kernel_all_ms": ms,
           "kernel_spread": (max(ms) - best) / best, "jobs_per_s": jobs / (best * 1e-3),
           "copy_ms": min(wl - m for wl, m in zip(wall, ms))}
    if host:
        out.update({"host_ms": min(host), "host_all_ms": host, "host_over_kernel": min(host) / best,
                    "host_over_device_call": min(host) / min(wall)})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
