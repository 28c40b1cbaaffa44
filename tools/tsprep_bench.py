"""Kernel times of the observation-preparation calls (kernels/tsprep.hip) on one MI355X; one JSON line.

region.ts_ice_packing_csr, ts_ice_packing_recession_csr, ts_min_max_fill_csr and ts_rating_curve_csr on three shapes:
  a  --series (1,000) hourly series of --points (87,600, ten years): temperatures with a cold spell of some weeks in
     each year through ice_packing at their own points (window 5 days, threshold -8, ALLOW_ANY_MISSING), then flows
     through ice_packing_recession with that indicator (alpha 1/(7 d), minimum 0.5): the parameters of the reference's
     ice_speed case (test/test_ice_packing.cpp:119-159)
  b  the same with about 20 % NaN and irregular times
  c  water levels with 5 % out-of-range points through min_max_fill (limits 0 .. 10, 6 hours), then a two-curve,
     three-segment rating
Per operation: the kernels' HIP-event milliseconds (region.tsprep_last_ms; --warmup calls, then --reps: best, all and
the spread (max - min) / min), the wall time of the call minus its kernels (uploads, the download, allocation and the
argument checks), and the wall time of the _host twin on one thread of the same machine (--host-reps, best). The device
result is compared with the host's bit for bit. There is no pass mark.

  python tools/tsprep_bench.py > profiles/r10/tsprep_bench.json
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
DAY = 24 * HOUR
T0 = 1230768000 * 10**6  # 2009-01-01


def shape(np, name, S, n):
    """(row, t, t_end, fx, temperature, flow, level)"""
    rng = np.random.default_rng(1)
    t = T0 + HOUR * np.arange(n, dtype=np.int64)[None, :] + np.zeros((S, 1), dtype=np.int64)
    t_end = np.full(S, T0 + HOUR * n, dtype=np.int64)
    year = 2.0 * np.pi * np.arange(n) / (365.0 * 24.0)
    temperature = 4.0 - 14.0 * np.cos(year)[None, :] + rng.normal(0.0, 2.0, (S, n))  # below -8 for about six weeks
    flow = 10.0 + 5.0 * rng.random((S, n))
    level = 5.0 + 2.0 * np.sin(7.0 * year)[None, :] + rng.normal(0.0, 0.5, (S, n))
    if name == "b":
        off = rng.integers(0, HOUR, (S, n), dtype=np.int64)
        off[:, 0] = 0
        t = t + off
        t_end = t[:, -1] + 1 + rng.integers(0, HOUR, S, dtype=np.int64)
        temperature[rng.random((S, n)) < 0.2] = np.nan
        flow[rng.random((S, n)) < 0.2] = np.nan
    if name == "c":
        bad = rng.random((S, n)) < 0.05
        level[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -50.0, 50.0)
    row = n * np.arange(S + 1, dtype=np.int64)
    return (row, t.reshape(-1), t_end, np.ones(S, dtype=np.int32), temperature.reshape(-1), flow.reshape(-1),
            level.reshape(-1))


def measure(np, region, what, call, warmup, reps, host_reps):
    host = []
    for i in range(host_reps):
        print(f"tsprep_bench: {what} host call {i}", file=sys.stderr, flush=True)
        c0 = time.perf_counter()
        ref = call(host=True)
        host.append((time.perf_counter() - c0) * 1e3)
    ms, wall = [], []
    for i in range(warmup + reps):
        print(f"tsprep_bench: {what} device call {i}", file=sys.stderr, flush=True)
        c0 = time.perf_counter()
        dev = call()
        c1 = time.perf_counter()
        if i >= warmup:
            ms.append(region.tsprep_last_ms())
            wall.append((c1 - c0) * 1e3)
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(dev)) and np.array_equal(dev[~nan], ref[~nan]), "device and host results differ"
    best = min(ms)
    return dev, {"kernel_ms": best, "kernel_all_ms": ms, "kernel_spread": (max(ms) - best) / best,
                 "points_per_s": dev.shape[0] / (best * 1e-3), "call_minus_kernel_ms": min(w - m for w, m in zip(wall, ms)),
                 "host_ms": min(host), "host_all_ms": host, "host_spread": (max(host) - min(host)) / min(host),
                 "host_over_kernel": min(host) / best, "host_over_device_call": min(host) / min(wall),
                 "nan_share": float(np.mean(nan))}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", type=str, default="a,b,c")
    ap.add_argument("--series", type=int, default=1000)
    ap.add_argument("--points", type=int, default=87600)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()

    import numpy as np
    import torch
    from shyft_amd import _native, region

    assert torch.cuda.is_available(), "tsprep_bench needs a GPU"
    torch.cuda.set_device(0)
    out = {"bench": "tsprep_bench", "lib_sha256": _native.lib_sha(), "warmup": a.warmup, "reps": a.reps,
           "host_reps": a.host_reps, "host_threads": 1, "cases": []}
    S, n = a.series, a.points
    for name in [x for x in a.shapes.split(",") if x]:
        row, t, t_end, fx, temperature, flow, level = shape(np, name, S, n)
        base = {"shape": name, "series": S, "points": int(row[-1])}

        def add(op, what, call):
            dev, r = measure(np, region, f"{name} {op}", call, a.warmup, a.reps, a.host_reps)
            out["cases"].append({**base, "op": op, "parameters": what, **r})
            return dev

        if name in ("a", "b"):
            ice = add("ice_packing", "window 5 d, threshold -8, ALLOW_ANY_MISSING, own points",
                      lambda **kw: region.ts_ice_packing_csr(row, t, temperature, t_end, fx, row, t, 5 * DAY, -8.0,
                                                             region.ICE_ALLOW_ANY_MISSING, **kw))
            out["cases"][-1]["ice_share"] = float(np.mean(ice == 1.0))
            add("ice_packing_recession", "alpha 1/(7 d), minimum 0.5",
                lambda **kw: region.ts_ice_packing_recession_csr(row, t, flow, t_end, fx, ice, T0, int(t_end.max()),
                                                                 1.0 / (7 * 86400.0), 0.5, **kw))
        else:
            filled = add("min_max_fill", "limits 0 .. 10, max_timespan 6 h",
                         lambda **kw: region.ts_min_max_fill_csr(row, t, level, t_end, fx, 0.0, 10.0, 6 * HOUR, **kw))
            segs = [[0.0, 1.2, -0.1, 1.6], [4.0, 2.0, 0.5, 2.0], [7.0, 0.8, 1.0, 2.5],
                    [0.0, 1.3, -0.1, 1.6], [4.5, 2.1, 0.5, 2.0], [7.5, 0.9, 1.0, 2.5]]
            add("rating_curve", "one pack, 2 curves of 3 segments",
                lambda **kw: region.ts_rating_curve_csr(row, t, filled, t_end, fx, [0, 2], [T0, T0 + (n // 2) * HOUR],
                                                        [0, 3, 6], segs, 0, **kw))
        del row, t, t_end, fx, temperature, flow, level
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
