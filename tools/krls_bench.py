#!/usr/bin/env python3
"""Batched KRLS training measurement (not part of bench.py): prints one JSON line.

region.krls_train_csr on --series hourly series with the reference's default parameters (dt = 3 h, gamma 1e-3,
tolerance 0.01): a noisy seasonal signal of 8,760 points (a year; the dictionary outgrows the LDS storage, so the
series are trained in the device-memory workspace after the attempt in LDS) and of 720 points (a month; the dictionary
stays in LDS). Per case: the kernels' HIP-event milliseconds (krls_last_ms, all launches of the call; --warmup calls,
best of --reps), the wall time of the whole call minus the kernels (uploads, downloads, allocation: the copies), the
paths and the dictionary sizes reached, the kernels' milliseconds with the LDS storage switched off
(region.krls_set_path), which is the two storages at equal dictionary size, and the wall time of the host restatement
(host=True) on the same inputs, split over --host-procs processes. The prediction of every series at its own points is
timed the same way. There is no pass mark.

  python tools/krls_bench.py > profiles/r09/krls_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOUR = 3600 * 10**6
DT = 3 * HOUR


def inputs(S, n, seed=1):
    import numpy as np
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    v = (np.sin(2 * np.pi * i / 8760.0)[None, :] * rng.uniform(0.5, 2.0, (S, 1))
         + 0.3 * np.sin(2 * np.pi * i / 24.0 + rng.uniform(0, 6.28, (S, 1))) + 0.05 * rng.normal(size=(S, n)))
    v[rng.random((S, n)) < 0.02] = np.nan
    row = n * np.arange(S + 1, dtype=np.int64)
    t = np.tile(HOUR * i.astype(np.int64), S)
    return row, t, v.reshape(-1), np.full(S, n * HOUR, np.int64), np.zeros(S, np.int32)


def host_share(args):
    """the host restatement on series [a, b) of the case, in a process of its own (no GPU is opened)"""
    S, n, a, b = args
    from shyft_amd import region
    row, t, v, t_end, fx = inputs(S, n)
    sl = slice(row[a], row[b])
    c0 = time.perf_counter()
    r = region.krls_train_csr(row[a:b + 1] - row[a], t[sl], v[sl], t_end[a:b], fx[a:b], DT, host=True)
    return time.perf_counter() - c0, [int(x) for x in r[0][1:] - r[0][:-1]]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--series", type=int, default=1000)
    ap.add_argument("--points", type=str, default="8760,720")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--host-procs", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()

    import numpy as np
    from shyft_amd import _native, region

    S = a.series
    out = {"bench": "krls_bench", "lib_sha256": _native.lib_sha(), "series": S, "warmup": a.warmup, "reps": a.reps,
           "dt_hours": 3, "gamma": 1e-3, "tolerance": 0.01, "lds_capacity": region.KRLS_LDS_CAPACITY,
           "max_dict": region.KRLS_MAX_DICT, "cases": []}
    points = [int(x) for x in a.points.split(",")]
    host = {}
    if not a.no_host:  # every host run first, in fresh processes, before this process opens the GPU
        import multiprocessing
        procs = max(1, min(a.host_procs, 16, S))
        cuts = [S * k // procs for k in range(procs + 1)]
        with ProcessPoolExecutor(procs, mp_context=multiprocessing.get_context("spawn")) as ex:
            list(ex.map(host_share, [(1, 24, 0, 1)] * procs))  # the workers are up and have loaded the library
            for n in points:
                print(f"krls_bench: {n} points, host restatement on {procs} processes", file=sys.stderr, flush=True)
                c0 = time.perf_counter()
                shares = list(ex.map(host_share, [(S, n, cuts[k], cuts[k + 1]) for k in range(procs)]))
                # wall_s has the workers' input generation in it, slowest_share_s is the training alone
                host[n] = ({"processes": procs, "wall_s": time.perf_counter() - c0,
                            "slowest_share_s": max(s for s, _ in shares),
                            "thread_seconds": sum(s for s, _ in shares)}, [m for _, ms in shares for m in ms])
    for n in points:
        case = {"points": n}
        if not a.no_host:
            case["host"], host_m = host[n]
        row, t, v, t_end, fx = inputs(S, n)

        def timed(label):
            ms, wall, r = [], [], None
            for i in range(a.warmup + a.reps):
                print(f"krls_bench: {n} points, {label}, call {i}", file=sys.stderr, flush=True)
                c0 = time.perf_counter()
                r = region.krls_train_csr(row, t, v, t_end, fx, DT)
                c1 = time.perf_counter()
                if i >= a.warmup:
                    ms.append(region.krls_last_ms())
                    wall.append((c1 - c0) * 1e3)
            return r, {"kernel_ms": min(ms), "kernel_all_ms": ms, "copy_ms": min(w - k for w, k in zip(wall, ms)),
                       "kernel_ms_per_series": min(ms) / S}

        r, case["train"] = timed("train")
        m = np.diff(r[0])
        case["dictionary"] = {"min": int(m.min()), "median": float(np.median(m)), "max": int(m.max())}
        case["paths"] = {name: int((r[6] == p).sum()) for name, p in
                         (("lds", region.KRLS_PATH_LDS), ("workspace", region.KRLS_PATH_WORKSPACE), ("host", region.KRLS_PATH_HOST))}
        if not a.no_host:
            case["host"]["same_dictionary_sizes"] = bool(host_m == m.tolist())
        region.krls_set_path(region.KRLS_PATH_WORKSPACE)
        try:
            r2, case["train_workspace_only"] = timed("workspace only")
        finally:
            region.krls_set_path(0)
        case["train_workspace_only"]["same_bits"] = bool(
            np.array_equal(r[2].view(np.uint64), r2[2].view(np.uint64)) and (r2[6] != region.KRLS_PATH_LDS).all())
        ms, wall = [], []
        for i in range(a.warmup + a.reps):
            c0 = time.perf_counter()
            region.krls_predict(r[0], r[1], r[2], DT, 1e-3, row, t)
            c1 = time.perf_counter()
            if i >= a.warmup:
                ms.append(region.krls_last_ms())
                wall.append((c1 - c0) * 1e3)
        case["predict"] = {"kernel_ms": min(ms), "copy_ms": min(w - k for w, k in zip(wall, ms))}
        out["cases"].append(case)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
