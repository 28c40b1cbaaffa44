"""Kernel time of convolve_w (kernels/tsfilter.hip) on one MI355X, DIRECT against TILED; one JSON document.

region.ts_convolve_w_csr on one batch of --series (1,024) evenly spaced series of --points (8,760) each, one shared
profile of K weights for every K of --weights, USE_FIRST. Per K the two paths alternate call by call (--warmup calls
each, then --reps): the kernel's HIP-event milliseconds (region.tsfilter_last_ms) as median, min and max. For the K of
--host-weights the host twin runs once on one thread (wall seconds) and both paths are compared with it bit for bit.
Beside the times stand the two floors: 16 bytes per point over 6.3 TB/s (the HBM rate a copy reaches) and 2 K
operations per point over 3.86e13 fp64 vector instructions per second (tools/mb/mb_fma64; a separate multiply and add
are two instructions). A second table times both paths at K = 64 on the same number of points in short series
(--short lengths), where the tiles are mostly empty. There is no pass mark.

  python tools/tsfilter_bench.py > profiles/r17/tsfilter_convolve.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--series", type=int, default=1024)
    ap.add_argument("--points", type=int, default=8760)
    ap.add_argument("--weights", type=str, default="2,4,8,16,32,64,512")
    ap.add_argument("--host-weights", type=str, default="8,64,512")
    ap.add_argument("--short", type=str, default="16,64,128")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()

    import numpy as np
    import torch
    from shyft_amd import _native, region
    from tests import resample_cases as rc

    assert torch.cuda.is_available(), "tsfilter_bench needs a GPU"
    torch.cuda.set_device(0)
    rng = np.random.default_rng(1)
    t0, dt = rc.EPOCHS[0]

    def batch(S, n):
        return (np.arange(S + 1, dtype=np.int64) * n, np.tile(t0 + dt * np.arange(n, dtype=np.int64), S),
                rng.normal(5.0, 10.0, S * n), np.full(S, t0 + dt * n, np.int64), np.ones(S, np.int32))

    def timed(b, w, host):
        """{path: [ms, ...]} with the paths alternating, and whether each path equals `host` bit for bit"""
        ms, same = {region.TSFILTER_PATH_DIRECT: [], region.TSFILTER_PATH_TILED: []}, {}
        try:
            for rep in range(a.warmup + a.reps):
                for path in ms:
                    region.tsfilter_set_path(path)
                    dev = region.ts_convolve_w_csr(*b, [0, len(w)], w, 0, region.CONVOLVE_USE_FIRST)
                    assert region.tsfilter_last_path() == path
                    if rep >= a.warmup:
                        ms[path].append(region.tsfilter_last_ms())
                    if rep == 0 and host is not None:
                        same["direct" if path == region.TSFILTER_PATH_DIRECT else "tiled"] = bool(rc.same_bits(dev, host))
        finally:
            region.tsfilter_set_path(region.TSFILTER_PATH_AUTO)
        return ms, same

    def stats(name, x):
        return {f"{name}_ms_median": float(np.median(x)), f"{name}_ms_min": float(np.min(x)), f"{name}_ms_max": float(np.max(x))}

    points = a.series * a.points
    out = {"library": _native.lib_sha()[:8],
           "series": a.series, "points_per_series": a.points, "warmup": a.warmup, "reps": a.reps,
           "floor_hbm_ms": 16.0 * points / 6.3e12 * 1e3, "long": [], "short": []}
    b = batch(a.series, a.points)
    host_ks = {int(k) for k in a.host_weights.split(",") if k}
    for K in (int(k) for k in a.weights.split(",")):
        w = rng.normal(0.0, 1.0, K)
        host = host_s = None
        if K in host_ks:
            c0 = time.perf_counter()
            host = region.ts_convolve_w_csr(*b, [0, K], w, 0, region.CONVOLVE_USE_FIRST, host=True)
            host_s = time.perf_counter() - c0
        ms, same = timed(b, w, host)
        out["long"].append({"K": K, **stats("direct", ms[region.TSFILTER_PATH_DIRECT]),
                            **stats("tiled", ms[region.TSFILTER_PATH_TILED]), "host_wall_s": host_s,
                            "bit_identical_to_host": same, "floor_fp64_ms": 2.0 * K * points / 3.86e13 * 1e3})
    for n in (int(x) for x in a.short.split(",") if x):
        S = max(1, points // n // 8)
        ms, _ = timed(batch(S, n), rng.normal(0.0, 1.0, 64), None)
        out["short"].append({"points_per_series": n, "series": S, "K": 64, **stats("direct", ms[region.TSFILTER_PATH_DIRECT]),
                             **stats("tiled", ms[region.TSFILTER_PATH_TILED])})
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
