#!/usr/bin/env python3
"""Ordinary-kriging kernel measurement (not part of bench.py): prints one JSON line.

For each shape (n sources, m destinations, T steps) and each dst_block of the sweep, shyft_hip_ok_bench times the
three kernels of kernels/ok.hip with HIP events (covariance, weights product W = Ainv[0:n] B, values product
out = obs W; best of --reps passes, summed over the destination blocks) and, in the same process, rocBLAS dgemm on
the same two product shapes as kernels/btk.hip calls it. Reported per product: achieved fp64 FMA/s, its fraction of
the measured vector peak (tools/mb/mb_fma64, run first in a process of its own when the binary is there) and the
time relative to rocBLAS. The default shapes are C3's chunk (n = 500, m = 1,048,576, T = 438) and two smaller m.

  python tools/ok_bench.py > profiles/r07/ok_bench.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measured_peak():
    exe = os.path.join(ROOT, "tools", "mb", "mb_fma64")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    return json.loads(out.strip().splitlines()[-1])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sources", type=int, default=500)
    ap.add_argument("--steps", type=int, default=438)
    ap.add_argument("--dst", type=int, nargs="+", default=[65536, 262144, 1048576])
    ap.add_argument("--dst-block", type=int, nargs="+", default=[8192, 16384, 32768, 65536, 131072])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-peak", action="store_true", help="skip the peak micro-benchmark (a profiled run)")
    a = ap.parse_args()

    peak = None if a.no_peak else measured_peak()  # before this process opens the device
    from shyft_amd import _native
    L = _native.lib()
    n, T = a.sources, a.steps
    shapes = []
    for m in a.dst:
        fma_w, fma_v = n * (n + 1) * m, T * n * m
        rows = []
        for blk in a.dst_block:
            if blk > m and rows:
                continue
            ms = (C.c_double * 6)()
            _native.check(L.shyft_hip_ok_bench(a.device, n, T, m, blk, a.reps, ms), None)
            cov, w, v, gw, gv, diff = list(ms)
            row = {"dst_block": blk, "cov_ms": cov, "weights_ms": w, "values_ms": v,
                   "weights_fma_per_s": fma_w / (w * 1e-3), "values_fma_per_s": fma_v / (v * 1e-3),
                   "rocblas_weights_ms": gw, "rocblas_values_ms": gv,
                   "weights_vs_rocblas": w / gw, "values_vs_rocblas": v / gv,
                   "max_abs_diff_vs_rocblas": diff}
            if peak:
                row["weights_fraction_of_peak"] = row["weights_fma_per_s"] / peak["fma_per_s"]
                row["values_fraction_of_peak"] = row["values_fma_per_s"] / peak["fma_per_s"]
            rows.append(row)
        best = min(rows, key=lambda r: r["weights_ms"] + r["values_ms"])
        shapes.append({"n_sources": n, "n_dst": m, "n_steps": T, "weights_fma": fma_w, "values_fma": fma_v,
                       "best_dst_block": best["dst_block"], "sweep": rows})
    print(json.dumps({"bench": "ok_bench", "lib_sha256": _native.lib_sha(), "reps": a.reps,
                      "fp64_fma_peak": peak, "shapes": shapes}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
