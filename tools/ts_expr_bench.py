"""Kernel time of the time-series arithmetic (kernels/ts_expr.hip) on one MI355X; one JSON line.

api.TsVector expressions over --series (1,000) hourly series of --points (87,600, ten years), evaluated by
TsVector.evaluate in one device call:
  values   a + b*3.0 - a/2.0 with a and b on the same axis: values mode, three raw loads per point
  at       the same with b on an axis half an hour later: at mode, three searches and interpolations per point on a
           merged axis of twice the points
  pow_max  api.max(a.pow(2.0), b) on the same axis
Per case: the kernel's HIP-event milliseconds (region.ts_expr_last_ms; --warmup calls, then --reps: best, all and the
spread (max - min) / min), the bytes the kernel must read (each terminal's values once per use in values mode, its
times and values once in at mode, plus the output times) and write (the result) per second at the best time, output
points per second, the wall time of the call minus its kernel (planning, uploads, the download), and the wall time of
the host twin on one thread (--host-reps, best). The device result is compared with the host's bit for bit. There is
no pass mark.

  python tools/ts_expr_bench.py --series 200 > profiles/r14/ts_expr_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOUR = 3600


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", type=str, default="values,at,pow_max")
    ap.add_argument("--series", type=int, default=1000)
    ap.add_argument("--points", type=int, default=87600)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()

    import numpy as np
    import torch
    from shyft_amd import _native, api, region

    assert torch.cuda.is_available(), "ts_expr_bench needs a GPU"
    torch.cuda.set_device(0)
    S, n = a.series, a.points
    rng = np.random.default_rng(1)
    t0 = 1230768000

    def vector(start):
        ta = api.TimeAxis(start, HOUR, n)
        return [api.TimeSeries(_impl=api._api._PointTs(ta, rng.normal(5.0, 3.0, n), api.POINT_INSTANT_VALUE))
                for _ in range(S)]

    va, vb, vb_late = vector(t0), vector(t0), vector(t0 + HOUR // 2)
    cases = {
        # name: (expression of one pair, the b operands, terminal reads per output point as (raw, at))
        "values": (lambda x, y: x + y * 3.0 - x / 2.0, vb, (3, 0)),
        "at": (lambda x, y: x + y * 3.0 - x / 2.0, vb_late, (0, 3)),
        "pow_max": (lambda x, y: api.max(x.pow(2.0), y), vb, (2, 0)),
    }
    out = {"bench": "ts_expr_bench", "lib_sha256": _native.lib_sha(), "series": S, "points_per_series": n,
           "warmup": a.warmup, "reps": a.reps, "host_reps": a.host_reps, "host_threads": 1, "cases": []}
    for name in [x for x in a.cases.split(",") if x]:
        f, other, (raw, at) = cases[name]
        make = lambda: api.TsVector([f(x, y) for x, y in zip(va, other)])  # noqa: E731  (fresh, unevaluated trees)
        host = []
        for i in range(a.host_reps):
            print(f"ts_expr_bench: {name} host call {i}", file=sys.stderr, flush=True)
            v = make()
            c0 = time.perf_counter()
            ref = v.evaluate(host=True)
            host.append((time.perf_counter() - c0) * 1e3)
        ms, wall = [], []
        for i in range(a.warmup + a.reps):
            print(f"ts_expr_bench: {name} device call {i}", file=sys.stderr, flush=True)
            v = make()
            c0 = time.perf_counter()
            dev = v.evaluate()
            c1 = time.perf_counter()
            if i >= a.warmup:
                ms.append(region.ts_expr_last_ms())
                wall.append((c1 - c0) * 1e3)
        n_out = 0
        for d, h in zip(dev, ref):
            x, y = d._ts._values, h._ts._values
            nan = np.isnan(y)
            assert np.array_equal(nan, np.isnan(x)) and np.array_equal(x[~nan], y[~nan]), "device and host results differ"
            n_out += len(x)
        best = min(ms)
        # a raw load reads 8 bytes; an at-mode load reads the terminal's times and values once (its searches hit the
        # cache after that): 16 bytes per terminal point, and a terminal has about half as many points as the merged axis
        read = n_out * (8 + 8 * raw) + S * n * 16 * at
        out["cases"].append({"case": name, "output_points": n_out, "kernel_ms": best, "kernel_all_ms": ms,
                             "kernel_spread": (max(ms) - best) / best, "points_per_s": n_out / (best * 1e-3),
                             "read_bytes": read, "written_bytes": 8 * n_out,
                             "read_GB_per_s": read / (best * 1e-3) / 1e9, "written_GB_per_s": 8 * n_out / (best * 1e-3) / 1e9,
                             "call_minus_kernel_ms": min(w - m for w, m in zip(wall, ms)), "host_ms": min(host),
                             "host_all_ms": host, "host_over_kernel": min(host) / best,
                             "host_over_device_call": min(host) / min(wall)})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
