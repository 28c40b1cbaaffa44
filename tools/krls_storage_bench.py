#!/usr/bin/env python3
"""The two storages of kernels/krls.hip at equal dictionary size (not part of bench.py): prints one JSON line.

region.krls_train_csr on 1, 64, 256 and 1,000 series, once as the entry chooses (both matrices in LDS) and once with
the LDS storage switched off (region.krls_set_path: the device-memory workspace), for three kinds of series: 720
hourly points at the reference's defaults (23 dictionary entries, mostly update steps), 95 points that all join the
dictionary (growth steps only), and those 95 points trained over eight passes (growth, then 665 update steps at 95
entries). Per case the kernels' HIP-event milliseconds, best of three calls after one. There is no pass mark.

  python tools/krls_storage_bench.py > profiles/r18/krls_storage_paths.json
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from shyft_amd import region

HOUR = 3600 * 10**6


def batch(S, n, seed=1):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(S, n))
    row = n * np.arange(S + 1, dtype=np.int64)
    t = np.tile(HOUR * np.arange(n, dtype=np.int64), S)
    return row, t, v.reshape(-1), np.full(S, n * HOUR, np.int64), np.zeros(S, np.int32)


def best(args, kw, reps=3):
    ms = []
    for _ in range(reps + 1):
        r = region.krls_train_csr(*args, **kw)
        ms.append(region.krls_last_ms())
    return min(ms[1:]), r


def main() -> int:
    out = []
    for name, n, dt, kw in (("m23", 720, 3 * HOUR, dict(gamma=1e-3, tolerance=0.01)),
                            ("m95_grow", 95, HOUR, dict(gamma=0.5, tolerance=0.001)),
                            ("m95_grow_then_update", 95, HOUR, dict(gamma=0.5, tolerance=0.001, iterations=8, mse_tol=0.0))):
        for S in (1, 64, 256, 1000):
            args = batch(S, n) + (dt,)
            region.krls_set_path(0)
            lds, r = best(args, kw)
            region.krls_set_path(region.KRLS_PATH_WORKSPACE)
            try:
                ws, r2 = best(args, kw)
            finally:
                region.krls_set_path(0)
            out.append(dict(case=name, series=S, dict=int(np.diff(r[0]).max()), lds_ms=lds, ws_ms=ws,
                            lds_paths=int((r[6] == region.KRLS_PATH_LDS).sum()),
                            ws_paths=int((r2[6] == region.KRLS_PATH_WORKSPACE).sum())))
            print(out[-1], file=sys.stderr, flush=True)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
