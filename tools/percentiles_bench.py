#!/usr/bin/env python3
"""Cell-percentile kernel measurement (not part of bench.py): prints one JSON line.

A region of --cells cells (default 1,048,576) holds --steps (438) resident steps of synthetic forcing
(shyft_hip_synthetic_forcing). Percentiles [0, 10, 25, 50, -1, 75, 90, 100] of one forcing variable are taken
  (a) over all cells as one segment (shyft_hip_percentiles), and
  (b) per catchment for every catchment count of --catchments (shyft_hip_catchment_percentiles, result on the device),
each timed with HIP events on the region's stream (shyft_hip_last_percentiles_ms: the kernels, first launch to
last) after --warmup calls, --reps times. Two reference values are timed in the same process with HIP events on
the same [steps][cells] device tensor:
  torch.sort along the cell dimension (what a full sort on the device costs), and
  a plain read of the rows, torch.sum over the cell dimension (one pass over the tensor: the HBM floor of a pass).
Reported: best and median ms of each, (a) relative to the sort and to the one-pass read, the read's bytes/s, and
whether (a) equals the host restatement on --check-steps steps.

  python tools/percentiles_bench.py > profiles/r07/percentiles_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PCTS = [0, 10, 25, 50, -1, 75, 90, 100]


def summary(ms):
    return {"best_ms": min(ms), "median_ms": statistics.median(ms), "all_ms": ms}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cells", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=438)
    ap.add_argument("--var", type=int, default=0, help="forcing variable (0 temperature .. 4 radiation)")
    ap.add_argument("--catchments", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-steps", type=int, default=3)
    ap.add_argument("--path", type=int, default=0, help="0 auto, 1 LDS sort, 2 radix select")
    a = ap.parse_args()

    import numpy as np
    import torch
    from shyft_amd import _native, synthetic
    from shyft_amd.region import (HipRegion, KNOB_PERCENTILES_PATH, PT_GS_K, SCOPE_CATCHMENT, SERIES_FORCING,
                                  percentiles_host)

    assert torch.cuda.is_available(), "percentiles_bench needs a GPU"
    torch.cuda.set_device(0)
    n, T, series = a.cells, a.steps, SERIES_FORCING + a.var
    geo = synthetic.geo11(n, n_catchments=1)
    r = HipRegion(PT_GS_K, n, device=0)
    r.set_geo(geo)
    r.set_time_axis(synthetic.T0_2015_US, synthetic.HOUR_US, T)
    r.synthetic_forcing(synthetic.SEED, 0, T)
    r.set_test_knob(KNOB_PERCENTILES_PATH, a.path)

    def timed(call):
        for _ in range(a.warmup):
            call()
        ms = []
        for _ in range(a.reps):
            call()
            ms.append(r.last_percentiles_ms())
        return summary(ms)

    out = {"bench": "percentiles_bench", "lib_sha256": _native.lib_sha(), "cells": n, "steps": T, "variable": a.var,
           "percentiles": PCTS, "warmup": a.warmup, "reps": a.reps}

    # (a) all cells as one segment
    res = {}
    all_cells = timed(lambda: res.__setitem__("v", r.percentiles(series, PCTS, [], SCOPE_CATCHMENT, 0, T)))
    all_cells["path"] = r.percentiles_path()
    rows = r.get_forcing(a.var, 0, a.check_steps)
    want = percentiles_host(rows, PCTS)
    got = res["v"][:, :a.check_steps]
    k_avg = PCTS.index(-1)
    sel = [k for k in range(len(PCTS)) if k != k_avg]
    all_cells["order_statistics_equal_host"] = bool(np.array_equal(got[sel], want[sel]))
    all_cells["average_max_abs_diff_vs_host"] = float(np.abs(got[k_avg] - want[k_avg]).max())
    out["all_cells"] = all_cells

    # (b) every catchment in one call, result left on the device
    out["catchment_percentiles"] = []
    for C in a.catchments:
        geo[:, 4] = 1 + (np.arange(n, dtype=np.int64) * C) // n  # contiguous catchments of n / C cells
        r.set_geo(geo)
        dst = torch.empty((C, len(PCTS), T), dtype=torch.float64, device="cuda")
        row = timed(lambda: r.catchment_percentiles_device(series, PCTS, 0, T, dst.data_ptr()))
        row.update({"catchments": C, "cells_per_catchment": n // C, "path": r.percentiles_path()})
        out["catchment_percentiles"].append(row)
        del dst

    # the reference values on the same tensor
    x = torch.empty((T, n), dtype=torch.float64, device="cuda")
    r.get_forcing_device(a.var, 0, T, x.data_ptr())
    r.close()

    def timed_torch(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return summary(ms)

    read = timed_torch(lambda: x.sum(dim=1))
    read["bytes"] = T * n * 8
    read["bytes_per_s"] = read["bytes"] / (read["best_ms"] * 1e-3)
    out["row_sum_read"] = read
    out["torch_sort"] = timed_torch(lambda: torch.sort(x, dim=1))
    out["all_cells_vs_torch_sort"] = all_cells["best_ms"] / out["torch_sort"]["best_ms"]
    out["all_cells_vs_one_pass_read"] = all_cells["best_ms"] / read["best_ms"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
