#!/usr/bin/env python3
"""Percentiles-of-a-vector measurement (not part of bench.py): prints one JSON line.

api.percentiles on two shapes:
  a  the reference's documented use (shyft/tests/api/test_time_series.py:485-523): 86 years of hourly values cut into
     80 yearly partitions by partition_by, 365 daily intervals, [0, 10, 25, -1, 50, 75, 90, 100];
  b  an ensemble: 1000 hourly series of one year on their own 8760 intervals, the same list plus -1000 and 1000.
Per shape, after --warmup calls, --reps timings each (best, all, and the spread (max - min) / min) of
  host        api.percentiles(..., host=True): the host twin shyft_hip_ts_percentiles_host;
  device      api.percentiles(..., host=False): wall time of the whole call, and the kernel's HIP-event milliseconds
              (region.ts_percentiles_last_ms);
  unfused     region.resample on the device, then region.percentiles_host: the alternative without the fused kernel
              (it has no extremes, so for shape b it does less than the others);
and the bytes uploaded with the partitions as views and as materialised series. There is no pass mark.

--parent runs on a checkout without the batched entry (the parent commit): it times that checkout's api.percentiles,
the Python host loop, over the same series (the partitions as api.time_shift results, whose making is timed apart as
vector_ms) and prints {"parent": ...};
--merge FILE copies that into this run's line. It needs no GPU.

  python tools/ts_percentiles_bench.py --parent > parent.json      (in the parent checkout)
  python tools/ts_percentiles_bench.py --merge parent.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PCTS_A = [0, 10, 25, -1, 50, 75, 90, 100]
PCTS_B = PCTS_A + [-1000, 1000]


def shape(api, np, name, views):
    """(the TsVector, the time axis, the percentile list, a description); the description's vector_ms is the wall time
    of making the vector from the stored series: partition_by, or without it one api.time_shift per partition"""
    c = api.Calendar()
    rng = np.random.default_rng(1)
    if name == "a":
        t0, common_t0, dt = c.time(1930, 9, 1), c.time(2016, 9, 1), api.deltahours(1)
        n = (common_t0 - t0) // dt
        src = api.TimeSeries(api.TimeAxis(t0, dt, n), 5.0 + 10.0 * rng.random(n), api.POINT_AVERAGE_VALUE)
        year = 365 * 86400  # Calendar.YEAR
        c0 = time.perf_counter()
        if views:
            tsv = src.partition_by(c, t0, year, 80, common_t0)
        else:  # the same vector where partition_by does not exist: calendar years by hand
            tsv = api.TsVector([api.time_shift(src, common_t0 - c.time(1930 + i, 9, 1)) for i in range(80)])
        return tsv, api.TimeAxis(common_t0, api.deltahours(24), 365), PCTS_A, {
            "series": 80, "stored_points": int(n), "steps": 365, "vector_ms": (time.perf_counter() - c0) * 1e3}
    t0, dt, n = c.time(2016, 1, 1), api.deltahours(1), 8760
    ta = api.TimeAxis(t0, dt, n)
    tsv = api.TsVector([api.TimeSeries(ta, 5.0 + 10.0 * rng.random(n), api.POINT_AVERAGE_VALUE) for _ in range(1000)])
    return tsv, ta, PCTS_B, {"series": 1000, "stored_points": 1000 * n, "steps": n}


def timed(fn, warmup, reps, label):
    ms, last = [], None
    for i in range(warmup + reps):
        print(f"ts_percentiles_bench: {label} call {i}", file=sys.stderr, flush=True)
        c0 = time.perf_counter()
        last = fn()
        c1 = time.perf_counter()
        if i >= warmup:
            ms.append((c1 - c0) * 1e3)
    return last, {"ms": min(ms), "all_ms": ms, "spread": (max(ms) - min(ms)) / min(ms)}


def as_arrays(np, tsv):
    return np.array([ts.values for ts in tsv])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", type=str, default="a,b")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--merge", type=str, default="", metavar="FILE")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    from shyft_amd import _native, api
    shapes = [x for x in a.shapes.split(",") if x]
    if a.parent:
        out = {"lib_sha256": _native.lib_sha(), "warmup": a.warmup, "reps": a.reps, "cases": {}}
        for name in shapes:
            tsv, ta, pcts, what = shape(api, np, name, views=False)
            _, t = timed(lambda: api.percentiles(tsv, ta, pcts), a.warmup, a.reps, f"parent {name}")
            out["cases"][name] = dict(what, **t)
        print(json.dumps({"parent": out}))
        return 0

    import torch
    from shyft_amd import region
    assert torch.cuda.is_available(), "ts_percentiles_bench needs a GPU"
    torch.cuda.set_device(0)
    out = {"bench": "ts_percentiles_bench", "lib_sha256": _native.lib_sha(), "warmup": a.warmup, "reps": a.reps,
           "host_threads": 1, "cases": []}
    paths = {region.TS_PERCENTILES_PATH_WAVE: "WAVE", region.TS_PERCENTILES_PATH_LDS: "LDS"}
    for name in shapes:
        tsv, ta, pcts, what = shape(api, np, name, views=True)
        host, t_host = timed(lambda: api.percentiles(tsv, ta, pcts, host=True), a.warmup, a.reps, f"{name} host")
        kernel = []

        def device():
            r = api.percentiles(tsv, ta, pcts, host=False)
            kernel.append(region.ts_percentiles_last_ms())
            return r
        dev, t_dev = timed(device, a.warmup, a.reps, f"{name} device")
        kernel = kernel[a.warmup:]
        h, d = as_arrays(np, host), as_arrays(np, dev)
        assert ((h == d) | (np.isnan(h) & np.isnan(d))).all(), "device and host results differ"
        if name == "a":
            assert all(ts._impl is None for ts in tsv), "a partition was materialised"
        series = [ts._ts for ts in tsv]  # the views become series here: the unfused path has no views
        sort_pcts = [p for p in pcts if abs(p) != 1000]
        _, t_unfused = timed(lambda: region.percentiles_host(region.resample(series, ta), sort_pcts), a.warmup, a.reps,
                             f"{name} unfused")
        points = sum(s.size() for s in series)
        case = dict(what, shape=name, pcts=pcts, path=paths[region.ts_percentiles_last_path()], host=t_host,
                    device_wall=t_dev,
                    device_kernel={"ms": min(kernel), "all_ms": kernel, "spread": (max(kernel) - min(kernel)) / min(kernel)},
                    unfused_wall=t_unfused, unfused_entries=len(sort_pcts),
                    upload_bytes_views=16 * what["stored_points"] + 12 * what["series"],
                    upload_bytes_materialised=16 * points)
        out["cases"].append(case)
        del tsv, series
    if a.merge:
        out["parent"] = json.load(open(a.merge))["parent"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
