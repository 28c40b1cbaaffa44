#!/usr/bin/env python3
"""Batched Kalman filter measurement (not part of bench.py): prints one JSON line.

shyft_hip_kalman_run on M points of size n over T steps of a 3-hourly axis (24/n-hourly for n = 24), about 10 % of
the bias missing, in update mode (predictor mode, no running bias) and in running-bias mode. Cases: n = 8 at
M = 1,048,576 and n = 24 at M = 262,144, T = 80 (ten days). Per case: the kernel's HIP-event milliseconds
(shyft_hip_kalman_last_ms; --warmup calls, best of --reps), point-steps per second, and the wall time of the whole
call minus the kernel (uploads, downloads, allocation: the copy time). The host restatement
(shyft_hip_kalman_run_host, one thread) is timed on --host-points points. Beside the times stands the static count
of vector-ALU instructions in the kernel's step loop, from its disassembly (hipcc -S on kernels/kalman.hip with the
library's flags), and the time those instructions alone would take at the fp64 vector issue rate measured by
tools/mb/mb_fma64 (3.86e13 lane-FMA/s = 6.03e11 wave-instructions/s), so a reader sees how far the kernel is from
its instruction floor. There is no pass mark.

  python tools/kalman_bench.py > profiles/r07/kalman_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAVE_INSTRUCTIONS_PER_S = 3.86e13 / 64  # tools/mb/mb_fma64


def static_valu():
    """{G: {"step_loop": VALU instructions in the step loop without the piece loop, "piece_loop": per piece,
    "ds_bpermute": cross-lane reads in the step loop, "lines": instructions in the step loop}} from the disassembly"""
    csrc = os.path.join(ROOT, "shyft_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        s_path = os.path.join(tmp, "kalman.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Wno-unused-function", "--cuda-device-only", "-S", "-o", s_path, "kernels/kalman.hip"],
                       check=True, cwd=csrc, capture_output=True)
        text = open(s_path).read().splitlines()
    out = {}
    starts = [(i, int(m.group(1))) for i, line in enumerate(text)
              for m in [re.match(r"^_Z\w*kalman_run_kILi(\d+)E\w*:", line)] if m]
    for i0, g in starts:
        i1 = next(i for i in range(i0, len(text)) if "s_endpgm" in text[i])
        body = text[i0:i1]
        labels = {m.group(1): i for i, line in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", line)] if m}
        loops = []  # backward branches: (start, end)
        for i, line in enumerate(body):
            m = re.match(r"^\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)", line)
            if m and labels.get(m.group(1), len(body)) <= i:
                loops.append((labels[m.group(1)], i))
        if not loops:
            continue
        step = max(loops, key=lambda ab: ab[1] - ab[0])
        inner = [ab for ab in loops if ab != step and step[0] <= ab[0] and ab[1] <= step[1]]

        def is_inner(i):
            return any(a <= i <= b for a, b in inner)

        def valu(line):
            return bool(re.match(r"^\s+v_", line))

        rng = range(step[0], step[1] + 1)
        out[g] = {"step_loop": sum(valu(body[i]) for i in rng if not is_inner(i)),
                  "piece_loop": sum(valu(body[i]) for i in rng if is_inner(i)),
                  "ds_bpermute": sum("ds_bpermute" in body[i] for i in rng if not is_inner(i)),
                  "lines": sum(bool(re.match(r"^\s+[a-z]", body[i])) for i in rng)}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cases", type=str, default="8:1048576,24:262144", help="n:M pairs")
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-points", type=int, default=16384)
    ap.add_argument("--no-static", action="store_true", help="skip the disassembly count")
    a = ap.parse_args()

    import numpy as np
    import torch
    from shyft_amd import _native, api, region

    assert torch.cuda.is_available(), "kalman_bench needs a GPU"
    torch.cuda.set_device(0)
    T = a.steps
    out = {"bench": "kalman_bench", "lib_sha256": _native.lib_sha(), "steps": T, "warmup": a.warmup, "reps": a.reps,
           "wave_instructions_per_s": WAVE_INSTRUCTIONS_PER_S, "cases": []}
    static = {} if a.no_static else static_valu()
    out["static_valu"] = {str(g): v for g, v in sorted(static.items())}
    t0 = api.Calendar().time(2016, 1, 1)

    def inputs(n, M, seed=1):
        rng = np.random.default_rng(seed)
        f = api.KalmanFilter(api.KalmanParameter(n_daily_observations=n))
        s0 = f.create_initial_state()
        t = f._tables(api.TimeAxis(t0, 3 * 3600 if n <= 8 else 86400 // n, T), True)
        bias = rng.normal(2.0, 1.0, (T, M))
        bias[rng.random((T, M)) < 0.1] = np.nan
        P = np.repeat(np.asarray(s0.P).reshape(n * n, 1), M, axis=1)
        return t, np.asarray(s0.W)[0, :n // 2 + 1].copy(), bias, np.zeros((n, M)), np.zeros((n, M)), P

    for case in a.cases.split(","):
        n, M = (int(v) for v in case.split(":"))
        t, w, bias, x, k, P = inputs(n, M)
        g = 1
        while g < n:
            g *= 2
        waves = -(-M * g // 256) * 4
        for mode in ("update", "running_bias"):
            running = (t["save_every"], t["piece_begin"], t["piece_ix"], t["piece_seconds"]) if mode != "update" else None
            ms, wall = [], []
            for i in range(a.warmup + a.reps):
                print(f"kalman_bench: n={n} M={M} {mode} call {i}", file=sys.stderr, flush=True)
                c0 = time.perf_counter()
                region.kalman_run(bias, t["fold"], w, t["v2"], x, k, P, running=running)
                c1 = time.perf_counter()
                if i >= a.warmup:
                    ms.append(region.kalman_last_ms())
                    wall.append((c1 - c0) * 1e3)
            best = min(ms)
            row = {"n": n, "lanes_per_point": g, "points": M, "mode": mode, "kernel_ms": best, "kernel_all_ms": ms,
                   "point_steps_per_s": M * T / (best * 1e-3), "copy_ms": min(wl - m for wl, m in zip(wall, ms)),
                   "pieces_per_step": float(len(t["piece_ix"])) / T}
            if g in static:
                valu = static[g]["step_loop"] + (static[g]["piece_loop"] * row["pieces_per_step"] if running else 0)
                row["static_valu_per_step"] = valu
                row["valu_issue_floor_ms"] = valu * T * waves / WAVE_INSTRUCTIONS_PER_S * 1e3
                row["kernel_over_floor"] = best / row["valu_issue_floor_ms"]
            out["cases"].append(row)
        del bias, P

    Mh = a.host_points
    t, w, bias, x, k, P = inputs(8, Mh)
    c0 = time.perf_counter()
    region.kalman_run(bias, t["fold"], w, t["v2"], x, k, P, host=True)
    dt = time.perf_counter() - c0
    out["host_restatement"] = {"n": 8, "points": Mh, "seconds": dt, "point_steps_per_s": Mh * T / dt, "threads": 1}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
