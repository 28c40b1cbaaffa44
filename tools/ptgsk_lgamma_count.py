#!/usr/bin/env python3
"""Where pt_gs_k's dlgamma evaluations arise, counted on the CPU oracle (the lgamma queue).

Runs the oracle over the bench year in the bench's chunks (20 x 438 steps, state carried, the lgamma cache and the
carry cold at each chunk's first step, as in a launch) on the first cells of the synthetic 1M-cell region and replays
the kernel's lgamma cache on the state series (tests/test_ptgsk_lgamma_queue.lgamma_events). Prints, per season, the
share of lane-steps with a new evaluation by where it arises, and the workgroup-step (256 lanes) tallies.

usage: ptgsk_lgamma_count.py [--cells 2048] [--chunks 20] [--steps 438]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from shyft_amd import synthetic  # noqa: E402
from tests import oracle_lib  # noqa: E402
from tests.test_ptgsk_lgamma_queue import lgamma_events  # noqa: E402

SEASONS = {"winter": (12, 1, 2), "spring": (3, 4, 5), "summer": (6, 7, 8), "autumn": (9, 10, 11)}
MONTH_START_DAY = np.cumsum([0, 31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30])


def month_of_hour(h):
    return int(np.searchsorted(MONTH_START_DAY, (h // 24) % 365, side="right"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=2048)
    ap.add_argument("--chunks", type=int, default=20)
    ap.add_argument("--steps", type=int, default=438)
    a = ap.parse_args()
    n, K = a.cells, a.steps
    geo = synthetic.geo11(n, n_total=1 << 20)
    p = synthetic.default_ptgsk_parameters()
    state = synthetic.default_ptgsk_state(n)
    keys = ("lane_steps", "front", "job", "job_new", "back", "melt", "reset_shape", "cold", "again", "uses",
            "wg_steps", "wg_back", "wg_back_brent", "wg_back_nobrent", "wg_over64", "back_in_nobrent")
    acc = {s: dict.fromkeys(keys, 0) for s in list(SEASONS) + ["year"]}
    hist = {s: [] for s in acc}
    for c in range(a.chunks):
        h0 = c * K
        f = synthetic.forcing(n, h0, K)
        o = oracle_lib.ptgsk_run(geo, p, state, synthetic.T0_2015_US + h0 * synthetic.HOUR_US, synthetic.HOUR_US, f,
                                 collect_state=True)
        state = o["state"]
        ev = lgamma_events(o["state_series"], f[0], f[1], p, hour0=h0)
        m = month_of_hour(h0 + K // 2)
        season = next(s for s, ms in SEASONS.items() if m in ms)
        nb, nj = ev["n_back"], ev["n_job"]
        for s in (season, "year"):
            d = acc[s]
            d["lane_steps"] += K * n
            for k in ("front", "job", "job_new", "back", "melt", "reset_shape", "cold", "again", "uses"):
                d[k] += int(ev[k].sum())
            d["wg_steps"] += nb.size
            d["wg_back"] += int((nb > 0).sum())
            d["wg_back_brent"] += int(((nb > 0) & (nj > 0)).sum())
            d["wg_back_nobrent"] += int(((nb > 0) & (nj == 0)).sum())
            d["wg_over64"] += int((nb > 64).sum())
            d["back_in_nobrent"] += int(nb[nj == 0].sum())
            hist[s].append(nb[nb > 0])
        print(f"chunk {c:2d} (month {m:2d}): back {ev['back'].mean():.4f} job {ev['job'].mean():.4f} "
              f"front {ev['front'].mean():.5f} of lane-steps", flush=True)
    print("\nshare of lane-steps with a new dlgamma, by where it arises; `back` = gs_back's final calc_snow_state "
          "(the queue's shapes), split by what made the shape new")
    print("season | job lanes | job lgamma(a2) new | front | back | = snowfall only | melt update | reset value | "
          "cold cache | back per using lane")
    for s, d in acc.items():
        L = d["lane_steps"]
        snow_only = d["back"] - d["melt"] - d["reset_shape"] - d["cold"]
        print(f"{s:6s} | {d['job'] / L:.4f} | {d['job_new'] / L:.4f} | {d['front'] / L:.5f} | {d['back'] / L:.4f} | "
              f"{snow_only / L:.4f} | {d['melt'] / L:.4f} | {d['reset_shape'] / L:.5f} | {d['cold'] / L:.5f} | "
              f"{d['back'] / max(1, d['uses']):.3f}")
    print("\nworkgroup-steps (256 lanes)")
    print("season | with new shapes | of those with a Brent job | without | > 64 shapes | shapes in no-Brent steps / "
          "all shapes | shapes per such step: mean, median, p90")
    for s, d in acc.items():
        h = np.concatenate(hist[s]) if hist[s] else np.zeros(1)
        if h.size == 0:
            h = np.zeros(1)
        print(f"{s:6s} | {d['wg_back'] / d['wg_steps']:.3f} | {d['wg_back_brent'] / max(1, d['wg_back']):.3f} | "
              f"{d['wg_back_nobrent'] / max(1, d['wg_back']):.3f} | {d['wg_over64'] / max(1, d['wg_back']):.3f} | "
              f"{d['back_in_nobrent'] / max(1, d['back']):.3f} | {h.mean():.1f}, {np.median(h):.0f}, "
              f"{np.percentile(h, 90):.0f}")


if __name__ == "__main__":
    main()
