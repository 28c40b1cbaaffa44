#!/usr/bin/env python3
"""What opening the Brent search on the solving wavefront's idle lanes can save, counted on the CPU oracle
(gs_brent_job_open, device/gs_brent.h).

Runs the oracle over the bench year in the bench's chunks (20 x 438 steps, state carried) on the first cells of the
synthetic 1M-cell region, takes the corr_lwc jobs of every step from the state series (the replay of
tests/test_ptgsk_lgamma_queue.lgamma_events) and solves each job with a Python restatement of brent_find_minima whose
f is built from the oracle's own incomplete gamma (oracle_gamma_pq_policy), counting f evaluations and comparing the
second and third evaluation points with gs_brent_point's, bit for bit. The restatement's result is compared with
oracle_gs_corr_lwc on every job.

A pass is one f evaluation issued by the solving wavefront for up to 64 jobs at once, so a workgroup-step with
nj <= 64 jobs costs max(evaluations per job) passes. With L lanes per job (4 with nj <= 16, 2 with nj <= 32) a job
whose points were predicted needs 2 (1) passes fewer. Prints and writes, per season: the histogram of jobs per
256-lane workgroup-step, evaluations per job, the share of predicted points, and passes saved over passes issued.

usage: ptgsk_brent_opening_count.py [--cells 2048] [--chunks 20] [--steps 438] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from shyft_amd import synthetic  # noqa: E402
from tests import oracle_lib  # noqa: E402
from tests.test_ptgsk_lgamma_queue import lgamma_events, SSF  # noqa: E402

SEASONS = {"winter": (12, 1, 2), "spring": (3, 4, 5), "summer": (6, 7, 8), "autumn": (9, 10, 11)}
MONTH_START_DAY = np.cumsum([0, 31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30])
CLASSES = (("0", 0, 0), ("1-16", 1, 16), ("17-32", 17, 32), ("33-64", 33, 64), (">64", 65, 1 << 30))
BLOCK = 256
TOL = 2.0 ** -11
GOLDEN = float(np.float32(0.3819660))
BRENT_SHARE = 0.6   # of wavefront time in the October-April chunks (tools/ptgsk_phases.py)


def month_of_hour(h):
    return int(np.searchsorted(MONTH_START_DAY, (h // 24) % 365, side="right"))


def brent_point(z1, k):
    """gs_brent_point (device/gs_brent.h)."""
    def golden_step(x, lo, hi):
        mid = (lo + hi) / 2
        fract1 = TOL * abs(x) + TOL / 4
        d2 = lo - x if x >= mid else hi - x
        delta = GOLDEN * d2
        if abs(delta) >= fract1:
            return x + delta
        return x + abs(fract1) if delta > 0 else x - abs(fract1)
    if k == 0:
        return z1
    u1 = golden_step(z1, 0.0, z1)
    if k == 1:
        return u1
    lo, hi, x = 0.0, z1, z1
    if k == 2:
        if u1 >= x:
            lo = x
        else:
            hi = x
        x = u1
    else:
        if u1 < x:
            lo = u1
        else:
            hi = u1
    return golden_step(x, lo, hi)


def brent(f, z1):
    """boost brent_find_minima over [0, z1], 12 bits, 60 iterations, as gs_corr_lwc (device/ptgsk_dev.h) states it.
    -> (x, the points evaluated in order)."""
    pts = []

    def fe(z):
        pts.append(z)
        return f(z)
    lo, hi = 0.0, z1
    x = w = v = hi
    fw = fv = fx = fe(x)
    delta2 = delta = 0.0
    for _ in range(60):
        mid = (lo + hi) / 2
        fract1 = TOL * abs(x) + TOL / 4
        fract2 = 2 * fract1
        if abs(x - mid) <= (fract2 - (hi - lo) / 2):
            break
        golden = True
        if abs(delta2) > fract1:
            r = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * r
            q = 2 * (q - r)
            if q > 0:
                p = -p
            q = abs(q)
            td = delta2
            delta2 = delta
            if not ((abs(p) >= abs(q * td / 2)) or (p <= q * (lo - x)) or (p >= q * (hi - x))):
                golden = False
                delta = p / q
                u = x + delta
                if (u - lo) < fract2 or (hi - u) < fract2:
                    delta = -abs(fract1) if (mid - x) < 0 else abs(fract1)
        if golden:
            delta2 = lo - x if x >= mid else hi - x
            delta = GOLDEN * delta2
        u = x + delta if abs(delta) >= fract1 else (x + abs(fract1) if delta > 0 else x - abs(fract1))
        fu = fe(u)
        if fu <= fx:
            if u >= x:
                lo = x
            else:
                hi = x
            v, w, x = w, x, u
            fv, fw, fx = fw, fx, fu
        else:
            if u < x:
                lo = u
            else:
                hi = u
            if fu <= fw or w == x:
                v, w, fv, fw = w, u, fw, fu
            elif fu <= fv or v == x or v == w:
                v, fv = u, fu
    return x, pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=2048)
    ap.add_argument("--chunks", type=int, default=20)
    ap.add_argument("--steps", type=int, default=438)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, K = a.cells, a.steps
    lib = oracle_lib.load("detmath")
    d = C.c_double
    lib.oracle_gamma_pq_policy.restype = None
    lib.oracle_gamma_pq_policy.argtypes = [d, d, C.POINTER(d), C.POINTER(d), C.POINTER(d)]
    gp, gp1, gpre = d(), d(), d()

    def calc_q(sa, sb, z):
        lib.oracle_gamma_pq_policy(sa, z / sb, C.byref(gp), C.byref(gp1), C.byref(gpre))
        return sa * sb * gp1.value + z * (1.0 - gp.value)

    geo = synthetic.geo11(n, n_total=1 << 20)
    p = synthetic.default_ptgsk_parameters()
    state = synthetic.default_ptgsk_state(n)
    max_water, ibgf, p_corr, cv2 = p[6], p[21], p[16], p[14] * p[14]
    names = list(SEASONS) + ["year"]
    acc = {s: {"wg_steps": {c[0]: 0 for c in CLASSES}, "jobs": 0, "f_evals": 0, "second_point_predicted": 0,
               "second_point_evaluated": 0, "third_point_predicted": 0, "third_point_evaluated": 0,
               "same_as_oracle_corr_lwc": 0, "passes_issued": 0, "passes_saved_L4": 0, "passes_saved_L4_L2": 0,
               "passes_issued_by_class": {c[0]: 0 for c in CLASSES}} for s in names}
    for c in range(a.chunks):
        h0 = c * K
        f = synthetic.forcing(n, h0, K)
        o = oracle_lib.ptgsk_run(geo, p, state, synthetic.T0_2015_US + h0 * synthetic.HOUR_US, synthetic.HOUR_US, f,
                                 collect_state=True)
        state = o["state"]
        ss = o["state_series"]
        ev = lgamma_events(ss, f[0], f[1], p, hour0=h0)
        m = month_of_hour(h0 + K // 2)
        season = next(s for s, ms in SEASONS.items() if m in ms)
        nwg = (n + BLOCK - 1) // BLOCK
        for i in range(K):
            job = ev["job"][i]
            for g in range(nwg):
                cells = np.flatnonzero(job[g * BLOCK:(g + 1) * BLOCK]) + g * BLOCK
                nj = cells.size
                cls = next(k for k, lo, hi in CLASSES if lo <= nj <= hi)
                for s in (season, "year"):
                    acc[s]["wg_steps"][cls] += 1
                if nj == 0:
                    continue
                nf, h1, h2 = [], [], []
                for cell in cells.tolist():
                    alpha, smm = float(ss[4, i, cell]), float(ss[5, i, cell])
                    lwc = float(ss[2, i, cell]) / SSF
                    prec = (float(f[1][i, cell]) * p_corr * 3600000000.0) / 3600000000.0
                    sdc_snow = prec / (1.0 - ibgf)
                    a2 = (smm * alpha + sdc_snow / cv2) / (sdc_snow + smm)
                    b2 = (smm + sdc_snow) / a2
                    b1 = smm / alpha if smm / alpha > 0.0 else b2
                    z1 = lwc / max_water
                    Q1 = calc_q(alpha, b1, z1)
                    x, pts = brent(lambda z: (calc_q(a2, b2, z) - Q1) ** 2, z1)
                    same = x == lib.oracle_gs_corr_lwc(z1, alpha, b1, 0.0, a2, b2)
                    e1 = len(pts) > 1
                    e2 = len(pts) > 2
                    hit1 = e1 and pts[1] == brent_point(z1, 1)
                    hit2 = e2 and pts[2] in (brent_point(z1, 2), brent_point(z1, 3))
                    nf.append(len(pts))
                    h1.append(hit1)
                    h2.append(hit1 and hit2)
                    for s in (season, "year"):
                        d_ = acc[s]
                        d_["jobs"] += 1
                        d_["f_evals"] += len(pts)
                        d_["second_point_evaluated"] += e1
                        d_["second_point_predicted"] += hit1
                        d_["third_point_evaluated"] += e2
                        d_["third_point_predicted"] += bool(hit2)
                        d_["same_as_oracle_corr_lwc"] += bool(same)
                nf, h1, h2 = np.array(nf), np.array(h1), np.array(h2)
                # passes: the jobs of a wavefront (64 in queue order; here cell order) advance together
                issued = sum(int(nf[k:k + 64].max()) for k in range(0, nj, 64))
                l4 = int((nf - h1 - h2).max()) if nj <= 16 else issued
                l42 = l4 if nj <= 16 else int((nf - h1).max()) if nj <= 32 else issued
                for s in (season, "year"):
                    d_ = acc[s]
                    d_["passes_issued"] += issued
                    d_["passes_issued_by_class"][cls] += issued
                    d_["passes_saved_L4"] += issued - l4
                    d_["passes_saved_L4_L2"] += issued - l42
        print(f"chunk {c:2d} (month {m:2d}) done: {acc['year']['jobs']} jobs so far", flush=True)
    for s, d_ in acc.items():
        j = max(1, d_["jobs"])
        pi = max(1, d_["passes_issued"])
        d_["f_evals_per_job"] = d_["f_evals"] / j
        d_["second_point_predicted_share"] = d_["second_point_predicted"] / max(1, d_["second_point_evaluated"])
        d_["third_point_predicted_share"] = d_["third_point_predicted"] / max(1, d_["third_point_evaluated"])
        d_["passes_saved_share_L4"] = d_["passes_saved_L4"] / pi
        d_["passes_saved_share_L4_L2"] = d_["passes_saved_L4_L2"] / pi
        d_["predicted_kernel_time_saved_L4"] = BRENT_SHARE * d_["passes_saved_share_L4"]
        d_["predicted_kernel_time_saved_L4_L2"] = BRENT_SHARE * d_["passes_saved_share_L4_L2"]
        print(f"{s:6s} wg-steps {d_['wg_steps']}  jobs {d_['jobs']}  f/job {d_['f_evals_per_job']:.2f}  predicted 2nd "
              f"{d_['second_point_predicted_share']:.4f} 3rd {d_['third_point_predicted_share']:.4f}  passes "
              f"{d_['passes_issued']} saved L4 {d_['passes_saved_share_L4']:.4f} L4+L2 "
              f"{d_['passes_saved_share_L4_L2']:.4f}  oracle-equal {d_['same_as_oracle_corr_lwc'] / j:.4f}")
    out = {"cells": n, "chunks": a.chunks, "steps": K, "brent_share_assumed": BRENT_SHARE, "seasons": acc}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1, default=lambda v: v.item())


if __name__ == "__main__":
    main()
