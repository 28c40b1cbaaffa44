"""The exit handling of the lean incomplete gamma's two term loops (device/gamma_lean.h), bit for bit.

The series and the continued fraction of gsb_gamma_pq are loops that every lane of a wavefront leaves at its own
term. With SHYFT_GAMMA_LOOPS (the default) they are hand-written: the term's compare writes the exec mask, a lane
that has met its tolerance stops executing and keeps the values of the term it left at, two terms per trip, the
fraction's two convergents changing roles from term to term (so the registers a lane's result is in depend on the
parity of its term count), and a wave-uniform 2,000-term cap. What can go wrong there is a lane that stops a term
early or late, takes its result from the wrong registers, runs on after its neighbours have left, or takes part in
a loop it should not be in. The cases are the smallest that hold each of those:
  - a wavefront whose 64 lanes leave the series at the terms 1, 2, ..., 64 (shape >= 2: the 2^-18 policy), and one
    that spreads over the terms the 2^-35 policy (shape < 2) can reach;
  - a wavefront of alternating series and fraction lanes, with odd and even fraction term counts;
  - lanes that leave at term 1 of the series and of the fraction, under both policies;
  - one active lane (all others outside the fast domain, which take no loop at all), and lanes 0 and 63 only;
  - a lane whose E sends it to the general evaluation between neighbours that stay on the fast path (the fraction's
    check of its largest |P| fires only in a lane that no longer converges, which is the cap's case, below);
  - lanes outside the fast domain (x <= 0, subnormal, |exp argument| > 708, inf, NaN) between lanes inside it.
The term counts are worked out on the CPU by a restatement of the loops (exact fma), and the module asserts that the
cases hold them before any GPU result is read. The device side is shyft_hip_device_selftest: GAMMA_LEAN (p, p1 and
the prefix of gs_gamma_pq_cs and gsb_gamma_pq's own verdict) against the oracle's general evaluation, and BRENT,
BRENT_OPEN4 and BRENT_OPEN2 (the lean job and the job entry on 4 and 2 lanes per job) against gs_corr_lwc and the
oracle's corr_lwc.

The 2,000-term cap is not run on the GPU. The CPU tests restate the control of the hand-written loops -- exec mask,
two terms per trip, the trip counter of the series, the fraction's compare of its own term count, the parity
select -- on a wavefront of lanes, and check it against the plain per-lane loops, a lane that never converges
(eps = 0) included."""
import ctypes as C
import functools
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import oracle_lib
from tests.test_device_functions import BRENT, BRENT_EDGE, GAMMA_LEAN, GOLDEN, _assert_bits, _device

BRENT_OPEN4, BRENT_OPEN2 = 11, 12   # function codes of include/shyft_hip.h
SCALE_HI = 1.0e200                  # detmath::GPQ_SCALE_HI
CAP = 2000
MIN_NORMAL, MAX_DOUBLE = 2.2250738585072014e-308, 1.7976931348623157e308
OUTSIDE = -1.0                      # an x outside the fast domain: the lane takes no loop


def policy_eps(a):
    return 2.0 ** -35 if a < 2.0 else 2.0 ** -18   # detmath::gamma_snow_policy_eps


def fma(a, b, c):
    """a * b + c rounded once."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    try:
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    except OverflowError:
        return math.copysign(math.inf, a * b + c)


# ------------------------------------------------------------------------------------------------ the plain loops
def series_term(a, x, st):
    ap, E, B, xn = st
    ap = ap + 1.0
    xn = xn * x
    E = E * ap
    B = fma(B, ap, xn)
    return (ap, E, B, xn)


def series(a, x, eps, exact=True):
    """gsb_gamma_pq's series as written: (terms, E, B); terms == CAP + 1: it ran into the cap."""
    st = (a, 1.0, 0.0, 1.0)
    for n in range(1, CAP + 1):
        if exact:
            st = series_term(a, x, st)
        else:   # (for scanning: the product and the sum rounded apart)
            ap, E, B, xn = st
            ap, xn = ap + 1.0, xn * x
            st = (ap, E * ap, B * ap + xn, xn)
        if st[3] < eps * (st[2] + st[1]):
            return n, st[1], st[2]
    return CAP + 1, st[1], st[2]


def fraction_term(a, st):
    """one term on (Pm, P, Qm, Qd, di, bcf) -> the new state and whether the lane goes on."""
    Pm, P, Qm, Qd, di, bcf, eps = st
    di = di + 1.0
    an = -di * (di - a)
    bcf = bcf + 2.0
    Pn = fma(bcf, P, an * Pm)
    Qn = fma(bcf, Qd, an * Qm)
    cross = Pn * Qd
    diff = cross - P * Qn
    return (P, Pn, Qd, Qn, di, bcf, eps), not (abs(diff) <= eps * abs(cross))


def fraction(a, x, eps):
    """gsb_gamma_pq's continued fraction as written: (terms, P, Qd, bigP)."""
    st = (1.0, x + 1.0 - a, 0.0, 1.0, 0.0, x + 1.0 - a, eps)
    bigP = 0.0
    for i in range(1, CAP + 1):
        st, on = fraction_term(a, st)
        if not on:
            return i, st[1], st[3], bigP
        if abs(st[1]) > bigP:   # fmax: a NaN P leaves bigP
            bigP = abs(st[1])
    return CAP + 1, st[1], st[3], bigP


# --------------------------------------------------------------------- the control of the hand-written loops, restated
def wave_series(lanes):
    """lanes: [(a, x, eps)] or None (not in the loop) -> [(terms, E, B)] by the loop of gsb_series_loop: exec, two
    terms per trip, a counter of trips from 999 that leaves at the borrow."""
    st = {k: (v[0], 1.0, 0.0, 1.0) for k, v in enumerate(lanes) if v is not None}
    terms = dict.fromkeys(st, 0)
    live = set(st)

    def term():
        for k in sorted(live):
            a, x, eps = lanes[k]
            st[k] = series_term(a, x, st[k])
            terms[k] += 1
            if st[k][3] < eps * (st[k][2] + st[k][1]):   # v_cmpx_nlt: the lane leaves exec
                live.discard(k)
    trips = 999
    while True:
        term()
        if not live:
            break
        term()
        trips -= 1
        if trips < 0:   # s_sub_u32 borrows: the cap
            break
        if not live:
            break
    return [None if v is None else (terms[k], st[k][1], st[k][2]) for k, v in enumerate(lanes)]


def wave_fraction(lanes):
    """lanes: [(a, x, eps)] or None -> [(terms, P, Qd, bigP)] by the loop of gsb_cf_loop: the two convergents in
    (pa, qa) and (pb, qb) changing roles, bigP only in the lanes that go on, the cap a compare of the term count,
    the result taken by the parity of the lane's own count."""
    reg = {k: {"pa": 1.0, "pb": v[1] + 1.0 - v[0], "qa": 0.0, "qb": 1.0, "di": 0.0, "bcf": v[1] + 1.0 - v[0],
               "big": 0.0} for k, v in enumerate(lanes) if v is not None}
    live = set(reg)

    def term(pm, p, qm, qd):
        for k in sorted(live):
            r = reg[k]
            a, _, eps = lanes[k]
            (_, Pn, _, Qn, di, bcf, _), on = fraction_term(a, (r[pm], r[p], r[qm], r[qd], r["di"], r["bcf"], eps))
            r[pm], r[qm], r["di"], r["bcf"] = Pn, Qn, di, bcf   # the new convergent over the previous one
            if not on:
                live.discard(k)
    while True:
        term("pa", "pb", "qa", "qb")
        if not live:
            break
        for k in live:
            if abs(reg[k]["pa"]) > reg[k]["big"]:
                reg[k]["big"] = abs(reg[k]["pa"])
        term("pb", "pa", "qb", "qa")
        for k in live:
            if abs(reg[k]["pb"]) > reg[k]["big"]:
                reg[k]["big"] = abs(reg[k]["pb"])
        for k in sorted(live):   # v_cmpx_gt 2000.0, di
            if not 2000.0 > reg[k]["di"]:
                live.discard(k)
        if not live:
            break
    out = []
    for k, v in enumerate(lanes):
        if v is None:
            out.append(None)
            continue
        r = reg[k]
        odd = int(r["di"]) & 1
        out.append((int(r["di"]), r["pa"] if odd else r["pb"], r["qa"] if odd else r["qb"], r["big"]))
    return out


# ------------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def dm():
    L = oracle_lib.load("detmath")
    d = C.c_double
    L.oracle_gamma_pq_policy.restype = None
    L.oracle_gamma_pq_policy.argtypes = [d, d, C.POINTER(d), C.POINTER(d), C.POINTER(d)]
    L.oracle_gamma_pq_rescaled.restype = C.c_int
    L.oracle_gamma_pq_rescaled.argtypes = [d, d, d]
    for f in (L.oracle_log, L.oracle_lgamma_fn):
        f.restype = d
        f.argtypes = [d]
    L.oracle_gs_corr_lwc.restype = d
    L.oracle_gs_corr_lwc.argtypes = [d] * 6
    return L


def lean(a, x):
    """What gsb_gamma_pq does with (a, x): kind 'none' (outside the fast domain: no loop), 'series' or 'fraction';
    the lane's term count; ok, its verdict."""
    inside = a > 0.0 and MIN_NORMAL <= x <= MAX_DOUBLE
    if inside:
        arg = a * dm().oracle_log(x) - x - dm().oracle_lgamma_fn(a)
        inside = abs(arg) <= 708.0
    if not inside:
        return {"kind": "none", "terms": 0, "ok": False}
    eps = policy_eps(a)
    if x < a + 1.0:
        n, E, _ = series(a, x, eps)
        return {"kind": "series", "terms": n, "ok": E <= SCALE_HI}
    n, _, _, bigP = fraction(a, x, eps)
    return {"kind": "fraction", "terms": n, "ok": not bigP > SCALE_HI}


def ladder(shapes, want):
    """k -> (a, x) at which the series leaves at term k inside the fast domain, for the k of `want` that the shapes
    reach: x from the middle of the range with that count (found with the product and the sum rounded apart,
    confirmed with the exact fma). A small count needs a small x, which only a small shape keeps inside
    |a log x - x - lgamma a| <= 708; a large count needs a large shape."""
    out = {}
    for a in shapes:
        eps = policy_eps(a)
        xs = (a + 1.0) * np.concatenate([np.geomspace(1e-12, 0.3, 2500), np.linspace(0.3, 0.99999, 2500)[1:]])
        n = np.array([series(a, float(x), eps, exact=False)[0] for x in xs])
        for k in want:
            at = np.flatnonzero(n == k)
            if k in out or not at.size:
                continue
            x = float(xs[at[at.size // 2]])
            v = lean(a, x)
            if v["kind"] == "series" and v["terms"] == k and v["ok"]:
                out[k] = (a, x)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> the 64 (a, x) of one wavefront."""
    w = {}
    hi = ladder((2.5, 6.25, 30.0, 170.0, 300.0), range(1, 65))
    assert sorted(hi) == list(range(1, 65)), sorted(set(range(1, 65)) - set(hi))
    w["series terms 1..64, shape >= 2"] = [hi[k] for k in range(1, 65)]
    lo = ladder((0.5, 1.5, 1.999), range(1, 65))
    assert 1 in lo and len(lo) >= 16, sorted(lo)
    ks = sorted(lo)
    w["series terms spread, shape < 2"] = [lo[ks[(7 * i) % len(ks)]] for i in range(64)]
    # series and fraction lanes side by side; the fraction's x from 1.02 to 12 times a + 1: odd and even counts
    mixed = []
    for i in range(64):
        a = (0.5, 1.26, 6.25, 30.0)[(i // 2) % 4]
        mixed.append((a, (a + 1.0) * (0.03 + 0.015 * i)) if i % 2 == 0 else (a, (a + 1.0) * (1.02 + 0.17 * i)))
    w["series and fraction lanes alternate"] = mixed
    # term 1 of each loop under both policies: x tiny (series); a = 1 makes the first partial numerator 0, and
    # a = 2 with x = 600 meets 2^-18 at once (fraction)
    first = [(6.25, 1e-9), (1.5, 1e-14), (2.0, 600.0), (1.0, 5.0)]
    w["term 1 of both loops between longer lanes"] = [first[i // 8 % 4] if i % 8 == 0 else mixed[i] for i in range(64)]
    for name, on in (("one lane, series", {17: (6.25, 3.0)}), ("one lane, fraction", {40: (6.25, 9.0)}),
                     ("lanes 0 and 63, series", {0: hi[64], 63: (6.25, 3.0)}),
                     ("lanes 0 and 63, series and fraction", {0: (30.0, 50.0), 63: (1.26, 0.4)})):
        w[name] = [on.get(i, (6.25, OUTSIDE)) for i in range(64)]
    # E > 1e200: the general evaluation, the neighbours stay. (A fraction lane whose largest |P| passes 1e200 is not
    # here: its P Qd has overflowed by then, the difference is a NaN and the lane runs to the cap.)
    general = {5: (1000.0, 0.9 * 1001.0), 6: (1500.0, 0.9 * 1501.0), 62: (1000.0, 0.9 * 1001.0), 63: (1500.0, 0.9 * 1501.0)}
    w["general-path lanes between fast ones"] = [general.get(i, mixed[i]) for i in range(64)]
    out = [0.0, -1.0, 5e-324, 1e-310, 800.0, math.inf, math.nan]
    w["lanes outside the fast domain between lanes inside"] = \
        [(6.25, out[(i // 3) % len(out)]) if i % 3 == 0 else ((300.0, 1e-3) if i % 3 == 1 and i % 2 else mixed[i])
         for i in range(64)]
    assert all(len(v) == 64 for v in w.values())
    return w


@functools.lru_cache(maxsize=None)
def expected():
    """name -> [lean(a, x)] of the wavefront's lanes, asserted to be what the case's name says."""
    e = {name: [lean(a, x) for a, x in lanes] for name, lanes in cases().items()}

    def count(name, kind):
        return [v["terms"] for v in e[name] if v["kind"] == kind]
    assert count("series terms 1..64, shape >= 2", "series") == list(range(1, 65))
    assert all(v["ok"] for v in e["series terms 1..64, shape >= 2"])
    n = count("series terms spread, shape < 2", "series")
    assert len(n) == 64 and min(n) == 1 and len(set(n)) >= 16, sorted(set(n))
    m = e["series and fraction lanes alternate"]
    assert [v["kind"] for v in m] == ["series", "fraction"] * 32 and all(v["ok"] for v in m)
    f = count("series and fraction lanes alternate", "fraction")
    assert any(k % 2 for k in f) and any(k % 2 == 0 for k in f) and len(set(f)) >= 8, f
    t1 = e["term 1 of both loops between longer lanes"]
    assert [(t1[i]["kind"], t1[i]["terms"]) for i in (0, 8, 16, 24)] == \
        [("series", 1), ("series", 1), ("fraction", 1), ("fraction", 1)]
    assert max(v["terms"] for v in t1) >= 8
    for name, kinds in (("one lane, series", {17: "series"}), ("one lane, fraction", {40: "fraction"}),
                        ("lanes 0 and 63, series", {0: "series", 63: "series"}),
                        ("lanes 0 and 63, series and fraction", {0: "fraction", 63: "series"})):
        assert {i: v["kind"] for i, v in enumerate(e[name]) if v["kind"] != "none"} == kinds, name
        assert all(v["ok"] for v in e[name] if v["kind"] != "none")
    g = e["general-path lanes between fast ones"]
    assert [(g[i]["kind"], g[i]["ok"]) for i in (5, 6, 62, 63)] == [("series", False)] * 4
    assert all(v["ok"] for i, v in enumerate(g) if i not in (5, 6, 62, 63))
    o = e["lanes outside the fast domain between lanes inside"]
    assert max(v["terms"] for v in sum(e.values(), [])) < 200   # nothing here runs into the cap
    assert sum(v["kind"] == "none" for v in o) >= 30 and sum(v["kind"] == "series" for v in o) >= 5 and \
        sum(v["kind"] == "fraction" for v in o) >= 5
    # ok is exactly "inside the fast domain and the general evaluation does not rescale"
    for name, lanes in cases().items():
        for (a, x), v in zip(lanes, e[name]):
            if v["kind"] != "none":
                assert v["ok"] == (dm().oracle_gamma_pq_rescaled(a, x, policy_eps(a)) == 0), (name, a, x)
    return e


# ------------------------------------------------------------------------------------------------ CPU tests
def test_cases_hold_their_term_counts():
    expected()


def _wave_lanes(kind):
    """every case's lanes of one kind as (a, x, eps), the others None."""
    for name, lanes in cases().items():
        yield name, [(a, x, policy_eps(a)) if v["kind"] == kind else None
                     for (a, x), v in zip(lanes, expected()[name])]


def test_restated_series_control_equals_the_plain_loop():
    for name, lanes in _wave_lanes("series"):
        got = wave_series(lanes)
        for v, g in zip(lanes, got):
            if v is not None:
                assert g == series(*v), (name, v)


def test_restated_fraction_control_equals_the_plain_loop():
    for name, lanes in _wave_lanes("fraction"):
        got = wave_fraction(lanes)
        for v, g in zip(lanes, got):
            if v is not None:
                n, P, Qd, bigP = fraction(*v)
                assert g == (n, P, Qd, bigP), (name, v)


def test_cap_ends_both_loops_after_2000_terms():
    """eps = 0 never converges. The plain loops make 2,000 terms; so does the restated control, with the values of
    term 2,000, while the lane beside it leaves at its own term."""
    n, E, B = series(6.25, 3.0, 0.0)
    assert n == CAP + 1
    got = wave_series([(6.25, 3.0, 0.0), (6.25, 3.0, 2.0 ** -18), None])
    assert got[0][0] == CAP and (got[0][1] == E or (math.isnan(E) and math.isnan(got[0][1]))) and got[2] is None
    assert got[0][2] == B or (math.isnan(B) and math.isnan(got[0][2]))
    assert got[1] == series(6.25, 3.0, 2.0 ** -18)
    n, P, Qd, bigP = fraction(6.25, 9.0, -1.0)   # |diff| <= -|cross| never holds
    assert n == CAP + 1
    got = wave_fraction([(6.25, 9.0, 2.0 ** -18), (6.25, 9.0, -1.0)])
    same = lambda u, v: u == v or (math.isnan(u) and math.isnan(v))
    assert got[1][0] == CAP and same(got[1][1], P) and same(got[1][2], Qd) and same(got[1][3], bigP)
    assert got[0] == fraction(6.25, 9.0, 2.0 ** -18)


# ------------------------------------------------------------------------------------------------ GPU tests
@functools.lru_cache(maxsize=None)
def _gamma_reference():
    names = list(cases())
    a = np.array([v[0] for n in names for v in cases()[n]])
    x = np.array([v[1] for n in names for v in cases()[n]])
    ok = np.array([float(v["ok"]) for n in names for v in expected()[n]])
    p, p1, pre = C.c_double(), C.c_double(), C.c_double()
    ref = np.empty((3, a.size))
    for i, (ai, xi) in enumerate(zip(a.tolist(), x.tolist())):
        dm().oracle_gamma_pq_policy(ai, xi, C.byref(p), C.byref(p1), C.byref(pre))
        ref[:, i] = p.value, p1.value, pre.value
    return names, a, x, ok, ref


@pytest.mark.gpu
def test_lean_gamma_wavefronts():
    """Every case is one wavefront of the test kernel (64 consecutive rows of a 256-lane workgroup)."""
    names, a, x, ok, ref = _gamma_reference()
    assert a.size == 64 * len(names)
    out = _device(GAMMA_LEAN, [a, x], 4)
    for w, name in enumerate(names):
        r = slice(64 * w, 64 * w + 64)
        _assert_bits(out[3][r], ok[r], f"{name}: gsb_gamma_pq's verdict", a[r], x[r])
        for k, nm in enumerate(("p", "p1", "prefix")):
            _assert_bits(out[k][r], ref[k][r], f"{name}: {nm}", a[r], x[r])


@pytest.mark.gpu
def test_lean_gamma_in_a_ragged_last_wavefront():
    """The ladder alone in a launch that ends inside a wavefront: 37 lanes, the others never start."""
    _, a, x, ok, ref = _gamma_reference()
    out = _device(GAMMA_LEAN, [a[:37], x[:37]], 4)
    _assert_bits(out[3], ok[:37], "verdict", a[:37], x[:37])
    for k, nm in enumerate(("p", "p1", "prefix")):
        _assert_bits(out[k], ref[k][:37], nm, a[:37], x[:37])


@functools.lru_cache(maxsize=None)
def _brent_jobs():
    """z1 a1 b1 a2 b2. Rows 0-63: recorded jobs in lanes 0 and 63, between them a job whose points all lie outside
    the fast domain (its f takes the general evaluation: no loop). Rows 64-127: recorded jobs with every eighth an
    edge job (series rescale inside f, |exp argument| > 708, both policies). Row 128: one job alone in its
    wavefront."""
    rec = np.load(os.path.join(GOLDEN, "brent_jobs_sample.npy"))
    edge = np.array(BRENT_EDGE)
    jobs = np.empty((129, 5))
    jobs[:64] = edge[2]
    jobs[0], jobs[63] = rec[0], rec[1]
    jobs[64:128] = rec[2:66]
    jobs[64:128:8] = edge[[0, 3, 4, 5, 0, 3, 4, 5]]
    jobs[128] = rec[66]
    return jobs


def test_brent_jobs_are_what_they_are_meant_to_be():
    jobs = _brent_jobs()
    z1, _, _, a2, b2 = jobs[5]
    assert all(lean(a2, z / b2)["kind"] == "none" for z in (z1, 0.618 * z1, 0.382 * z1))
    kinds = {lean(a2, z1 * m / b2)["kind"] for z1, _, _, a2, b2 in jobs[64:128].tolist() for m in (1.0, 0.618, 0.382, 0.1)}
    assert {"series", "fraction"} <= kinds, kinds


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_brent_jobs_through_the_lean_loops(mode):
    jobs = _brent_jobs()
    cols = [np.ascontiguousarray(jobs[:, k]) for k in range(5)] + [np.full(len(jobs), float(mode))]
    ref = np.array([dm().oracle_gs_corr_lwc(z1, a1, b1, 0.0, a2, b2) for z1, a1, b1, a2, b2 in jobs.tolist()])
    both = _device(BRENT, cols, 2)
    _assert_bits(both[0], ref, f"gs_corr_lwc, q1 mode {mode}", *cols[:5])
    _assert_bits(both[1], ref, f"the lean job, q1 mode {mode}", *cols[:5])
    _assert_bits(_device(BRENT_OPEN4, cols, 1)[0], ref, f"job entry, groups of 4, q1 mode {mode}", *cols[:5])
    _assert_bits(_device(BRENT_OPEN2, cols, 1)[0], ref, f"job entry, groups of 2, q1 mode {mode}", *cols[:5])
