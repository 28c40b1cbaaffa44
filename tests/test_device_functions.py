"""The device-only restatements of the hot paths, function by function, against the oracle's own entry points.

The stack parity tests compare whole runs on the synthetic region, which never produces the arguments at which these
functions change path. Here shyft_hip_device_selftest (include/shyft_hip.h) runs each of them on chosen inputs from
test kernels that live in the kernel file whose run kernel calls them:
  device/fastmath.h   gsb_exp / gsb_log through exp_fast / log_fast (the inline exp / log of the step loops) and
                      through dexp / dlog / dexp2 as built with the SGPR constant table (pt_ss_k);
  device/special.h    dexp / dlog / dexp2 as out-of-line detmath calls (pt_gs_k), dpowr, dpow4, dpow8, dpow;
  device/gamma_lean.h gsb_gamma_pq and the general redo it asks for (gs_gamma_pq_cs);
  device/gs_brent.h   gs_corr_lwc_lean, gs_corr_lwc_spec + gs_corr_lwc_memo on 4 and 2 lanes per job, against
                      gs_corr_lwc;
  device/ptssk_dev.h  ss_sca_rel_red and ss_sca_rel_red_group on 2 and 4 lanes per job.
Every comparison is bit for bit (NaN equal to NaN); a failure names the first differing input. How accurate detmath
itself is at the same arguments is tests/test_detmath.py's business.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import edge_sets, oracle_lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# function codes of include/shyft_hip.h
EXPLOG_INLINE, EXPLOG_CALLS, EXPLOG_TABLE, POWERS, GAMMA_LEAN, BRENT, BRENT_SPEC4, BRENT_SPEC2, SKAUGEN, \
    SKAUGEN_GROUP2, SKAUGEN_GROUP4 = range(11)


def _device(fn, cols, n_out):
    """cols: the input columns (equal lengths) -> out [n_out][n]."""
    from shyft_amd import _native
    a = np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.float64) for c in cols]))
    out = np.empty((n_out, a.shape[1]))
    rc = _native.lib().shyft_hip_device_selftest(fn, a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1],
                                                 out.ctypes.data_as(C.c_void_p), n_out)
    assert rc == 0, f"shyft_hip_device_selftest({fn}) failed"
    return out


def _assert_bits(got, ref, what, *inputs):
    got, ref = np.asarray(got), np.asarray(ref)
    same = (got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))
    if not same.all():
        i = int(np.argmax(~same))
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} rows differ; first at row {i}, input "
                             f"{tuple(float(c[i]) for c in inputs)!r}: device {got[i]!r} ({got[i].hex()}) "
                             f"reference {ref[i]!r} ({ref[i].hex()})")


def _map(f, *cols):
    return np.array([f(*v) for v in zip(*(np.asarray(c, dtype=np.float64).tolist() for c in cols))], dtype=np.float64)


@pytest.fixture(scope="module")
def dm():
    L = oracle_lib.load("detmath")
    d = C.c_double
    L.oracle_gamma_pq_rescaled.restype = C.c_int
    L.oracle_gamma_pq_rescaled.argtypes = [d, d, d]
    L.oracle_powr.restype = d
    L.oracle_powr.argtypes = [d, d]
    for f in (L.oracle_pow4, L.oracle_pow8):
        f.restype = d
        f.argtypes = [d]
    L.oracle_skaugen_sca_rel_red_checked.restype = C.c_int
    L.oracle_skaugen_sca_rel_red_checked.argtypes = [C.c_uint64, C.c_uint64, d, d, C.POINTER(d)]
    return L


# ------------------------------------------------------------------------------------------------ exp / log
@pytest.fixture(scope="module")
def explog(dm):
    """x: the exp set and the log set together (each function sees both); y: x shuffled, with rows made so that all
    four combinations of |x| <= 708 and |y| <= 708 (dexp2's fast / general split) occur; the oracle's exp and log."""
    x = np.concatenate([edge_sets.exp_set(), edge_sets.log_set()])
    rng = np.random.default_rng(104)
    y = x[rng.permutation(x.size)].copy()
    beyond = np.flatnonzero(~(np.abs(x) <= 708.0))
    inside = np.flatnonzero(np.abs(x) <= 708.0)
    y[beyond[:40]] = x[beyond[40:80]]   # both beyond
    y[beyond[80:120]] = x[inside[:40]]  # x beyond, y inside
    y[inside[40:80]] = x[beyond[:40]]   # x inside, y beyond
    xi, yi = np.abs(x) <= 708.0, np.abs(y) <= 708.0
    for cx in (True, False):
        for cy in (True, False):
            assert ((xi == cx) & (yi == cy)).sum() >= 40
    return {"x": x, "y": y, "exp_x": _map(dm.oracle_exp, x), "log_x": _map(dm.oracle_log, x),
            "exp_y": _map(dm.oracle_exp, y)}


def test_inline_exp_log(explog):
    """exp_fast / log_fast (kmath<true>): gsb_exp / gsb_log inline, the call beyond |x| <= 708 / the positive normals."""
    x = explog["x"]
    out = _device(EXPLOG_INLINE, [x], 2)
    _assert_bits(out[0], explog["exp_x"], "exp_fast", x)
    _assert_bits(out[1], explog["log_x"], "log_fast", x)


@pytest.mark.parametrize("fn,what", [(EXPLOG_CALLS, "detmath calls (pt_gs_k)"), (EXPLOG_TABLE, "table calls (pt_ss_k)")])
def test_exp_log_calls(explog, fn, what):
    """dexp, dlog and the two-argument dexp2 as each kernel file builds them (SHYFT_TABLE_CALLS 0 / 1)."""
    x, y = explog["x"], explog["y"]
    out = _device(fn, [x, y], 4)
    _assert_bits(out[0], explog["exp_x"], f"dexp, {what}", x)
    _assert_bits(out[1], explog["log_x"], f"dlog, {what}", x)
    _assert_bits(out[2], explog["exp_x"], f"dexp2(x, y).a, {what}", x, y)
    _assert_bits(out[3], explog["exp_y"], f"dexp2(x, y).b, {what}", x, y)


def test_powers(dm):
    """dpowr = exp(y log x) (OPOWR), dpow4, dpow8 (OPOW4 / OPOW8) and the double-double dpow (OPOW)."""
    x, y = edge_sets.pow_set()
    out = _device(POWERS, [x, y], 4)
    _assert_bits(out[0], _map(dm.oracle_powr, x, y), "dpowr", x, y)
    _assert_bits(out[1], _map(dm.oracle_pow4, x), "dpow4", x)
    _assert_bits(out[2], _map(dm.oracle_pow8, x), "dpow8", x)
    _assert_bits(out[3], _map(dm.oracle_pow, x, y), "dpow", x, y)


# ------------------------------------------------------------------------------------------------ lean gamma
def _gamma_set():
    shapes = (0.05, 0.1, 0.5, 1.26, 1.999, 2.0, 2.03, 6.245, 6.25, 30.0, 300.0, 1000.0, 4000.0)
    a, x = [], []
    for s in shapes:
        xs = [(s + 1.0) * m for m in (1e-6, 0.2, 0.9, 0.999, 1.0001, 1.5, 3.0, 20.0)] + edge_sets.neighbours(s + 1.0, 1)
        xs += [0.0, -1.0, 5e-324, 1e-310, edge_sets.MIN_NORMAL, 1e-300, 800.0, 1e5, edge_sets.INF, edge_sets.NAN]
        a += [s] * len(xs)
        x += xs
    rng = np.random.default_rng(105)
    ar = np.exp(rng.uniform(np.log(0.05), np.log(300.0), 3000))
    return np.concatenate([a, ar]), np.concatenate([x, ar * rng.uniform(0.0, 3.0, 3000)])


def test_lean_gamma_and_its_general_redo(dm):
    """gsb_gamma_pq has no 2^-200 rescale and covers positive normal x with |a log x - x - lgamma a| <= 708 only; it
    must say so (ok = 0) wherever the general evaluation is needed, and gs_gamma_pq_cs, which redoes those rows,
    must then return detmath's (p, p1, prefix) on every row. a = 1000, x = 0.9 * 1001 (series) and a = 4000,
    x = 4001 (continued fraction) are rows that rescale at the policy eps."""
    a, x = _gamma_set()
    out = _device(GAMMA_LEAN, [a, x], 4)
    p, p1, pre = C.c_double(), C.c_double(), C.c_double()
    ref = np.empty((3, a.size))
    for i, (ai, xi) in enumerate(zip(a.tolist(), x.tolist())):
        dm.oracle_gamma_pq_policy(ai, xi, C.byref(p), C.byref(p1), C.byref(pre))
        ref[:, i] = p.value, p1.value, pre.value
    ok = out[3]
    assert np.isin(ok, (0.0, 1.0)).all()
    # the three reasons for the general evaluation
    eps = np.where(a < 2.0, 2.0 ** -35, 2.0 ** -18)  # detmath::gamma_snow_policy_eps
    rescaled = np.array([dm.oracle_gamma_pq_rescaled(ai, xi, ei) for ai, xi, ei in zip(a.tolist(), x.tolist(), eps.tolist())]) > 0
    normal = (x >= edge_sets.MIN_NORMAL) & (x <= edge_sets.MAX_DOUBLE)
    arg = np.zeros(a.size)
    arg[normal] = a[normal] * _map(dm.oracle_log, x[normal]) - x[normal] - _map(dm.oracle_lgamma_fn, a[normal])
    far = normal & ~(np.abs(arg) <= 708.0)
    counts = {"rescaled": int(rescaled.sum()), "x not a positive normal": int((~normal).sum()),
              "|exp argument| > 708": int(far.sum()), "ok == 0": int((ok == 0).sum()), "ok == 1": int((ok == 1).sum())}
    print("lean gamma rows:", counts)
    for why, rows in (("rescaled", rescaled), ("x not a positive normal", ~normal), ("|exp argument| > 708", far)):
        assert rows.any(), f"no row with: {why}"
        bad = rows & (ok != 0)
        assert not bad.any(), f"ok == 1 on a row that needs the general evaluation ({why}): a, x = " \
                              f"{a[np.argmax(bad)]!r}, {x[np.argmax(bad)]!r}"
    for ai, xi in ((1000.0, 0.9 * 1001.0), (4000.0, 4001.0)):
        row = np.flatnonzero((a == ai) & (x == xi))
        assert row.size and rescaled[row].all(), (ai, xi)
    assert (ok == 1).sum() >= 3000
    for k, nm in enumerate(("p", "p1", "prefix")):
        _assert_bits(out[k], ref[k], f"gs_gamma_pq_cs {nm}", a, x)


# ------------------------------------------------------------------------------------------------ Brent jobs
BRENT_EDGE = ((900.0, 1000.0, 1.0, 1100.0, 0.9),       # series rescale inside the lean f
              (3990.0, 4000.0, 1.0, 4100.0, 0.98),     # continued-fraction rescale
              (1e-300, 6.25, 0.01, 6.0, 0.012),        # points at and below 0
              (5e3, 6.25, 0.01, 6.0, 0.012),           # |exp argument| > 708
              (0.3, 0.5, 0.5, 0.4, 0.7),               # both shapes below 2: the 2^-35 policy
              (0.3, 1.999, 0.1, 2.0, 0.1))             # the two policies on either side of 2


@pytest.fixture(scope="module")
def brent(dm):
    rec = np.load(os.path.join(GOLDEN, "brent_jobs_sample.npy"))  # z1 a1 b1 a2 b2, recorded from the oracle's January
    assert rec.shape == (2048, 5) and rec.dtype == np.float64
    rng = np.random.default_rng(106)
    a1 = rng.uniform(0.1, 2.0, 200)
    b1 = np.exp(rng.uniform(np.log(0.01), np.log(30.0), 200))
    low = np.stack([a1 * b1 * rng.uniform(0.05, 2.0, 200), a1, b1, rng.uniform(0.1, 2.0, 200),
                    b1 * rng.uniform(0.8, 1.2, 200)], axis=1)
    jobs = np.concatenate([rec, np.array(BRENT_EDGE), low])
    cols = [np.ascontiguousarray(jobs[:, k]) for k in range(5)]
    ref = _map(lambda z1, a1, b1, a2, b2: dm.oracle_gs_corr_lwc(z1, a1, b1, 0.0, a2, b2), *cols)
    # z2 is not used by corr_lwc
    z2 = _map(lambda z1, a1, b1, a2, b2: dm.oracle_gs_corr_lwc(z1, a1, b1, 0.5 * z1 + 1.0, a2, b2), *cols)
    _assert_bits(z2, ref, "oracle_gs_corr_lwc with another z2", *cols)
    edge = ref[len(rec):len(rec) + len(BRENT_EDGE)]
    assert np.isfinite(edge).all(), edge
    moved = ref[:len(rec)] != rec[:, 0]
    assert moved.sum() * 2 >= len(rec), "the solver did not iterate on half of the recorded jobs"
    return {"cols": cols, "ref": ref}


@pytest.mark.parametrize("mode", [0, 1])
def test_brent_job_paths(brent, mode):
    """gs_corr_lwc (the reference-shaped job), gs_corr_lwc_lean (the job the solving wavefront runs) and the
    speculative opening on 4 and 2 lanes per job with the memo solve, with Q1 left to the job (mode 0) or supplied
    (mode 1): all the oracle's corr_lwc, bit for bit."""
    cols = brent["cols"] + [np.full(brent["ref"].size, float(mode))]
    both = _device(BRENT, cols, 2)
    _assert_bits(both[0], brent["ref"], f"gs_corr_lwc, q1 mode {mode}", *cols[:5])
    _assert_bits(both[1], brent["ref"], f"gs_corr_lwc_lean, q1 mode {mode}", *cols[:5])
    _assert_bits(_device(BRENT_SPEC4, cols, 1)[0], brent["ref"], f"spec + memo, 4 lanes, q1 mode {mode}", *cols[:5])
    _assert_bits(_device(BRENT_SPEC2, cols, 1)[0], brent["ref"], f"spec + memo, 2 lanes, q1 mode {mode}", *cols[:5])


# ------------------------------------------------------------------------------------------------ Skaugen jobs
def _skaugen_jobs():
    rec = np.load(os.path.join(GOLDEN, "ptssk_jobs_sample.npy"))  # columns 0-3: u n nu_a alpha
    assert rec.shape == (4000, 9)
    edge = [(u, n, nu, al) for u, n in ((7, 7), (5806, 5806), (1, 5806), (3, 100))
            for nu in (0.5, 0.999, 1.0, 1024.0, 4095.9, 23502.0) for al in (0.21, 40.77)]
    return np.concatenate([rec[:, :4], np.array(edge, dtype=np.float64)])


def test_skaugen_job_paths(dm):
    """ss_sca_rel_red by one lane and by groups of 2 and 4 lanes per job: the same value and the same error code on
    every row, the oracle's sca_rel_red where it returns one, and an error code exactly where the oracle raises (the
    pdf's pole at 0 for a shape below 1, or bisect's evaluation error)."""
    jobs = _skaugen_jobs()
    cols = [np.ascontiguousarray(jobs[:, k]) for k in range(4)]
    v = C.c_double()
    ref = np.full(len(jobs), np.nan)
    raised = np.zeros(len(jobs), dtype=np.int64)
    for i, (u, n, nu, al) in enumerate(jobs.tolist()):
        raised[i] = dm.oracle_skaugen_sca_rel_red_checked(int(u), int(n), nu, al, C.byref(v))
        if raised[i] == 0:
            ref[i] = v.value
    print(f"skaugen jobs: {len(jobs)}, oracle raised pole {int((raised == 1).sum())}, bisect {int((raised == 2).sum())}")
    assert (raised[:4000] == 0).all()  # recorded jobs come from a run that completed
    single = _device(SKAUGEN, cols, 2)
    g2 = _device(SKAUGEN_GROUP2, cols, 2)
    g4 = _device(SKAUGEN_GROUP4, cols, 2)
    for nm, g in (("group of 2", g2), ("group of 4", g4)):
        _assert_bits(g[1], single[1], f"error code, {nm} vs one lane", *cols)
        _assert_bits(g[0], single[0], f"value, {nm} vs one lane", *cols)
    err = single[1]
    mism = (err != 0) != (raised != 0)
    assert not mism.any(), f"device error code {err[np.argmax(mism)]} where the oracle " \
                           f"{'raised' if raised[np.argmax(mism)] else 'returned'}: job {jobs[np.argmax(mism)]!r}"
    good = raised == 0
    _assert_bits(single[0][good], ref[good], "ss_sca_rel_red vs oracle", *[c[good] for c in cols])
