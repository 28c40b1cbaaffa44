"""The step loop's two-argument inline exp and log (device/pt_dev.h kmath<true>::exp2 / log2p), bit for bit.

Both fast-path bodies of a pair run side by side (device/fastmath.h gsb_exp2 / gsb_log2) and ONE merged test sends
a pair with an argument beyond the fast domain to the general path, where each such argument takes the out-of-line
call. So each output has to be the one-argument function of its own argument whatever its partner is: inside or
beyond the domain, equal to it, or far away from it. shyft_hip_device_selftest's EXPLOG_PAIRS (include/shyft_hip.h)
evaluates the pairs from the pt_gs_k kernel file; the references are EXPLOG_INLINE's exp_fast / log_fast of the same
argument from the same library, and the oracle's exp / log. Every comparison is bit for bit (NaN equal to NaN).
"""
import ctypes as C

import numpy as np
import pytest

from tests import edge_sets, oracle_lib

pytestmark = pytest.mark.gpu

EXPLOG_INLINE, EXPLOG_PAIRS = 0, 13  # function codes of include/shyft_hip.h


def _device(fn, cols, n_out):
    from shyft_amd import _native
    a = np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.float64) for c in cols]))
    out = np.empty((n_out, a.shape[1]))
    rc = _native.lib().shyft_hip_device_selftest(fn, a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1],
                                                 out.ctypes.data_as(C.c_void_p), n_out)
    assert rc == 0, f"shyft_hip_device_selftest({fn}) failed"
    return out


def _assert_bits(got, ref, what, x, y):
    got, ref = np.asarray(got), np.asarray(ref)
    same = (got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))
    if not same.all():
        i = int(np.argmax(~same))
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} rows differ; first at row {i}, pair "
                             f"({float(x[i])!r}, {float(y[i])!r}): device {got[i]!r} ({got[i].hex()}) "
                             f"reference {ref[i]!r} ({ref[i].hex()})")


def _exp_fast(v):
    return np.abs(v) <= 708.0


def _log_fast(v):
    return (v >= edge_sets.MIN_NORMAL) & (v <= edge_sets.MAX_DOUBLE)  # positive normal finite


@pytest.fixture(scope="module")
def ref():
    """x: the exp set and the log set together; the one-argument references of every value of x, computed once: the
    oracle's exp / log and the same library's exp_fast / log_fast (EXPLOG_INLINE)."""
    L = oracle_lib.load("detmath")
    x = np.concatenate([edge_sets.exp_set(), edge_sets.log_set()])
    xs = x.tolist()
    dev = _device(EXPLOG_INLINE, [x], 2)
    return {"x": x,
            "oracle": (np.array([L.oracle_exp(v) for v in xs]), np.array([L.oracle_log(v) for v in xs])),
            "inline": (dev[0].copy(), dev[1].copy())}


def _partners(x, which):
    """Index of each row's partner in x: y = x[j]."""
    n = x.size
    if which == "same":
        return np.arange(n)
    if which == "reverse":
        return np.arange(n)[::-1].copy()
    # a seeded shuffle, then rows placed as the explog fixture of tests/test_device_functions.py places them (40
    # rows both beyond the domain, 40 x beyond and y inside, 40 x inside and y beyond), once for exp's domain and
    # once for log's, so that all four combinations occur at least 40 times for each (asserted by the test)
    rng = np.random.default_rng(113)
    j = rng.permutation(n)
    ix = np.arange(n)
    for fast, skip in ((_exp_fast, 0), (_log_fast, 120)):
        beyond = np.flatnonzero(~fast(x))[skip:]
        inside = np.flatnonzero(fast(x))[skip:]
        j[beyond[:40]] = ix[beyond[40:80]]
        j[beyond[80:120]] = ix[inside[:40]]
        j[inside[40:80]] = ix[beyond[:40]]
    return j


@pytest.mark.parametrize("which", ["shuffled", "same", "reverse"])
def test_pairs(ref, which):
    """exp2(x, y) and log2p(x, y): each output is the one-argument function of its own argument, bit for bit."""
    x = ref["x"]
    j = _partners(x, which)
    y = x[j]
    if which == "shuffled":
        for fast, name in ((_exp_fast, "exp"), (_log_fast, "log")):
            fx, fy = fast(x), fast(y)
            for cx in (True, False):
                for cy in (True, False):
                    assert ((fx == cx) & (fy == cy)).sum() >= 40, f"{name}: combination x {cx} y {cy} too rare"
    out = _device(EXPLOG_PAIRS, [x, y], 4)
    for src in ("inline", "oracle"):
        e, l = ref[src]
        _assert_bits(out[0], e, f"exp2(x, y).a against {src} exp(x)", x, y)
        _assert_bits(out[1], e[j], f"exp2(x, y).b against {src} exp(y)", x, y)
        _assert_bits(out[2], l, f"log2p(x, y).a against {src} log(x)", x, y)
        _assert_bits(out[3], l[j], f"log2p(x, y).b against {src} log(y)", x, y)
