"""Batches and parameters for the point-wise filter calls (region.ts_convolve_w_csr, ts_derivative_csr, ts_inside_csr,
ts_decode_csr), shared by tests/test_tsfilter_host.py and tests/test_tsfilter_gpu.py.

The series batches are those of tests/resample_cases.py (lengths rotating over 0, 1, 2, 3, 63, 64, 65, 257, 1000, three
time bases, both point types, NaN / inf hazards; series with an even index are evenly spaced, the odd ones irregular).
Where S > 8, series 8 is replaced by one of 3 * TILE + 228 points, so one series spans more than three tiles of the
tiled convolution and most series start in the middle of a tile of the flat array.
"""
import numpy as np

from tests import resample_cases as rc
from tests import tsprep_cases as tc

NAN = float("nan")
TILE = 256    # output points per workgroup of the tiled convolution in kernels/tsfilter.hip (TF_TILE)
CHUNK = 256   # taps per staged window there (TF_CHUNK)
BLOCK = 256   # lanes per workgroup of the pointwise kernels there (TF_BLOCK)
N_LONG = 3 * TILE + 228
LONG_AT = 8
SS = (1, 63, 64, 65, 257)
KS = (0, 1, 2, 5, 63, 64, 65, 255, 256, 257, 300, 2 * TILE + 3)
USE_FIRST, USE_ZERO, USE_NAN = 0, 1, 2
DEFAULT, FORWARD, BACKWARD, CENTER = 0, 1, 2, 3


def batch(S, k, seed=9300):
    """(t0, dt, (row, t, v, t_end, fx), fixed_dt): fixed_dt [S] is dt for the evenly spaced series and 0 for the rest"""
    t0, dt = rc.EPOCHS[k % len(rc.EPOCHS)]
    if S > LONG_AT:
        b = tc.long_batch(S, t0, dt, seed + S, LONG_AT, N_LONG)  # the long series has irregular times
    else:
        b = rc.make_batch(S, t0, dt, seed + S, first=7 if S == 1 else 0)  # S == 1: one series of 257 points
    fixed = np.array([dt if s % 2 == 0 and not (S > LONG_AT and s == LONG_AT) else 0 for s in range(S)], np.int64)
    return t0, dt, b, fixed


def weights(K, seed):
    """K weights with exact zeros and negatives among them"""
    rng = np.random.default_rng(seed)
    w = rng.normal(0.0, 1.0, K)
    w[rng.random(K) < 0.15] = 0.0
    return w


def profiles(Ks, seed, nan_in=()):
    """(w_row, w) of one profile per entry of Ks; the profiles listed in nan_in get a NaN in the middle"""
    parts = []
    for p, K in enumerate(Ks):
        w = weights(K, seed + p)
        if p in nan_in and K:
            w[K // 2] = np.nan
        parts.append(w)
    w_row = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return w_row, (np.concatenate(parts) if parts else np.empty(0))


def with_nan_runs(b, flat_boundary=BLOCK):
    """the batch with NaN runs of two points at the first, second, last-but-one and last point of series of at least
    8 points (rotating over the four places) and a run over the flat points flat_boundary - 3 .. flat_boundary + 2,
    which lie in two workgroups of a pointwise kernel"""
    row, t, v, t_end, fx = b
    v = v.copy()
    place = 0
    for s in range(len(row) - 1):
        a, e = int(row[s]), int(row[s + 1])
        if e - a < 8:
            continue
        at = (a, a + 1, e - 3, e - 2)[place % 4]
        v[at:at + 2] = np.nan
        place += 1
    if len(v) > flat_boundary + 3:
        v[flat_boundary - 3:flat_boundary + 3] = np.nan
    return row, t, v, t_end, fx


def decode_values(b, seed):
    """the batch with values for decode: integers up to 2^52, 2^52 + 2, non-integers, negatives, NaN and inf"""
    row, t, v, t_end, fx = b
    rng = np.random.default_rng(seed)
    n = len(v)
    x = np.floor(rng.random(n) * 2.0 ** rng.integers(1, 53, n))
    kind = rng.integers(0, 12, n)
    x[kind == 0] = 2.0 ** 52
    x[kind == 1] = 2.0 ** 52 + 2
    x[kind == 2] += 0.75
    x[kind == 3] = -x[kind == 3] - 1.0
    x[kind == 4] = np.nan
    x[kind == 5] = np.inf
    x[kind == 6] = 2.0 ** 52 - 1
    x[kind == 7] = 0.0
    return row, t, x, t_end, fx


def same(a, b, what=""):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(~((np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))))
    assert rc.same_bits(a, b), (what, len(bad), bad[:4].tolist(), a[bad[:4, 0]].tolist(), b[bad[:4, 0]].tolist())
