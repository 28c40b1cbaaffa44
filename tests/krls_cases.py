"""Series and helpers shared by tests/test_krls_host.py and tests/test_krls_gpu.py."""
import numpy as np

US = 10**6
HOUR = 3600 * US
T0 = 1451606400 * US  # 2016-01-01

# the grow-only setting: with a narrow kernel on unit spacing every sample is far from the span of the dictionary
# (delta stays near 1), so every valid point joins and the dictionary size is the count of valid points
GROW = dict(gamma=0.5, tolerance=0.001)
# the mixed setting of the issue: a wide kernel, most samples take the update branch
MIXED = dict(gamma=1e-3, tolerance=0.01)


def grow_series(valid, seed, step=HOUR, nan_every=7):
    """(t, v): `valid` random normal values on an even axis of `step`, a NaN in front of every nan_every - 1 of them"""
    rng = np.random.default_rng(seed)
    v = []
    for x in rng.normal(size=valid):
        if len(v) % nan_every == 0:
            v.append(np.nan)
        v.append(float(x))
    v = np.asarray(v, dtype=np.float64)
    return T0 + step * np.arange(v.shape[0], dtype=np.int64), v


def noisy_sine(n, seed, step=HOUR, holes=()):
    rng = np.random.default_rng(seed)
    v = np.sin(np.arange(n) / 40.0) + 0.05 * rng.normal(size=n)
    for h in holes:
        v[h] = np.nan
    return T0 + step * np.arange(n, dtype=np.int64), v


def csr(series, step=HOUR):
    """(row, t, v, t_end, fx) of a list of (t, v); an empty series ends at T0 + step"""
    row = np.concatenate([[0], np.cumsum([len(t) for t, _ in series])]).astype(np.int64)
    t = np.concatenate([np.asarray(t, np.int64) for t, _ in series]) if series else np.empty(0, np.int64)
    v = np.concatenate([np.asarray(v, np.float64) for _, v in series]) if series else np.empty(0)
    t_end = np.asarray([(t[-1] if len(t) else T0) + step for t, _ in series], np.int64)
    return row, t, v, t_end, np.zeros(len(series), np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_state(x, y):
    """two results of region.krls_train_csr, bit for bit in d_row, d, alpha, Kinv, P and mse"""
    return (np.array_equal(x[0], y[0]) and same_bits(x[1], y[1]) and same_bits(x[2], y[2])
            and all(same_bits(a, b) for a, b in zip(x[3], y[3])) and all(same_bits(a, b) for a, b in zip(x[4], y[4]))
            and same_bits(x[5], y[5]))
