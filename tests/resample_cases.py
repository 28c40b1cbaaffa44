"""Batches of point series in the CSR form of shyft_hip_resample, and the axes they are resampled onto.

A batch has S series on a common base time t0 and spacing dt (int64 microseconds). Series k has N = lengths[k % len]
points, alternates between evenly spaced and irregular times (every point but the first moved by a random whole
number of microseconds inside its step), alternates the point type every two series, and takes one of eight value
hazards by k % 8: plain, about 20 % NaN, a NaN run over the middle third (whole target intervals without a finite
point), NaN first and last point, all NaN, +-inf among the values, about 20 % NaN again (it falls on the other
spacing kind), negative values with exact zeros. Series differ in length, so one axis is at once inside, past the end
of and wholly after different rows of the batch.
"""
import numpy as np

HOUR = 3600 * 10**6
T_2016 = 1451606400 * 10**6            # about 1.45e15 us
T_NEGATIVE = -86400 * 10**6 * 365 * 7  # 1963
T_ABOVE_2_53 = 2**53 + 1               # odd: the conversion of these times to fp64 rounds
EPOCHS = ((T_2016, HOUR), (T_NEGATIVE, 3 * HOUR), (T_ABOVE_2_53, HOUR + 1))
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 257, 1000)
AXES = ("own", "x2", "x24", "half", "quarter", "shifted", "before", "before_aligned", "past_end", "wholly_before",
        "wholly_after")


def make_batch(S, t0, dt, seed, lengths=LENGTHS, first=0, min_points=0):
    """(row, t, v, t_end, fx) of S series; `first` rotates the lengths, min_points raises the short ones."""
    rng = np.random.default_rng(seed)
    row, ts, vs, t_end, fx = [0], [], [], [], []
    for k in range(S):
        n = max(lengths[(k + first) % len(lengths)], min_points)
        t = t0 + dt * np.arange(n, dtype=np.int64)
        end = t0 + dt * n
        if k % 2 and n:
            off = rng.integers(0, dt, n, dtype=np.int64)
            off[0] = 0
            t = t + off
            end = int(t[-1]) + int(rng.integers(1, dt + 1))
        v = rng.normal(5.0, 10.0, n)
        h = k % 8
        if h in (1, 6):
            v[rng.random(n) < 0.2] = np.nan
        elif h == 2:
            v[n // 3: 2 * n // 3 + 1] = np.nan
        elif h == 3 and n:
            v[0] = v[-1] = np.nan
        elif h == 4:
            v[:] = np.nan
        elif h == 5:
            v[rng.random(n) < 0.1] = np.inf
            v[rng.random(n) < 0.1] = -np.inf
        elif h == 7:
            v = -np.abs(v)
            v[rng.random(n) < 0.2] = 0.0
        row.append(row[-1] + n)
        ts.append(t)
        vs.append(v)
        t_end.append(end)
        fx.append((k // 2) % 2)
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.empty(0, dtype)  # noqa: E731
    return (np.asarray(row, np.int64), cat(ts, np.int64), cat(vs, np.float64), np.asarray(t_end, np.int64),
            np.asarray(fx, np.int32))


def axis(kind, t0, dt, T):
    """(ta_t0, ta_dt) of a T-step axis against series that start at t0 with spacing dt."""
    return {
        "own": (t0, dt),
        "x2": (t0, 2 * dt),
        "x24": (t0, 24 * dt),
        "half": (t0, dt // 2),
        "quarter": (t0, dt // 4),
        "shifted": (t0 + dt // 4, dt),
        # periods that start before the first point: two that end before it, then one that holds it
        "before": (t0 - 2 * dt - dt // 2, dt),
        "before_aligned": (t0 - 3 * dt, dt),
        # the last steps of a 63- to 65-point series, its end and beyond (a regular series ends on a period start)
        "past_end": (t0 + 60 * dt, dt),
        "wholly_before": (t0 - (T + 2) * dt, dt),
        "wholly_after": (t0 + 1100 * dt, dt),
    }[kind]


def same_bits(a, b):
    """NaN in the same places and the finite values (and infinities) equal as bit patterns"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))
