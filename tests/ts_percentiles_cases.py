"""Batches, views and the independent restatement for the percentiles of a vector of series
(shyft_hip_ts_percentiles, region.ts_percentiles_csr, api.percentiles).

A batch is the CSR form of tests/resample_cases.py. A view is (src, shift): stored series src moved shift microseconds
later. `materialise` writes every view out as a series of its own, which is what the reference's time_shift_ts is.

`reference_percentiles` is the path api.percentiles took before the batched entry existed: the true average of every
materialised series (region.resample_csr on the host), the sort and the R7 reads of region.percentiles_host, and for
MIN_EXTREME / MAX_EXTREME the Python restatement of extract_statistics (core/time_series_statistics.h:24-90), here on
int64 microseconds so that it is exact for every epoch. It shares no code with host/ts_percentiles.hpp.
"""
import numpy as np

from tests.resample_cases import AXES, EPOCHS, axis, make_batch, same_bits  # noqa: F401  (re-exported for the tests)

AVERAGE, MIN_EXTREME, MAX_EXTREME = -1, -1000, 1000
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 1000)
SHORT_LENGTHS = (0, 1, 2, 3, 5, 8)
PCT_LISTS = ([], [50], [0, 100], [-1], [-1000, 1000], [0, 10, 25, -1, 50, 75, 90, 100], [101, -2, 999],
             [(7 * k) % 101 for k in range(36)] + [-1, -1000, 1000, 555])  # the last has 40 entries


def same(a, b):
    """every pair of values has equal bits, or is NaN twice, or is zero twice (the sign of a zero result is not
    specified: +0.0 and -0.0 compare equal in a sort and in min / max); nothing else passes"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    ok = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)) | ((a == 0.0) & (b == 0.0))
    return bool(ok.all())


def identity_views(batch):
    S = len(batch[3])
    return np.arange(S, dtype=np.int32), np.zeros(S, dtype=np.int64)


def materialise(batch, src, shift):
    """the batch in which view s is row s, its times and t_end moved by shift[s]"""
    row, t, v, t_end, fx = batch
    r, ts, vs = [0], [], []
    for s, d in zip(src, shift):
        p = slice(row[s], row[s + 1])
        ts.append(t[p] + np.int64(d))
        vs.append(v[p])
        r.append(r[-1] + len(ts[-1]))
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.empty(0, dtype)  # noqa: E731
    src = np.asarray(src, dtype=np.int64)
    return (np.asarray(r, np.int64), cat(ts, np.int64), cat(vs, np.float64),
            (np.asarray(t_end, np.int64)[src] + np.asarray(shift, np.int64)).astype(np.int64),
            np.asarray(fx, np.int32)[src])


def nan_fold(pick):
    """nan_min / nan_max (time_series_statistics.h:24-39): the fold ignores non-finite values"""
    def fx(r, x):
        if not np.isfinite(x):
            return r
        if not np.isfinite(r):
            return x
        return pick(r, x)
    return fx


def extract_statistics(times, vals, t_end, ta_t0, ta_dt, T, fx):
    """extract_statistics (time_series_statistics.h:41-75): fx folded over the points of a series inside each interval
    of the axis; times in int64 microseconds"""
    n = len(times)
    t_first = ta_t0 if T else 0
    i_s = None  # make_time_axis_map(ts.time_axis(), ta).src_index(0)
    if n and times[0] <= t_first < t_end:
        i_s = int(np.searchsorted(np.asarray(times), t_first, side="right")) - 1
    r = []
    for i in range(T):
        p0, p1 = ta_t0 + i * ta_dt, ta_t0 + (i + 1) * ta_dt
        rv = float("nan")
        if i_s is None:
            if n and p0 <= times[0] < p1:
                i_s = 0
            else:
                r.append(rv)
                continue
        if i_s < n and times[i_s] < p0:
            i_s += 1
        while i_s < n and times[i_s] < p1:
            rv = fx(rv, float(vals[i_s]))
            i_s += 1
        r.append(rv)
    return r


def reference_percentiles(region, batch, src, shift, ta_t0, ta_dt, T, pcts):
    """[len(pcts)][T]: resample_csr(host=True) of the materialised views, percentiles_host, and the Python fold for
    the extremes"""
    row, t, v, t_end, fx = m = materialise(batch, src, shift)
    S, pcts = len(t_end), [int(p) for p in pcts]
    samples = region.resample_csr(*m, ta_t0, ta_dt, T, 0, host=True)
    values = region.percentiles_host(samples, pcts) if S and T and pcts else np.full((len(pcts), T), np.nan)
    for k, p in enumerate(pcts):
        if p in (MIN_EXTREME, MAX_EXTREME):
            fold = nan_fold(min if p == MIN_EXTREME else max)
            out = [float("nan")] * T
            for s in range(S):  # extract_statistic_from_vector (:77-90)
                q = slice(row[s], row[s + 1])
                x = extract_statistics([int(a) for a in t[q]], v[q], int(t_end[s]), int(ta_t0), int(ta_dt), T, fold)
                out = x if s == 0 else [fold(a, b) for a, b in zip(out, x)]
            values[k] = out
    return values


def batch_for(kind, S, epoch, seed, lengths=LENGTHS):
    """a mixed batch that the axis kind can be resampled from: the "before" axis holds the first point of every series
    strictly inside a period, which a one-point series refuses"""
    t0, dt = EPOCHS[epoch]
    return make_batch(S, t0, dt, seed, lengths=lengths, first=seed % len(lengths), min_points=2 if kind == "before" else 0)
