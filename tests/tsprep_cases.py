"""Batches for the observation-preparation calls (region.ts_*_csr) and plain-Python transcriptions of the four rules.

The transcriptions are written from the reference's text (core/time_series.h:202-284, 1395-1408, 1493-1506, 1808-1831;
core/time_series_dd.h:1323-1354, 1463-1471; core/time_series_dd.cpp:1335-1376) with ordinary loops, Python ints for
the microsecond ticks and math.exp / math.pow. They do not use host/ts_prep.hpp or anything compiled.
"""
import bisect
import math

import numpy as np

from tests import resample_cases as rc

NAN = float("nan")
DISALLOW_MISSING, ALLOW_INITIAL_MISSING, ALLOW_ANY_MISSING = 0, 1, 2
SCAN_SPAN = 1024  # keys per workgroup of the index scan in kernels/tsprep.hip


def to_seconds(dt):
    return float(dt) / 1e6


def series(batch, s):
    """(t list of int, v list of float, t_end, fx) of series s of a CSR batch"""
    row, t, v, t_end, fx = batch
    a, b = int(row[s]), int(row[s + 1])
    return [int(x) for x in t[a:b]], [float(x) for x in v[a:b]], int(t_end[s]), int(fx[s])


# ---- accumulate_value (time_series.h:202-284) over a point_dt axis (time_axis.h:329-374) -------------------------------
def _open_range_index_of(t, t_end, tx):
    n = len(t)
    if n == 0:
        return None
    if tx >= t_end:
        return n - 1
    if tx < t[0]:
        return None
    if tx >= t[-1]:
        return n - 1
    return bisect.bisect_right(t, tx) - 1


def accumulate_value(t, v, t_end, ps, pe, linear):
    """(area or NaN, tsum)"""
    n = len(t)
    extrapolate_flat = not linear
    if n == 0:
        return NAN, 0
    i = _open_range_index_of(t, t_end, ps)
    lt, lv, l_finite = 0, NAN, False
    if i is None:
        i = 0
        lt, lv = t[i], v[i]
        i += 1
        l_finite = math.isfinite(lv)
        if not ps <= lt < pe:
            return NAN, 0
    area, tsum = 0.0, 0
    while True:
        if not l_finite:
            lt, lv = t[i], v[i]
            i += 1
            l_finite = math.isfinite(lv)
            if i == n:
                if l_finite and lt < pe:
                    if extrapolate_flat:
                        dt = pe - max(ps, lt)
                        tsum += dt
                        area += to_seconds(dt) * lv
                break
            if lt >= pe:
                break
        else:
            rt, rv = t[i], v[i]
            i += 1
            r_finite = math.isfinite(rv)
            px_start, px_end = max(lt, ps), min(rt, pe)
            dt = px_end - px_start
            if linear and r_finite:
                a = (rv - lv) / to_seconds(rt - lt)
                b = rv - a * to_seconds(rt)
                area += to_seconds(dt) * (0.5 * a * to_seconds(px_start + px_end) + b)
                tsum += dt
            elif extrapolate_flat:
                area += lv * to_seconds(dt)
                tsum += dt
            if i == n:
                if r_finite and rt < pe:
                    if extrapolate_flat:
                        dt = pe - rt
                        tsum += dt
                        area += to_seconds(dt) * rv
                break
            if rt >= pe:
                break
            l_finite, lt, lv = r_finite, rt, rv
    return (area if tsum else NAN), tsum


# ---- ice packing (time_series.h:1808-1831) ---------------------------------------------------------------------------------
def detect_ice_packing(t, v, t_end, fx, window, threshold, policy, tq):
    ps, pe = tq - window, tq
    start = t[0] if t else 0  # total_period() of an empty series is [0, 0)
    if policy != DISALLOW_MISSING:
        if ps < start:
            ps = min(start, pe)
    if pe - ps == 0:
        return 0.0
    p_sum, t_sum = accumulate_value(t, v, t_end, ps, pe, fx == 0)
    if not math.isfinite(p_sum) or t_sum == 0:
        return NAN
    if policy == ALLOW_ANY_MISSING or t_sum == pe - ps:
        return 1.0 if p_sum / to_seconds(t_sum) < threshold else 0.0
    return NAN


def ice_packing(batch, qrow, qt, window, threshold, policy):
    S = len(batch[0]) - 1
    out = np.empty(len(qt))
    for s in range(S):
        t, v, t_end, fx = series(batch, s)
        for j in range(int(qrow[s]), int(qrow[s + 1])):
            out[j] = detect_ice_packing(t, v, t_end, fx, int(window[s]), float(threshold[s]), int(policy[s]), int(qt[j]))
    return out


# ---- ice packing recession (time_series_dd.h:1323-1354) ------------------------------------------------------------------
def flow_at_own_point(t, v, fx, i):
    """point_ts::operator()(time(i)) (time_series.h:360-380)"""
    if fx == 0 and i + 1 < len(t):
        a = (v[i + 1] - v[i]) / to_seconds(t[i + 1] - t[i])
        return v[i] + a * to_seconds(t[i] - t[i])
    return v[i]


def recession_terms(t, v, fx, ice, alpha, qbf, i):
    """(value, qs) of point i: qs is None when the value does not come from the recession formula"""
    x = ice[i]
    if not math.isfinite(x):
        return NAN, None
    if x > 0.5:
        f_ix = i
        while f_ix > 0 and x > 0.5:
            f_ix -= 1
            x = ice[f_ix]
            if not math.isfinite(x):
                return NAN, None
        qs, ts = v[f_ix], t[f_ix]
        return qbf + (qs - qbf) * math.exp(-alpha * to_seconds(t[i] - ts)), qs
    return flow_at_own_point(t, v, fx, i), None


# ---- min-max check with linear fill (time_series_dd.h:1463-1471, time_series_dd.cpp:1335-1376) -------------------------------
def is_ok_quality(x, min_x, max_x):
    if not math.isfinite(x):
        return False
    if math.isfinite(min_x) and x < min_x:
        return False
    if math.isfinite(max_x) and x > max_x:
        return False
    return True


def fill_value(t, v, min_x, max_x, max_timespan, i):
    x = v[i]
    if is_ok_quality(x, min_x, max_x):
        return x
    n = len(t)
    if i == 0 or i + 1 >= n or max_timespan == 0:
        return NAN
    j = i
    while j > 0:
        j -= 1
        t0 = t[j]
        if t[i] - t0 > max_timespan:
            return NAN
        x0 = v[j]
        if is_ok_quality(x0, min_x, max_x):
            for k in range(i + 1, n):
                t1 = t[k]
                if t1 - t0 > max_timespan:
                    return NAN
                x1 = v[k]
                if is_ok_quality(x1, min_x, max_x):
                    a = (x1 - x0) / to_seconds(t1 - t0)
                    b = x0 - a * to_seconds(t0)
                    return a * to_seconds(t[i]) + b
    return NAN


def min_max_fill(batch, min_x, max_x, max_timespan):
    S = len(batch[0]) - 1
    out = np.empty(len(batch[1]))
    for s in range(S):
        t, v, _, _ = series(batch, s)
        for i in range(len(t)):
            out[int(batch[0][s]) + i] = fill_value(t, v, float(min_x[s]), float(max_x[s]), int(max_timespan[s]), i)
    return out


# ---- rating curve (time_series.h:1395-1408, 1493-1506) ---------------------------------------------------------------------
def rating_segment(curves, tq, level):
    """curves: [(t, [(lower, a, b, c), ...]), ...] ascending; the segment rating_curve_parameters::flow(t, level)
    evaluates, or None where it gives NaN without evaluating one"""
    if not curves:
        return None
    times = [c[0] for c in curves]
    it = bisect.bisect_left(times, tq)
    if it == 0 and times[it] > tq:
        return None
    if it == len(curves) or times[it] > tq:
        it -= 1
    segs = curves[it][1]
    g = 0  # lower_bound on `lower < level`
    while g < len(segs) and segs[g][0] < level:
        g += 1
    if g != len(segs) and level == segs[g][0]:
        return segs[g]
    if g != 0:
        return segs[g - 1]
    return None


def packs_csr(packs):
    """pack_row, curve_t, curve_row, seg of a list of packs in the form of rating_segment's `curves`"""
    pack_row, curve_t, curve_row, seg = [0], [], [0], []
    for curves in packs:
        for t, segs in curves:
            curve_t.append(t)
            seg.extend(segs)
            curve_row.append(len(seg))
        pack_row.append(len(curve_t))
    return (np.asarray(pack_row, np.int64), np.asarray(curve_t, np.int64), np.asarray(curve_row, np.int64),
            np.asarray(seg, np.float64).reshape(-1, 4))


def make_packs(n_packs, t0, dt, seed):
    """packs with 1 or 3 curves of 1 to 9 segments; curve times fall on, between and before the points of a series that
    starts at t0 with spacing dt; levels of make_batch are N(5, 10), so lowers spread over -15 .. 25 and some b lie
    above the level (a negative base), with integer and fractional exponents"""
    rng = np.random.default_rng(seed)
    packs = []
    for p in range(n_packs):
        n_curves = 1 if p % 2 == 0 else 3
        starts = [t0 + 2 * dt, t0 + 7 * dt + dt // 3, t0 + 40 * dt][:n_curves] if p % 3 else [t0 - dt, t0 + 5 * dt, t0 + 64 * dt][:n_curves]
        curves = []
        for c, ts in enumerate(starts):
            n_seg = 1 + (p * 3 + c * 4) % 9
            lowers = np.sort(rng.choice(np.arange(-15.0, 25.0, 0.5), n_seg, replace=False))
            segs = [(float(lo), float(rng.uniform(0.5, 3.0)), float(lo - rng.choice([0.0, 0.25, -3.0])),
                     float(rng.choice([1.0, 2.0, 3.0, 1.5, 2.37, 0.5]))) for lo in lowers]
            curves.append((int(ts), segs))
        packs.append(curves)
    return packs


def ulp_distance(a, b):
    """the distance of two finite doubles in units in the last place of b"""
    return abs(a - b) / math.ulp(b)


# ---- batches ------------------------------------------------------------------------------------------------------------
def ice_policies(batch, shift):
    """the three policies rotating over the series; a one-point series never DISALLOW_MISSING (a window over its
    point is refused, as point_dt::time throws in the reference)"""
    row = batch[0]
    policy = np.array([(s + shift) % 3 for s in range(len(row) - 1)], np.int32)
    one = (row[1:] - row[:-1]) == 1
    policy[one & (policy == DISALLOW_MISSING)] = ALLOW_INITIAL_MISSING
    return policy


def foreign_axis(batch, t0, dt):
    """(qrow, qt): per series a query axis shifted by a quarter spacing, from two steps before t0 to past the end"""
    row = batch[0]
    qrow, qt = [0], []
    for s in range(len(row) - 1):
        n = int(row[s + 1] - row[s])
        qt.extend(t0 - 2 * dt + dt // 4 + dt * k for k in range(n + 5))
        qrow.append(len(qt))
    return np.asarray(qrow, np.int64), np.asarray(qt, np.int64)


def ice_windows(dt):
    """0, below one spacing, exactly one, 2.5 spacings, longer than any series"""
    return (0, dt // 3, dt, 5 * dt // 2, 5000 * dt)
def long_batch(S, t0, dt, seed, long_at, n_long):
    """make_batch with series long_at replaced by one of n_long points (several scan spans), irregular times"""
    row, t, v, t_end, fx = rc.make_batch(S, t0, dt, seed)
    rng = np.random.default_rng(seed + 1)
    a, b = int(row[long_at]), int(row[long_at + 1])
    tl = t0 + dt * np.arange(n_long, dtype=np.int64) + rng.integers(0, dt // 2, n_long, dtype=np.int64)
    vl = rng.normal(5.0, 10.0, n_long)
    vl[rng.random(n_long) < 0.2] = np.nan
    t = np.concatenate([t[:a], tl, t[b:]])
    v = np.concatenate([v[:a], vl, v[b:]])
    row = row.copy()
    row[long_at + 1:] += n_long - (b - a)
    t_end = t_end.copy()
    t_end[long_at] = int(tl[-1]) + dt
    return row, t, v, t_end, fx


def indicator(batch, seed):
    """an indicator per point of a batch, by series k % 10: no ice, ice from point 0 (the predecessor, all
    ice-free, ends without ice), all ice, runs of 1 / 63 / 64 / 65 points, NaN just before a run and inside one, +-inf, exactly
    0.5 among ice, random with about 20 % NaN, one run longer than two scan spans where the series is long enough"""
    row = batch[0]
    rng = np.random.default_rng(seed)
    ice = np.zeros(int(row[-1]))
    for s in range(len(row) - 1):
        a, b = int(row[s]), int(row[s + 1])
        n = b - a
        x = np.zeros(n)
        h = s % 10
        if h == 1:  # ice from point 0; series k - 1 has none, so its last point is the nearest one without ice
            x[:max(1, n // 2)] = 1.0
        elif h == 2:
            x[:] = 1.0
        elif h == 3:
            for start, length in ((1, 1), (4, 63), (70, 64), (140, 65)):
                x[start:start + length] = 1.0
        elif h == 4 and n > 4:
            x[2:] = 1.0
            x[1] = np.nan          # just before the run
            x[n // 2 + 1] = np.nan  # inside it
        elif h == 5:
            x[:] = 1.0
            x[rng.random(n) < 0.2] = np.inf
            x[rng.random(n) < 0.2] = -np.inf
        elif h == 6:
            x[:] = 1.0
            x[rng.random(n) < 0.3] = 0.5
        elif h == 7:
            x = rng.choice([0.0, 1.0, 0.6, 0.4], n)
            x[rng.random(n) < 0.2] = np.nan
        elif h == 8 and n > 10:
            x[3:n - 2] = 1.0  # one run over nearly the whole series
        elif h == 9:
            x = rng.choice([0.0, 1.0], n, p=[0.1, 0.9])
        ice[a:b] = x[:n]
    return ice
