"""Plain restatements of the reductions in kernels/stats.hip and of kernels/routing.hip, with the planted inputs and
the size classes the edge tests share (tests/test_stats_edges.py, tests/test_routing_edges.py, tests/test_segment_sums.py).
Nothing here touches the device: the restatements are numpy / Python floats in the kernels' order of additions, the exact
references are math.fsum over exact products and fractions.Fraction.

The library is built with -ffp-contract=off, so every product is rounded before it is added: no fma anywhere below."""
import math
from fractions import Fraction

import numpy as np

RB = 256    # threads of a reduction workgroup: 4 wavefronts of 64
U = 2.0 ** -53  # unit roundoff of fp64

# Segment sizes at which the lane stride (256), the wavefront butterfly (64) and the four-loads-ahead condition
# (k + 3*256 < e: first true for lane 0 at 769 cells, a second trip at 1793) change behaviour.
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 768, 769, 1023, 1024, 1025, 2049]
# catchment ids, deliberately unsorted: catchment k of the contiguous layout has SIZES[k] cells
CIDS = [42, 7, 11, 3, 99, 5, 64, 1, 77, 23, 8, 150, 2, 31]
N_CELLS = sum(SIZES)
LAYOUTS = ("contiguous", "permuted")


def device_order_sum(vals, w=None):
    """The segment-sum kernel's reduction of one segment's values (in segment order); with w, of the rounded products
    vals[k] * w[k]. vals is [n] or [..., n] (the leading axes are reduced independently, e.g. steps)."""
    v = np.asarray(vals, dtype=np.float64)
    if w is not None:
        v = v * np.asarray(w, dtype=np.float64)  # each product rounded to fp64 before any add
    lead, n = v.shape[:-1], v.shape[-1]
    v = v.reshape(-1, n)
    acc = np.zeros((v.shape[0], RB))
    for k in range(0, n, RB):  # lane l adds its terms k = l, l + 256, ... in order
        m = min(RB, n - k)
        acc[:, :m] += v[:, k:k + m]
    x = acc.reshape(-1, RB // 64, 64)
    lanes = np.arange(64)
    with np.errstate(invalid="ignore"):  # inf - inf is NaN on the device too, without a warning
        off = 32
        while off:  # the xor butterfly, offsets 32, 16, ..., 1
            x = x + x[:, :, lanes ^ off]
            off >>= 1
        part = x[:, :, 0]
        r = part[:, 0]
        for p in range(1, RB // 64):  # the wavefront partials in order
            r = r + part[:, p]
    return r.reshape(lead) if lead else r[0]


def select_order_sum(row, ids=None, areas=None):
    """select_sum_kernel on one or more series rows [..., n_cells]: the selection is the cells named by ids in cell
    order, each once (ids None or empty: every cell); with areas [n_cells], each value times its own cell's area,
    rounded, then the same lanes and tree as the segment kernel."""
    row = np.asarray(row, dtype=np.float64)
    n = row.shape[-1]
    sel = np.arange(n) if ids is None or len(ids) == 0 else np.unique(np.asarray(ids, dtype=np.int64))
    sel = sel[sel < n]
    if sel.size == 0:
        return np.zeros(row.shape[:-1])
    return device_order_sum(row[..., sel], None if areas is None else np.asarray(areas)[sel])


def sequential_sum(vals):
    """vals added left to right from 0.0, as the reference adds cell after cell."""
    r = 0.0
    for v in np.asarray(vals, dtype=np.float64).tolist():
        r += v
    return r


def exact_sum(vals, w=None):
    """(the exact sum correctly rounded, the exact sum of |terms| rounded): of vals, or of the exact products."""
    if w is None:
        terms = [float(v) for v in vals]
        return math.fsum(terms), math.fsum(abs(t) for t in terms)
    s = sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(vals, w)), Fraction(0))
    sa = sum((abs(Fraction(float(a)) * Fraction(float(b))) for a, b in zip(vals, w)), Fraction(0))
    return float(s), float(sa)


def planted(T, n, seed):
    """[T][n] values +-2^e (1 + r), e uniform in -20..20 and r in [0, 1): 40 binades of cancellation, so that the sum
    depends on the order in which it is taken."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-20, 21, (T, n))
    r = rng.random((T, n))
    s = np.where(rng.random((T, n)) < 0.5, -1.0, 1.0)
    return s * np.ldexp(1.0 + r, e)


def planted_areas(n, seed=77):
    return np.random.default_rng(seed).uniform(0.5e6, 2e6, n)


def layout(kind):
    """The catchment id of each of the N_CELLS cells. "contiguous": catchment CIDS[k] is SIZES[k] consecutive cells, in
    cell order, so the segments are the identity permutation; "permuted": the same cells dealt through a fixed
    permutation, the indexed path (every catchment keeps its size)."""
    cid = np.repeat(np.asarray(CIDS, dtype=np.int64), SIZES)
    if kind == "contiguous":
        return cid
    assert kind == "permuted"
    return cid[np.random.default_rng(20).permutation(N_CELLS)]


def size_of_cid(c):
    return SIZES[CIDS.index(int(c))]


# ---------------------------------------------------------------- routing

def levels_first(down):
    """river indices, every river after all of its upstream rivers"""
    R = len(down)
    ups = [[u for u in range(R) if down[u] == r] for r in range(R)]  # ascending
    done, order = [False] * R, []
    while len(order) < R:
        progressed = False
        for r in range(R):
            if not done[r] and all(done[u] for u in ups[r]):
                done[r] = True
                order.append(r)
                progressed = True
        assert progressed, "cycle"
    return ups, order


def route_restated(group_sums, group_uhgs, group_river, river_uhgs, river_downstream):
    """kernels/routing.hip in Python floats, in the kernels' order: per river its groups ascending, per group a subtotal
    over the taps j ascending with j <= t and then acc += subtotal; the upstream rivers ascending from 0.0;
    inflow = local + up; output over the taps ascending. Returns (local, upstream, output), each [R][T]."""
    S = [[float(x) for x in row] for row in np.asarray(group_sums, dtype=np.float64).reshape(len(group_uhgs), -1)]
    T = len(S[0]) if S else np.asarray(group_sums).shape[-1]
    R = len(river_uhgs)
    gw = [[float(x) for x in w] for w in group_uhgs]
    rw = [[float(x) for x in w] for w in river_uhgs]
    ups, order = levels_first([int(d) for d in river_downstream])
    local = [[0.0] * T for _ in range(R)]
    up = [[0.0] * T for _ in range(R)]
    out = [[0.0] * T for _ in range(R)]
    for r in range(R):
        for t in range(T):
            acc = 0.0
            for g in range(len(gw)):
                if int(group_river[g]) != r:
                    continue
                v = 0.0
                for j in range(len(gw[g])):
                    v += gw[g][j] * S[g][t - j] if j <= t else 0.0
                acc += v
            local[r][t] = acc
    for r in order:
        inflow = [0.0] * T
        for t in range(T):
            a = 0.0
            for u in ups[r]:
                a += out[u][t]
            up[r][t] = a
            inflow[t] = local[r][t] + a
        for t in range(T):
            v = 0.0
            for j in range(len(rw[r])):
                v += rw[r][j] * inflow[t - j] if j <= t else 0.0
            out[r][t] = v
    return np.array(local).reshape(R, T), np.array(up).reshape(R, T), np.array(out).reshape(R, T)


def route_exact(group_sums, group_uhgs, group_river, river_uhgs, river_downstream):
    """The same network in exact rational arithmetic. Returns ((local, upstream, output), (a_local, a_upstream,
    a_output)): the exact values rounded once to fp64, and for each the exact sum of the absolute values of its
    elementary terms (products of UHG weights along the path times one group sum), the scale of its error bound."""
    G = len(group_uhgs)
    S = [[Fraction(float(x)) for x in row] for row in np.asarray(group_sums, dtype=np.float64).reshape(G, -1)]
    T = len(S[0]) if S else np.asarray(group_sums).shape[-1]
    R = len(river_uhgs)
    gw = [[Fraction(float(x)) for x in w] for w in group_uhgs]
    rw = [[Fraction(float(x)) for x in w] for w in river_uhgs]
    ups, order = levels_first([int(d) for d in river_downstream])
    Z = Fraction(0)
    val = {k: [[Z] * T for _ in range(R)] for k in ("local", "up", "out")}
    mag = {k: [[Z] * T for _ in range(R)] for k in ("local", "up", "out")}
    for r in range(R):
        for g in range(G):
            if int(group_river[g]) != r:
                continue
            for t in range(T):
                for j in range(min(len(gw[g]), t + 1)):
                    p = gw[g][j] * S[g][t - j]
                    val["local"][r][t] += p
                    mag["local"][r][t] += abs(p)
    for r in order:
        for t in range(T):
            val["up"][r][t] = sum((val["out"][u][t] for u in ups[r]), Z)
            mag["up"][r][t] = sum((mag["out"][u][t] for u in ups[r]), Z)
        vin = [val["local"][r][t] + val["up"][r][t] for t in range(T)]
        min_ = [mag["local"][r][t] + mag["up"][r][t] for t in range(T)]
        for t in range(T):
            for j in range(min(len(rw[r]), t + 1)):
                val["out"][r][t] += rw[r][j] * vin[t - j]
                mag["out"][r][t] += abs(rw[r][j]) * min_[t - j]
    f = lambda m: np.array([[float(x) for x in row] for row in m]).reshape(R, T)  # noqa: E731
    return tuple(f(val[k]) for k in ("local", "up", "out")), tuple(f(mag[k]) for k in ("local", "up", "out"))


def route_term_counts(group_uhgs, group_river, river_uhgs, river_downstream):
    """[R] of L_max + G_r + U_r + 2: the taps of the longest UHG in the call, the river's groups, its upstream rivers,
    and two (see tests/test_routing_edges.py for the derivation)."""
    R = len(river_uhgs)
    l_max = max([1] + [len(w) for w in group_uhgs] + [len(w) for w in river_uhgs])
    return np.array([l_max + sum(1 for g in group_river if int(g) == r) +
                     sum(1 for d in river_downstream if int(d) == r) + 2 for r in range(R)])
