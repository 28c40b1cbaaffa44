"""Inputs of the inverse-distance edge tests (tests/test_idw_edges.py), shared by the CPU and the GPU tests.

Edge geometry (S = 49, N = 333): stations on a 7 x 7 lattice 1000 m apart, z = 100 on the even lattice rows (exact
distance and elevation ties), random on the odd rows; cells 500 m apart in rows of 19, so many sit on a station or
midway between 2 or 4 of them, every third cell at z = 100, and the last 20 cells 1000 km away (no candidate at all).
333 cells are 5 wavefronts + 13 lanes and 1 workgroup + 77 lanes. 49 stations fit every wavefront's union, so the
wavefront-union gather runs; SHYFT_IDW_TILE=1 takes the LDS row tiles.

Two parameter sets: "near" (max_distance 2500 m: 0..22 candidates per cell, counts below, at and above every
max_members up to 21, weight ties at the cut, stations exactly at max_distance) and "far" (100 km: every cell in range
has all 49 candidates, so the cells of wavefronts 0-3 hold exactly max_members neighbours for every max_members;
wavefront 4 is mixed and wavefront 5 has no neighbour at all).

Large station set (S = 4100): the same cells inside a 64 x 65 lattice with the same spacing and elevation rule, so the
same kinds of counts; 8 x 4100 B exceed the 32 KB row-tile budget, so the tile gather reads its rows from global memory.
"""
import functools

import numpy as np

from tests import oracle_lib

# name, forcing variable (region), oracle kind, gradient_by_equation
MODELS = {
    "temperature": (0, 0, False),
    "temperature_eq": (0, 0, True),
    "precipitation": (1, 1, False),
    "wind_speed": (2, 3, False),
    "rel_hum": (3, 4, False),
    "radiation": (4, 2, False),
}
K_VALUES = (1, 7, 8, 9, 12, 13, 20, 21, 32)     # both sides of every register tier (8, 12, 20, 32) and the tiers
PARAM_SETS = {"near": (2500.0, 2.0, 1.0), "far": (1.0e5, 1.5, 0.5)}   # max_distance, distance_measure_factor, zscale
DEFAULT_GRADIENT = -0.006
SCALE_FACTOR = 1.02

N_CELLS = 333
N_FAR_CELLS = 20            # the last cells, out of every station's reach
T_ROWS = 67                 # two LDS tiles of 64 + 3 rows, and an odd count for the temperature row pairs
ROW_SOME_NAN, ROW_ALL_NAN, ROW_INF, ROW_HUGE, ROW_SOME_NAN_2, ROW_ALL_NAN_2 = 1, 3, 5, 63, 64, 66
HUGE = 1.0e300
HUGE_STATION, NEAR_PLANE_STATION = 17, 24   # lattice (row 2, column 3) and its neighbour (row 3, column 3)


def param(pset, K, by_equation=False, default_gradient=DEFAULT_GRADIENT):
    max_distance, factor, zscale = PARAM_SETS[pset]
    return [K, max_distance, factor, zscale, default_gradient, 1.0 if by_equation else 0.0, SCALE_FACTOR]


def _lattice(nx, ny, x0, y0, n, rng):
    s = np.arange(n)
    col, row = s % nx, s // nx
    assert row.max() < ny
    z = np.where(row % 2 == 0, 100.0, rng.uniform(0.0, 1500.0, n))
    return np.stack([x0 + 1000.0 * col, y0 + 1000.0 * row, z], 1)


@functools.lru_cache(maxsize=None)
def cells():
    """geo11 rows of the 333 cells: x, y, z, area, catchment id, radiation slope factor, land type fractions."""
    rng = np.random.default_rng(71)
    i = np.arange(N_CELLS)
    geo = np.zeros((N_CELLS, 11))
    geo[:, 0] = 500.0 * (i % 19)
    geo[:, 1] = 500.0 * (i // 19)
    geo[:, 2] = np.where(i % 3 == 0, 100.0, rng.uniform(0.0, 1500.0, N_CELLS))
    geo[-N_FAR_CELLS:, 0] += 1.0e6
    geo[:, 3] = 1.0e6
    geo[:, 4] = 1 + i % 3
    geo[:, 5] = rng.uniform(0.7, 1.0, N_CELLS)
    geo[:, 6:10] = (0.01, 0.05, 0.19, 0.30)
    geo[:, 10] = 0.45
    geo.setflags(write=False)
    return geo


@functools.lru_cache(maxsize=None)
def stations(which="edge"):
    """[S][3] station coordinates: "edge" (S = 49) or "large" (S = 4100, the cells well inside the lattice)."""
    if which == "edge":
        xyz = _lattice(7, 7, 0.0, 0.0, 49, np.random.default_rng(72))
        # one station of an odd row a hair off the even rows' plane: with three z = 100 stations its 3 x 3 system is
        # nearly singular (inverse entries ~1e10), so the HUGE value overflows the solve and the min/max rule is used
        xyz[NEAR_PLANE_STATION, 2] = 100.0 + 1.0e-9
    else:
        xyz = _lattice(64, 65, -27000.0, -28000.0, 4100, np.random.default_rng(73))
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def rows(which="edge"):
    """[T][S] station values. "edge": 67 rows with the non-finite rows next to the start, the call split, the LDS tile
    boundary (63 | 64) and the end; "large": 5 rows, one with missing values."""
    if which == "edge":
        rng = np.random.default_rng(74)
        v = rng.normal(5.0, 4.0, (T_ROWS, 49))
        for r in (ROW_SOME_NAN, ROW_SOME_NAN_2):
            v[r, rng.uniform(size=49) < 0.2] = np.nan
        v[ROW_ALL_NAN] = np.nan
        v[ROW_ALL_NAN_2] = np.nan
        v[ROW_INF, 10] = np.inf
        v[ROW_INF, 30] = -np.inf
        v[ROW_HUGE, HUGE_STATION] = HUGE
    else:
        rng = np.random.default_rng(75)
        v = rng.normal(5.0, 4.0, (5, 4100))
        v[2, rng.uniform(size=4100) < 0.2] = np.nan
    v.setflags(write=False)
    return v


def oracle(model, prm, xyz, vals, geo):
    """The oracle's run_interpolation of one model -> [T][N]."""
    _, kind, by_equation = MODELS[model]
    assert bool(prm[5]) == by_equation
    return oracle_lib.idw_run(kind, xyz, vals, geo[:, :3], prm, dst_slope=geo[:, 5])


@functools.lru_cache(maxsize=None)
def expected(model, K, pset, which="edge"):
    """The oracle on the shared inputs, computed once per case and read-only."""
    out = oracle(model, param(pset, K, MODELS[model][2]), stations(which), rows(which), cells())
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# A plain numpy restatement of inverse_distance.h:142-330 (as oracle/src/idw.hpp documents it), vectorised over rows and
# cells, sequential over the neighbour slots in the reference's order.

def np_weights(xyz, geo, prm):
    """[N][S] weights min(1, 1 / distance_measure) and the candidate mask weight >= min_weight."""
    _, max_distance, f, zs = prm[:4]
    d = geo[:, None, :3] - xyz[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2] * zs * zs
    with np.errstate(divide="ignore"):
        w = np.minimum(1.0, 1.0 / np.power(d2, f / 2.0))
    min_w = 1.0 / np.power(max_distance * max_distance + 0.0 * 0.0 + 0.0 * 0.0 * zs * zs, f / 2.0)
    return w, w >= min_w


def np_neighbours(xyz, geo, prm, ties_to_lower=True):
    """Per cell the kept sources ([N][K], -1 past the count) and weights: all candidates in source order, or -- more
    than max_members of them -- the max_members largest weights, descending, ties to the lower source index
    (ties_to_lower=False: to the higher one, the other order a partial_sort may leave)."""
    K = int(prm[0])
    w, cand = np_weights(xyz, geo, prm)
    N = geo.shape[0]
    nb = np.full((N, K), -1, dtype=np.int64)
    nw = np.zeros((N, K))
    for j in range(N):
        s = np.flatnonzero(cand[j])
        if s.size > K:
            if not ties_to_lower:
                s = s[::-1]
            s = s[np.argsort(-w[j, s], kind="stable")[:K]]
        nb[j, :s.size] = s
        nw[j, :s.size] = w[j, s]
    return nb, nw


def np_idw(model, prm, xyz, vals, geo, ties_to_lower=True):
    """[T][N] interpolated values; also returns the number of (row, cell) pairs where the 3 x 3 system had a usable
    determinant but a non-finite solution (the fallback to the min/max gradient)."""
    _, kind, by_equation = MODELS[model]
    default_gradient, scale_factor = prm[4], prm[6]
    nb, nw = np_neighbours(xyz, geo, prm, ties_to_lower)
    N, K = nb.shape
    T = vals.shape[0]
    has = nb >= 0
    s = np.where(has, nb, 0)
    sx, sy, sz = xyz[s, 0], xyz[s, 1], xyz[s, 2]                  # [N][K]
    valid = [np.isfinite(vals[:, s[:, k]]) & has[None, :, k] for k in range(K)]   # K x [T][N]
    scale = np.ones((T, N))
    overflowed = 0
    with np.errstate(all="ignore"):
        if kind == 0:
            n = np.zeros((T, N), dtype=np.int64)
            z_mn, z_mx, t_mn, t_mx = (np.zeros((T, N)) for _ in range(4))
            first = [[np.zeros((T, N)) for _ in range(4)] for _ in range(4)]     # x, y, z, value of valid points 0..3
            for k in range(K):
                m, v = valid[k], vals[:, s[:, k]]
                z = np.broadcast_to(sz[:, k], (T, N))
                start = m & (n == 0)
                lower = m & ~start & (z < z_mn)
                higher = m & ~start & ~lower & (z > z_mx)
                z_mn = np.where(start | lower, z, z_mn)
                t_mn = np.where(start | lower, v, t_mn)
                z_mx = np.where(start | higher, z, z_mx)
                t_mx = np.where(start | higher, v, t_mx)
                for q in range(4):
                    here = m & (n == q)
                    for c, col in enumerate((sx[:, k], sy[:, k], sz[:, k], v)):
                        first[q][c] = np.where(here, col, first[q][c])
                n = n + m
            dz = z_mx - z_mn
            scale = np.where(n > 1, np.where(dz > 50.0, (t_mx - t_mn) / dz, default_gradient), default_gradient)
            if by_equation:
                A = [[first[q + 1][c] - first[0][c] for c in range(3)] for q in range(3)]
                b = [first[q + 1][3] - first[0][3] for q in range(3)]
                det = (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]))
                inv = [[(A[1][1] * A[2][2] - A[1][2] * A[2][1]) / det, (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det,
                        (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det],
                       [(A[1][2] * A[2][0] - A[1][0] * A[2][2]) / det, (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det,
                        (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det],
                       [(A[1][0] * A[2][1] - A[1][1] * A[2][0]) / det, (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det,
                        (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det]]
                x = [inv[i][0] * b[0] + inv[i][1] * b[1] + inv[i][2] * b[2] for i in range(3)]
                usable = (n > 3) & (np.abs(det) > 0.0) & np.isfinite(det)
                finite = np.isfinite(x[0]) & np.isfinite(x[1]) & np.isfinite(x[2])
                overflowed = int((usable & ~finite).sum())
                scale = np.where(usable & finite, x[2], scale)
        elif kind == 1:
            scale = np.full((T, N), scale_factor)
        swv, sw = np.zeros((T, N)), np.zeros((T, N))
        for k in range(K):
            v = vals[:, s[:, k]]
            ddz = geo[:, 2] - sz[:, k]
            if kind == 0:
                tr = v + scale * ddz
            elif kind == 1:
                tr = v * np.power(scale, ddz / 100.0)
            elif kind == 2:
                tr = v * geo[:, 5]
            else:
                tr = v
            swv = np.where(valid[k], swv + nw[:, k] * tr, swv)
            sw = np.where(valid[k], sw + nw[:, k], sw)
        return swv / sw, overflowed
