"""Case builders for Bayesian temperature kriging at its edges, shared by the host and the GPU tests of
tests/test_btk_edges.py. Every builder returns (src [S][3], vals [T][S], prior [T], prm [5], dst [D][3]).

A case is admitted (admission(), asserted on the CPU) only if
  conditioning: max |oracle_btk - numpy_btk| < COND, so the oracle's own rounding noise is far below the device
                tolerance and cannot hide a device error, and
  sensitivity : neighbouring destinations and neighbouring steps differ in the oracle by more than SENS, so a
                device index slip of one row or column is about 1000 x TOL.
Random networks keep sources 0 and 1 always valid and at least 500 m apart in height: patterns drawn freely from
all subsets of 8 sources reach 2e-10 between oracle and numpy, because some subsets are nearly level.
"""
import itertools

import numpy as np

from tests.test_btk import TEST_PARAM, numpy_btk, oracle_btk, random_case

COND, SENS = 1e-10, 1e-6
PRM = [0.0025, 25.0, 0.5, 20000.0, 20.0]  # gradient_sd, sill, nugget, range, zscale (as tests/test_btk.py)


def _spread(src, vals):
    """Sources 0 and 1 at 150 m and 1350 m, their temperatures moved along the lapse rate of random_case."""
    for s, z in ((0, 150.0), (1, 1350.0)):
        vals[:, s] -= 0.0065 * (z - src[s, 2])
        src[s, 2] = z
    return src, vals


def network(S, D, T, seed, missing=0.0):
    src, vals, prior, dst = random_case(S=S, D=D, T=T, seed=seed, missing=missing)
    src, vals = _spread(src, vals)
    return src, vals, prior, dst


def admission(case, ref=None, numpy_steps=None):
    """(conditioning, smallest neighbouring-destination difference, smallest neighbouring-step difference) of a
    case; a direction with no neighbours (D == 1, T == 1) gives inf. numpy_steps limits the numpy comparison to
    those steps (numpy_btk is a Python loop over steps, each step on its own): for a long series whose steps all
    share a few patterns and one distribution of values."""
    src, vals, prior, prm, dst = case
    ref = oracle_btk(src, vals, prior, prm, dst) if ref is None else ref
    k = slice(None) if numpy_steps is None else numpy_steps
    cond = float(np.max(np.abs(ref[k] - numpy_btk(src, vals[k], np.asarray(prior)[k], prm, dst))))
    by_dst = float(np.min(np.abs(np.diff(ref, axis=1)))) if ref.shape[1] > 1 else np.inf
    by_step = float(np.min(np.abs(np.diff(ref, axis=0)))) if ref.shape[0] > 1 else np.inf
    return cond, by_dst, by_step


# ---- shapes: destination counts at and around the 256-thread block, source counts at and around a wavefront ------------
SHAPE_D, SHAPE_S, SHAPE_T = (1, 2, 255, 256, 257, 513), (2, 3, 64, 65), (1, 5)
SHAPES = [(D, SHAPE_S[(i + k) % 4], T) for k, T in enumerate(SHAPE_T) for i, D in enumerate(SHAPE_D)]


def shapes(D, S, T):
    src, vals, prior, dst = network(S, D, T, seed=100 + D + S)
    return src, vals, prior, PRM, dst


# ---- patterns: every way the steps of a valid-source pattern can lie in the window ----------------------------------------
def pattern_layout():
    """The missing-source sets of each step (sources 2..7 only; 0 and 1 are always valid)."""
    full, p1, p2, p3, p4 = (), (3,), (4,), (5, 6), (7,)
    used = {p1, p2, p3, p4}
    singles = [c for r in (1, 2, 3) for c in itertools.combinations(range(2, 8), r) if c not in used][:26]
    seq = [full] * 5             # the full set first: direct write at row 0
    seq += [p1] * 8              # one reduced pattern, contiguous: direct write at a row offset
    seq += [p2, p3] * 5          # two patterns step by step: scatter
    seq += [p4] * 2
    seq += singles[:13]          # single-step patterns, all distinct
    seq += [p4] * 2              # p4 returns after a gap
    seq += singles[13:]
    seq += [full] * 3            # the full set again: its steps are no longer contiguous
    return seq


def patterns():
    seq = pattern_layout()
    T = len(seq)
    src, vals, prior, dst = network(8, 65, T, seed=21)
    marks = (np.nan, np.inf, -np.inf)  # every non-finite value is a missing source
    for t, miss in enumerate(seq):
        for s in miss:
            vals[t, s] = marks[(t + s) % 3]
    return src, vals, prior, PRM, dst


def nan_only(case):
    """The same case with every missing value written as NaN."""
    src, vals, prior, prm, dst = case
    v = vals.copy()
    v[~np.isfinite(v)] = np.nan
    return src, v, prior, prm, dst


# ---- coincident: the first S destinations are the sources --------------------------------------------------------------------
def coincident():
    S, T = 8, 10
    src, vals, prior, dst = network(S, S + 20, T, seed=33)
    dst[:S] = src
    vals[4:7, 3] = np.nan
    vals[7:10, 2] = np.nan
    vals[7:10, 5] = np.nan
    return src, vals, prior, PRM, dst


# ---- far: destinations beyond the reach of the covariance, across the underflow of exp ------------------------------------
FAR_AWAY = 8  # destinations of far() at 1e6 m, then the sweep of 257


def far():
    S, T = 6, 6
    rng = np.random.default_rng(44)
    src, vals, prior, _ = network(S, 1, T, seed=44, missing=0.0)
    src[:, :2] = rng.uniform(0, 2000, (S, 2))  # a network of about two ranges across
    vals[2:4, 3] = np.nan
    prm = [0.0025, 25.0, 0.5, 1000.0, 20.0]
    away = np.stack([np.full(FAR_AWAY, 1.0e6), np.linspace(0, 2000, FAR_AWAY), rng.uniform(0, 2000, FAR_AWAY)], 1)
    # distance / range from 690 to 760 along x: exp(-690) is a small normal number, exp(-760) is 0, and between
    # them lies exp's gradual underflow
    sweep = np.stack([np.linspace(690.0e3, 760.0e3, 257), np.full(257, 1000.0), rng.uniform(0, 2000, 257)], 1)
    return src, vals, prior, prm, np.concatenate([away, sweep])


def zscale0():
    src, vals, prior, dst = network(12, 150, 12, seed=55, missing=0.15)
    return src, vals, prior, [0.0025, 25.0, 0.5, 20000.0, 0.0], dst


def kat_range():
    """The reference test's parameter (range 200 km) on a 60 km network: the least well conditioned admitted case."""
    src, vals, prior, dst = network(65, 257, 12, seed=66, missing=0.1)
    return src, vals, prior, TEST_PARAM, dst


def long_alternating():
    """Source 2 missing at odd steps: two patterns of 65537 non-contiguous steps each, more than the 65535 rows one
    scatter launch may place."""
    T = 131074
    src, vals, prior, dst = network(3, 3, T, seed=77)
    vals[1::2, 2] = np.nan
    return src, vals, prior, PRM, dst


BUILDERS = {"patterns": patterns, "coincident": coincident, "far": far, "zscale0": zscale0, "kat_range": kat_range,
            "long_alternating": long_alternating}
BUILDERS.update({f"shapes-D{D}-S{S}-T{T}": (lambda D=D, S=S, T=T: shapes(D, S, T)) for D, S, T in SHAPES})

_ORACLE = {}


def case_and_oracle(name):
    """(case, oracle result) of a builder, computed once and shared; callers do not modify either."""
    if name not in _ORACLE:
        case = BUILDERS[name]()
        ref = oracle_btk(*case)
        ref.setflags(write=False)
        _ORACLE[name] = (case, ref)
    return _ORACLE[name]


# ---- region cases: 600 cells in three catchments of 200, 18 sources, a window of 30 steps ---------------------------------
REGION_N, REGION_T, REGION_W0, REGION_W = 600, 48, 10, 30


def region_geo(dz=0.0):
    rng = np.random.default_rng(4)
    N = REGION_N
    geo = np.zeros((N, 11))
    geo[:, 0] = rng.uniform(0, 60000, N)
    geo[:, 1] = rng.uniform(0, 60000, N)
    geo[:, 2] = rng.uniform(0, 2000, N) + dz
    geo[:, 3] = 1e6
    geo[:, 4] = 1 + np.arange(N) // 200  # catchments 1, 2, 3, contiguous
    geo[:, 5] = 0.9
    geo[:, 6:10] = (0.01, 0.05, 0.19, 0.30)
    geo[:, 10] = 0.45
    return geo


def region_case(layout, seed=11):
    """18 sources over the window's 30 steps. layout 'contiguous': full set, one reduced pattern in a contiguous
    run, full set; 'alternating': the full set and one reduced pattern step by step; 'full': no missing value;
    'reduced': every step misses a source (two patterns), so the full set is factorised but never placed."""
    W = REGION_W
    src, vals, prior, _ = network(18, 1, W, seed=seed)
    if layout == "contiguous":
        vals[10:22, 5] = np.nan
    elif layout == "alternating":
        vals[1::2, 7] = np.nan
        vals[1::2, 9] = np.nan
    elif layout == "reduced":
        vals[:W // 2, 4] = np.nan
        vals[W // 2:, 11] = np.nan
    else:
        assert layout == "full"
    return src, vals, prior, PRM, region_geo()[:, :3]


LEVEL_SOURCE = 2  # cache_case(): the source at z = 0


def cache_case(layout="contiguous", seed=11):
    """region_case with source LEVEL_SOURCE at sea level: a step with that source alone has H^-1 = [[1/c0, 0], [0, 0]],
    singular whatever the rounding, so single_valid() of it raises after the full-set steps before it were placed."""
    src, vals, prior, prm, dst = region_case(layout, seed)
    vals[:, LEVEL_SOURCE] -= 0.0065 * (0.0 - src[LEVEL_SOURCE, 2])
    src[LEVEL_SOURCE, 2] = 0.0
    return src, vals, prior, prm, dst


def single_valid(vals, step, source):
    """vals with `source` the only valid one at `step`."""
    v = vals.copy()
    keep = v[step, source]
    v[step] = np.nan
    v[step, source] = keep
    return v
