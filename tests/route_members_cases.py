"""Shared inputs of the ensemble-routing tests (test_route_members_host.py, test_ensemble_routing_gpu.py)."""
import numpy as np

from tests.test_routing import RIVERS

HOUR_S = 3600.0
DISTANCES = (0.0, 1500.0, 5000.0, 12000.0)
RIVER_DOWN = [ds - 1 for (_, ds, *_rest) in RIVERS]  # river indices in ascending id, -1 = none


def river_uhgs():
    from shyft_amd import api
    return [api.make_uhg_from_gamma(int((d / v) / HOUR_S + 0.5), a, b) for (_, _, d, v, a, b) in RIVERS]


def random_case(counts, T, lengths, seed, n_rivers=4, river_lengths=None):
    """Members with counts[m] groups each over a chain-and-branch network of n_rivers rivers (RIVER_DOWN's shape):
    random UHG weights and group sums with negative values and exact zeros, the group lengths cycling through
    `lengths`, rivers drawn at random. Returns the arguments of region.route_members."""
    rng = np.random.default_rng(seed)
    G = int(sum(counts))
    row = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    sums = rng.normal(0.0, 3.0, (G, T))
    sums[rng.random((G, T)) < 0.1] = 0.0
    uhgs = []
    for g in range(G):
        w = rng.normal(0.0, 1.0, lengths[g % len(lengths)])
        w[rng.random(w.size) < 0.1] = 0.0
        uhgs.append(w)
    river = rng.integers(0, n_rivers, G).astype(np.int32)
    rl = river_lengths or [3, 1, 2, 5]
    ruhgs = []
    for r in range(n_rivers):
        w = rng.normal(0.0, 1.0, rl[r % len(rl)])
        ruhgs.append(w)
    down = RIVER_DOWN[:n_rivers]
    return row, sums, uhgs, river, ruhgs, down


def member_slice(case, m):
    """The arguments of one member of `case` as a one-member call."""
    row, sums, uhgs, river, ruhgs, down = case
    b, e = int(row[m]), int(row[m + 1])
    return np.array([0, e - b], np.int64), sums[b:e], uhgs[b:e], river[b:e], ruhgs, down
