"""Batches for shyft_hip_forecast_skill: a pool of forecasts and observations in the CSR form of
tests/resample_cases.py, and the problem arrays over it.

The forecasts come in groups of 8 from resample_cases.make_batch (min_points=1; 1, 2, 3, 63, 64, 65 and 257 points,
evenly spaced and irregular, both point types, all eight value hazards); group g starts 6 steps after group g - 1,
as forecasts issued every 6 steps do. The observations follow in the same pool: without points, with 2 points 8 steps
apart, with 65 (the slices run past its end), with 1000 (irregular, about 20 % NaN), and one of 300 points that starts
20 steps late (slices before its start); stair-case and linear alternate among them; one-point observations are left
to the refusal tests. Problem p takes F_p forecasts drawn from the whole pool (so
problems share forecasts, and one may hold a forecast twice) against observation (p + 3) % 6, where 5 stands for
none (obs_ix == -1) and problem 0 so gets the longest, over n_p slices with F_p * n_p = the job count asked for, and
has a t0_offset and dt of its own: dt equal to, twice, a quarter of and not commensurate with the spacing, offsets of
nothing, a quarter step, a step, 5 steps and a tick, and 70 steps (past the end of all but the longest forecast)."""
import numpy as np

from tests import resample_cases as rc

FC_LENGTHS = (1, 2, 3, 63, 64, 65, 257)
FC_GROUP = 8  # one series per value hazard of make_batch
N_OBS = 5
JOBS = (1, 2, 63, 64, 65, 129, 1000)
# F x n with F * n == jobs, both orders are used
FACTORS = {1: (1, 1), 2: (1, 2), 63: (7, 9), 64: (8, 8), 65: (5, 13), 129: (3, 43), 1000: (25, 40)}


def concat(batches):
    """one CSR batch of several"""
    row = [np.zeros(1, np.int64)]
    for b in batches:
        row.append(b[0][1:] + row[-1][-1])
    return (np.concatenate(row), np.concatenate([b[1] for b in batches]), np.concatenate([b[2] for b in batches]),
            np.concatenate([b[3] for b in batches]), np.concatenate([b[4] for b in batches]))


def pick(batch, ids):
    """the batch of the series `ids` of a batch, in that order"""
    row, t, v, t_end, fx = batch
    return concat([(np.asarray([0, row[s + 1] - row[s]], np.int64), t[row[s]:row[s + 1]], v[row[s]:row[s + 1]],
                    t_end[s:s + 1], fx[s:s + 1]) for s in ids])


def make_pool(groups, t0, dt, seed):
    """(batch, n_forecasts, n_observations): 8 * groups forecasts, then 5 observations"""
    parts = [rc.make_batch(FC_GROUP, t0 + 6 * g * dt, dt, seed + g, lengths=FC_LENGTHS, first=g, min_points=1)
             for g in range(groups)]
    parts.append(rc.make_batch(1, t0, dt, seed + 1000, lengths=(0,)))
    parts.append(rc.make_batch(1, t0 + 2 * dt, 8 * dt, seed + 1001, lengths=(2,)))
    parts.append(rc.make_batch(2, t0 - 3 * dt, dt, seed + 1002, lengths=(65, 1000)))
    parts.append(rc.make_batch(1, t0 + 20 * dt, dt, seed + 1003, lengths=(300,)))
    batch = concat(parts)
    batch[4][-N_OBS:] = (1, 1, 0, 1, 0)
    return batch, FC_GROUP * groups, N_OBS


def make_problems(P, jobs_of, n_fc, n_obs, dt, seed):
    """(fc_row, fc_ix, obs_ix, t0_offset, dt, n) of P problems; jobs_of(p) is the job count of problem p"""
    rng = np.random.default_rng(seed)
    dts = (dt, 2 * dt, dt // 4, (7 * dt) // 5 + 1)
    offsets = (0, dt // 4, dt, 5 * dt + 1, 70 * dt)
    fc_row, fc_ix, obs_ix, off, pdt, pn = [0], [], [], [], [], []
    for p in range(P):
        F, n = FACTORS[jobs_of(p)]
        if p % 2:
            F, n = n, F
        fc_ix.extend(rng.integers(0, n_fc, F).tolist())
        fc_row.append(len(fc_ix))
        o = (p + 3) % (n_obs + 1)
        obs_ix.append(n_fc + o if o < n_obs else -1)
        off.append(offsets[(p + p // 5) % len(offsets)])
        pdt.append(dts[(p + p // 4) % len(dts)])
        pn.append(n)
    as64 = lambda x: np.asarray(x, np.int64)  # noqa: E731
    return as64(fc_row), as64(fc_ix), as64(obs_ix), as64(off), as64(pdt), as64(pn)


def make_case(P, first_jobs, epoch, seed, groups=3):
    """(batch, problems) with problem p of JOBS[(JOBS.index(first_jobs) + p) % 7] jobs on time base rc.EPOCHS[epoch]"""
    t0, dt = rc.EPOCHS[epoch]
    batch, n_fc, n_obs = make_pool(groups, t0, dt, seed)
    j0 = JOBS.index(first_jobs)
    return batch, make_problems(P, lambda p: JOBS[(j0 + p) % len(JOBS)], n_fc, n_obs, dt, seed + 1)
