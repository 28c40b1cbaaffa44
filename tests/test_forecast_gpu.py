"""The forecast-skill kernel on the GPU: ns, sim and obs of shyft_hip_forecast_skill are bit-identical to
shyft_hip_forecast_skill_host (host/forecast.hpp on one thread) over the shapes at which kernels/forecast.hip can go
wrong.

A wavefront takes a problem and its jobs 64 at a time, so the job counts F * n in {1, 2, 63, 64, 65, 129, 1000} lie
on both sides of the chunk boundary and P in {1, 63, 64, 65, 257} on both sides of a workgroup of 4 problems and of 64;
every pair of the two meets, the leading problem of a batch having the job count named and the others rotating
through the rest, and the three time bases (2016, negative, above 2^53 us with an odd spacing) rotate over them. The
batches are those of tests/forecast_cases.py: forecasts of 1, 2, 3, 63, 64, 65 and 257 points, both point types,
evenly spaced and irregular, the value hazards of resample_cases.make_batch; dt equal to, twice, a quarter of and not
commensurate with the spacing; slices that run past a forecast's end, past the observation's end and before its start;
observations of 0 and of 2 points and obs_ix == -1; t0_offset, dt and n that differ from problem to problem; problems
that share forecasts."""
import numpy as np
import pytest

from tests import forecast_cases as fcs
from tests import resample_cases as rc

pytestmark = pytest.mark.gpu

PS = (1, 63, 64, 65, 257)


def _cases():
    cases = [(P, jobs, (i + 2 * k) % len(rc.EPOCHS)) for k, P in enumerate(PS) for i, jobs in enumerate(fcs.JOBS)]
    assert {c[2] for c in cases} == {0, 1, 2}
    return cases


@pytest.fixture(scope="module")
def region():
    from shyft_amd import region
    return region


def _assert_same(dev, host, what):
    for name, d, h in zip(("ns", "sim", "obs"), dev, host):
        bad = np.argwhere(~((np.isnan(d) & np.isnan(h)) | (d.view(np.uint64) == h.view(np.uint64))))
        assert rc.same_bits(d, h), (what, name, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("P,jobs,epoch", _cases())
def test_device_is_bit_identical_to_host(region, P, jobs, epoch):
    batch, prob = fcs.make_case(P, jobs, epoch, 9000 + 10 * P + fcs.JOBS.index(jobs))
    fc_row, n = prob[0], prob[5]
    assert fc_row[1] * n[0] == jobs
    host = region.forecast_skill_csr(*batch, *prob, host=True, slices=True)
    dev = region.forecast_skill_csr(*batch, *prob, slices=True)
    assert host[0].shape == (P,) and host[1].shape == host[2].shape == (int(np.sum(np.diff(fc_row) * n)),)
    _assert_same(dev, host, (P, jobs, epoch))
    # the score alone, without the slices downloaded
    assert rc.same_bits(region.forecast_skill_csr(*batch, *prob), host[0])
    if P >= 63:  # the batch reaches finite scores, NaN scores and both kinds of slices
        assert np.isfinite(host[0]).any() and np.isnan(host[0]).any()
        assert np.isfinite(host[1]).any() and np.isnan(host[1]).any() and np.isfinite(host[2]).any()


def test_a_lead_time_table_shares_the_forecasts_of_a_location(region):
    """3 locations x 40 lead times: every row of a location lists the same 16 forecasts and the same observation"""
    t0, dt = rc.EPOCHS[0]
    batch, n_fc, n_obs = fcs.make_pool(6, t0, dt, 77)
    fc_row, fc_ix, obs_ix, off = [0], [], [], []
    for loc in range(3):
        for lead in range(40):
            fc_ix.extend(range(16 * loc, 16 * loc + 16))
            fc_row.append(len(fc_ix))
            obs_ix.append(n_fc + (3, 2, 4)[loc])
            off.append(lead * dt)
    prob = (fc_row, fc_ix, obs_ix, off, dt, 6)
    host = region.forecast_skill_csr(*batch, *prob, host=True, slices=True)
    dev = region.forecast_skill_csr(*batch, *prob, slices=True)
    _assert_same(dev, host, "table")
    assert np.isfinite(host[0]).sum() > 60


def test_calls_count_device_launches_only(region):
    from shyft_amd._native import ShyftHipError
    batch, prob = fcs.make_case(5, 65, 0, 11)
    n0 = region.forecast_skill_calls()
    region.forecast_skill_csr(*batch, *prob)
    assert region.forecast_skill_calls() == n0 + 1
    assert region.forecast_skill_last_ms() > 0.0
    region.forecast_skill_csr(*batch, *prob, slices=True)
    assert region.forecast_skill_calls() == n0 + 2
    region.forecast_skill_csr(*batch, *prob, host=True)
    region.forecast_skill_csr(*batch, [0], [], [], 0, rc.HOUR, 6)                    # P == 0 launches nothing
    ns = region.forecast_skill_csr(*batch, *prob[:5], 0)                             # J == 0 by n == 0
    assert np.isnan(ns).all() and ns.shape == (5,)
    ns = region.forecast_skill_csr(*batch, [0, 0, 0], [], [3, -1], 0, rc.HOUR, 6)    # J == 0 by no forecasts
    assert np.isnan(ns).all() and ns.shape == (2,)
    with pytest.raises(ShyftHipError, match="dt, average interval, must be specified as > 0 s"):
        region.forecast_skill_csr(*batch, *prob[:4], 0, prob[5])
    assert region.forecast_skill_calls() == n0 + 2


def test_a_problem_without_jobs_among_others(region):
    batch, prob = fcs.make_case(9, 129, 1, 12)
    fc_row, fc_ix, obs_ix, off, dt, n = prob
    n = n.copy()
    n[2] = 0                                              # no slices
    fc_row = np.concatenate([fc_row, fc_row[-1:]])        # and a last problem without forecasts
    prob = (fc_row, fc_ix, np.append(obs_ix, obs_ix[0]), np.append(off, 0), np.append(dt, dt[0]), np.append(n, 4))
    host = region.forecast_skill_csr(*batch, *prob, host=True, slices=True)
    dev = region.forecast_skill_csr(*batch, *prob, slices=True)
    _assert_same(dev, host, "empty problems")
    assert np.isnan(dev[0][2]) and np.isnan(dev[0][-1]) and np.isfinite(dev[0]).any()
