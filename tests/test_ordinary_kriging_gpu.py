"""Ordinary kriging on the GPU: shyft_hip_ordinary_kriging is bit-identical to shyft_hip_ordinary_kriging_host
(same chain order, explicit FMA, detmath::exp), over the shapes at which the product kernel's tiling can go wrong;
then the second act of shyft/tests/api/test_interpolation.py:178-187 and two kriging properties.

The product kernel holds 16 rows per lane, 8 row tiles and 64 destinations per workgroup and stages k in panels of
32: n in {2, 3, 5, 33, 65, 130} gives K = n and n + 1 across panel remainders and one or two workgroup rows, m in
{1, 63, 64, 65, 257, 1000} a partial wave, a wave boundary and several workgroups, T in {1, 3, 17, 50} row-tile
remainders, dst_block in {64, 100} blocks that are not a multiple of a wave and a last short block."""
import numpy as np
import pytest

from tests import ok_cases
from tests.ok_cases import EXPONENTIAL, GAUSSIAN

pytestmark = pytest.mark.gpu

NS, MS, TS = (2, 3, 5, 33, 65, 130), (1, 63, 64, 65, 257, 1000), (1, 3, 17, 50)


def _sampled_cases():
    """every value of each axis, both covariance types, the corners, and dst_block at m = 257 and m = 1000"""
    cases = [(2, 1, 1, EXPONENTIAL, 0), (130, 1000, 50, GAUSSIAN, 0), (130, 1000, 50, EXPONENTIAL, 0)]
    for i, n in enumerate(NS):
        for j, m in enumerate(MS):
            if (i + j) % 2 == 0:  # a checkerboard of n x m, T and the covariance cycling through it
                cases.append((n, m, TS[(i + 2 * j) % 4], (GAUSSIAN, EXPONENTIAL)[(i + j // 2) % 2], 0))
    for k, (m, blk) in enumerate([(257, 64), (257, 100), (1000, 64), (1000, 100)]):
        cases.append((NS[k + 2], m, TS[k], (GAUSSIAN, EXPONENTIAL)[k % 2], blk))
        cases.append((NS[(k + 5) % 6], m, TS[(k + 2) % 4], (EXPONENTIAL, GAUSSIAN)[k % 2], blk))
    for t in TS:  # every T at the K = 33 panel remainder
        cases.append((33, 65, t, EXPONENTIAL, 0))
    cases += [(65, 63, 3, EXPONENTIAL, 0), (65, 65, 50, GAUSSIAN, 0), (130, 64, 3, GAUSSIAN, 0), (3, 257, 17, GAUSSIAN, 0),
              (5, 63, 3, EXPONENTIAL, 0), (2, 1000, 17, GAUSSIAN, 0), (33, 64, 50, GAUSSIAN, 0),
              (65, 1000, 50, EXPONENTIAL, 0)]
    assert {c[0] for c in cases} == set(NS) and {c[1] for c in cases} == set(MS) and {c[2] for c in cases} == set(TS)
    return sorted(set(cases))


def _param(cov_type, n):
    # the range the host tests pair with this covariance and n (a well-conditioned system)
    return (1.0, 10000.0 if cov_type == EXPONENTIAL else (2000.0 if n > 65 else 3000.0), 1.0, cov_type)


@pytest.mark.parametrize("n,m,T,cov_type,dst_block", _sampled_cases())
def test_device_is_bit_identical_to_host(n, m, T, cov_type, dst_block):
    from shyft_amd import region
    src, obs, dst = ok_cases.case(n, m, T)
    if T > 2:
        obs[1, n // 2] = np.nan  # a NaN observation: its whole step is NaN on both sides
    param = _param(cov_type, n)
    host = region.ordinary_kriging(src, obs, param, dst, host=True)
    dev = region.ordinary_kriging(src, obs, param, dst, dst_block=dst_block)
    assert dev.shape == (T, m)
    if T > 2:
        assert np.isnan(dev[1]).all() and np.isfinite(np.delete(dev, 1, 0)).all()
    assert np.array_equal(dev, host, equal_nan=True)


def test_layout_with_asymmetric_data():
    from shyft_amd import region
    n, m, T = 33, 257, 17
    src, _, dst = ok_cases.case(n, m, T)
    src[:, 2] = 10.0 + 30.0 * np.arange(n)  # distinct source heights
    obs = 1000.0 * np.arange(T)[:, None] + np.arange(n)[None, :]
    param = _param(EXPONENTIAL, n)
    host = region.ordinary_kriging(src, obs, param, dst, host=True)
    dev = region.ordinary_kriging(src, obs, param, dst)
    assert np.array_equal(dev, host)
    swapped = src.copy()
    swapped[[4, 20]] = swapped[[20, 4]]
    other = region.ordinary_kriging(swapped, obs, param, dst)
    assert not np.array_equal(dev, other)
    assert np.array_equal(other, region.ordinary_kriging(swapped, obs, param, dst, host=True))


def test_three_sites_onto_the_grid_through_the_api():
    from shyft_amd import api
    from tests.test_ordinary_kriging import _axes, _grid, _site
    ta_obs, ta_grid = _axes(api)
    p = api.OKParameter(c=1.0, a=10.0 * 1000.0, cov_type=api.OKCovarianceType.EXPONENTIAL, z_scale=1.0)
    series = [_site(api, ta_obs, 1.0, 0.1), _site(api, ta_obs, 0.8, 0.2), _site(api, ta_obs, 1.2, 0.1)]
    where = [(50.0, 50.0, 5.0), (9000.0, 500.0, 500.0), (9000.0, 12000.0, 1050.0)]
    sites = api.GeoPointSourceVector()
    for xyz, ts in zip(where, series):
        sites.append(api.GeoPointSource(api.GeoPoint(*xyz), ts))
    p.cov_type = api.OKCovarianceType.GAUSSIAN
    grid = _grid(api, 5, 5, 1000)
    r = api.ordinary_kriging(sites, grid, ta_grid, p)
    assert len(r) == 25
    one_site = series[0].average(ta_grid).values.to_numpy()
    got = np.stack([gts.ts.values.to_numpy() for gts in r], 1)
    for gts in r:
        assert gts.ts.size() == ta_grid.size()
        assert not np.allclose(one_site, gts.ts.values.to_numpy())
    obs = np.stack([ts.average(ta_grid).values.to_numpy() for ts in series], 1)
    dst = np.array([[g.x, g.y, g.z] for g in grid])
    expected, cond = ok_cases.numpy_kriging(np.array(where), obs, (1.0, 10000.0, 1.0, GAUSSIAN), dst)
    assert cond <= 1e3, cond
    assert np.max(np.abs(got - expected)) <= 1e-9


def test_kriging_properties():
    from shyft_amd import region
    n, T = 33, 17
    src, obs, dst = ok_cases.case(n, 65, T)
    param = _param(EXPONENTIAL, n)
    assert np.linalg.cond(ok_cases.system(src, *param)) <= 1e3
    dst[5] = src[11]  # a destination on a source reproduces that source's series
    got = region.ordinary_kriging(src, obs, param, dst)
    assert np.max(np.abs(got[:, 5] - obs[:, 11])) <= 1e-9
    flat = region.ordinary_kriging(src, np.full((T, n), 7.25), param, dst)  # the weights sum to 1
    assert np.max(np.abs(flat - 7.25)) <= 1e-9
