"""Ordinary kriging without a device: the host restatement (shyft_hip_ordinary_kriging_host) against numpy, and the
api surface (OKParameter, OKCovarianceType, GeoPointSource, api.ordinary_kriging) on the paths that need no GPU.

Follows api/boostpython/api_interpolation.cpp:73-186 and the first act of
shyft/tests/api/test_interpolation.py:141-176 (one site kriged onto a 5x5 grid).

Tolerance of the numpy comparison, 1e-9: cond(A) eps (n+1) max|obs| <= 1e3 * 2.2e-16 * 131 * 15 = 4.3e-10; every
case asserts cond(A) <= 1e3, so an ill-conditioned draw fails loudly instead of hiding behind the bound."""
import numpy as np
import pytest

from tests import ok_cases
from tests.ok_cases import EXPONENTIAL, GAUSSIAN

HOST_CASES = [(EXPONENTIAL, 10000.0, n) for n in (2, 5, 33, 130)] + \
             [(GAUSSIAN, 3000.0, n) for n in (33, 65)] + [(GAUSSIAN, 2000.0, 130)]


@pytest.mark.parametrize("z_scale", [1.0, 0.0])
@pytest.mark.parametrize("cov_type,a,n", HOST_CASES)
def test_host_restatement_matches_numpy(cov_type, a, n, z_scale):
    from shyft_amd import region
    src, obs, dst = ok_cases.case(n, 70, 8)
    param = (1.0, a, z_scale, cov_type)
    expected, cond = ok_cases.numpy_kriging(src, obs, param, dst)
    assert cond <= 1e3, cond
    got = region.ordinary_kriging(src, obs, param, dst, host=True)
    assert got.shape == (8, 70)
    err = np.max(np.abs(got - expected))
    print(f"n={n} cov={cov_type} a={a} z_scale={z_scale}: cond {cond:.3g}, max |host - numpy| {err:.3g}")
    assert err <= 1e-9


def test_ok_parameter_defaults_fields_and_enum():
    from shyft_amd import api
    assert int(api.OKCovarianceType.GAUSSIAN) == 0 and int(api.OKCovarianceType.EXPONENTIAL) == 1
    assert api.GAUSSIAN == api.OKCovarianceType.GAUSSIAN and api.EXPONENTIAL == api.OKCovarianceType.EXPONENTIAL
    p = api.OKParameter()
    assert (p.c, p.a, p.cov_type, p.z_scale) == (1.0, 10000.0, api.OKCovarianceType.EXPONENTIAL, 1.0)
    p = api.OKParameter(c=2.0, a=500.0, cov_type=api.OKCovarianceType.GAUSSIAN, z_scale=3.0)
    assert (p.c, p.a, p.cov_type, p.z_scale) == (2.0, 500.0, api.OKCovarianceType.GAUSSIAN, 3.0)
    p.c, p.a, p.cov_type, p.z_scale = 4.0, 5.0, api.OKCovarianceType.EXPONENTIAL, 0.0
    assert (p.c, p.a, p.cov_type, p.z_scale) == (4.0, 5.0, api.OKCovarianceType.EXPONENTIAL, 0.0)


def test_geo_point_source_surface():
    from shyft_amd import api
    ta = api.TimeAxisFixedDeltaT(0, 3600, 4)
    ts = api.TimeSeries(ta, [1.0, 2.0, 3.0, 4.0], api.POINT_AVERAGE_VALUE)
    g = api.GeoPointSource(api.GeoPoint(1.0, 2.0, 3.0), ts)
    assert (g.mid_point().x, g.mid_point_.y, g.mid_point().z) == (1.0, 2.0, 3.0)
    assert g.ts is ts and g.uid == ""
    g.mid_point_ = api.GeoPoint(7.0, 8.0, 9.0)
    g.uid = "site"
    assert g.mid_point().x == 7.0 and g.uid == "site"
    v = api.GeoPointSourceVector()
    v.append(g)
    assert v.size() == 1 and len(v) == 1
    assert isinstance(api.TemperatureSource(), api.GeoPointSource)


def _grid(api, nx, ny, dx, max_elevation=1000):
    out = api.GeoPointVector()
    for i in range(nx):
        for j in range(ny):
            out.append(api.GeoPoint(i * dx, j * dx, max_elevation * (i + j) / (nx + ny)))
    return out


def _axes(api):
    t = api.Calendar().time(2016, 9, 1)
    d, n = api.deltahours(1), 24
    return api.TimeAxisFixedDeltaT(t, d * 3, n // 3), api.TimeAxisFixedDeltaT(t, d, n)


def _site(api, ta_obs, level, amplitude):
    wave = np.sin(np.arange(ta_obs.size()) * 2 * np.pi / 8.0 - np.pi / 2.0)
    return api.TimeSeries(ta_obs, values=api.DoubleVector.from_numpy(level + amplitude * wave),
                          point_fx=api.POINT_AVERAGE_VALUE)


def test_one_site_is_copied_to_the_grid():
    from shyft_amd import api
    ta_obs, ta_grid = _axes(api)
    p = api.OKParameter(c=1.0, a=10.0 * 1000.0, cov_type=api.OKCovarianceType.EXPONENTIAL, z_scale=1.0)
    ts_site_1 = _site(api, ta_obs, 1.0, 0.1)
    sites = api.GeoPointSourceVector()
    sites.append(api.GeoPointSource(api.GeoPoint(50.0, 50.0, 5.0), ts_site_1))
    grid = _grid(api, 5, 5, 1000)
    r = api.ordinary_kriging(sites, grid, ta_grid, p)
    assert isinstance(r, api.GeoPointSourceVector) and len(r) == 25
    expected = ts_site_1.average(ta_grid).values.to_numpy()
    for gts, gp in zip(r, grid):
        assert isinstance(gts, api.GeoPointSource) and gts.mid_point() is gp
        assert gts.ts.size() == ta_grid.size()
        assert gts.ts.point_interpretation() == api.POINT_AVERAGE_VALUE
        assert np.allclose(expected, gts.ts.values.to_numpy())
    # the typed source vectors are accepted as well
    typed = api.TemperatureSourceVector()
    typed.append(api.TemperatureSource(api.GeoPoint(50.0, 50.0, 5.0), ts_site_1))
    assert np.allclose(expected, api.ordinary_kriging(typed, grid, ta_grid, p)[3].ts.values.to_numpy())


def test_error_texts():
    from shyft_amd import api
    ta_obs, ta_grid = _axes(api)
    sites = api.GeoPointSourceVector()
    sites.append(api.GeoPointSource(api.GeoPoint(50.0, 50.0, 5.0), _site(api, ta_obs, 1.0, 0.1)))
    grid = _grid(api, 2, 2, 1000)
    ok = api.OKParameter()
    with pytest.raises(RuntimeError, match="at least one time-series"):
        api.ordinary_kriging(api.GeoPointSourceVector(), grid, ta_grid, ok)
    with pytest.raises(RuntimeError, match="at least one time-series"):
        api.ordinary_kriging(sites, api.GeoPointVector(), ta_grid, ok)
    with pytest.raises(RuntimeError, match="more than 0 element"):
        api.ordinary_kriging(sites, grid, api.TimeAxisFixedDeltaT(0, 3600, 0), ok)
    with pytest.raises(RuntimeError, match="parameter a, covariance practical range, must be >0.0"):
        api.ordinary_kriging(sites, grid, ta_grid, api.OKParameter(a=0.0))
    with pytest.raises(RuntimeError, match="parameter c, covariance sill, must be >0.0"):
        api.ordinary_kriging(sites, grid, ta_grid, api.OKParameter(c=-1.0))
    with pytest.raises(RuntimeError, match="z_scale used to scale vertical distance must be >= 0.0"):
        api.ordinary_kriging(sites, grid, ta_grid, api.OKParameter(z_scale=-0.5))


def test_coincident_sources_are_singular():
    from shyft_amd import region
    src, obs, dst = ok_cases.case(5, 7, 3)
    src[3] = src[1]
    with pytest.raises(RuntimeError, match=r"inv\(\): matrix is singular"):
        region.ordinary_kriging(src, obs, (1.0, 10000.0, 1.0, EXPONENTIAL), dst, host=True)


def test_nan_observation_makes_exactly_its_step_nan():
    from shyft_amd import region
    src, obs, dst = ok_cases.case(5, 70, 8)
    param = (1.0, 10000.0, 1.0, EXPONENTIAL)
    clean = region.ordinary_kriging(src, obs, param, dst, host=True)
    obs[3, 2] = np.nan
    got = region.ordinary_kriging(src, obs, param, dst, host=True)
    assert np.isnan(got[3]).all()
    keep = np.arange(8) != 3
    assert np.array_equal(got[keep], clean[keep])


def test_empty_steps_or_destinations_return_empty():
    from shyft_amd import region
    src, obs, dst = ok_cases.case(5, 7, 3)
    param = (1.0, 10000.0, 1.0, EXPONENTIAL)
    assert region.ordinary_kriging(src, obs, param, dst[:0], host=True).shape == (3, 0)
    assert region.ordinary_kriging(src, obs[:0], param, dst, host=True).shape == (0, 7)
