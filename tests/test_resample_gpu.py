"""The resample kernels on the GPU: shyft_hip_resample is bit-identical to shyft_hip_resample_host (which runs the
host's average_values / accumulate_value) in all three modes and on both launch shapes, over the shapes at which
kernels/resample.hip can go wrong, then TsVector.average / integral / accumulate on the device and the sources of
region_model.run_interpolation.

Every one of the eleven axes of tests/resample_cases.py (the series' own, 2x and 24x coarser, 2x and 4x finer, shifted
by dt/4, starting before the first point with it inside a period and on a period boundary, running past the series'
end with a period starting exactly at t_end, wholly before and wholly after) meets T in {1, 2, 63, 64, 65, 300}; S in
{1, 63, 64, 65, 257} and the three time bases (2016, negative, above 2^53 us with an odd spacing) rotate over them.
A batch mixes series of 0, 1, 2, 3, 63, 64, 65, 257 and 1000 points, evenly spaced and irregular, both point types
and the value hazards of resample_cases.make_batch, so the CSR offsets matter. T = 63 / 64 / 65 and S = 1 / 63 / 65 /
257 leave partial 16 x 64 tiles and partial workgroups, 300 x 257 takes many of both."""
import numpy as np
import pytest

from tests import resample_cases as rc

pytestmark = pytest.mark.gpu

SS = (1, 63, 64, 65, 257)
TS = (1, 2, 63, 64, 65, 300)
MODES = (0, 1, 2)  # AVERAGE, INTEGRAL, ACCUMULATE


def _cases():
    cases = []
    for k, kind in enumerate(rc.AXES):
        for j, T in enumerate(TS):
            cases.append((kind, SS[(j + k) % len(SS)], T, (j + 2 * k) % len(rc.EPOCHS)))
    assert {c[1] for c in cases} == set(SS) and {c[3] for c in cases} == {0, 1, 2}
    return cases


@pytest.fixture(scope="module")
def region():
    from shyft_amd import region
    yield region
    region.resample_set_path(region.RESAMPLE_PATH_AUTO)


@pytest.mark.parametrize("kind,S,T,epoch", _cases())
def test_device_is_bit_identical_to_host(region, kind, S, T, epoch):
    t0, dt = rc.EPOCHS[epoch]
    seed = 7000 + 100 * rc.AXES.index(kind) + 10 * TS.index(T) + epoch
    batch = rc.make_batch(S, t0, dt, seed, first=seed % len(rc.LENGTHS), min_points=2 if kind == "before" else 0)
    ta_t0, ta_dt = rc.axis(kind, t0, dt, T)
    for mode in MODES:
        host = region.resample_csr(*batch, ta_t0, ta_dt, T, mode, host=True)
        assert host.shape == (T, S)
        for path in (region.RESAMPLE_PATH_DIRECT, region.RESAMPLE_PATH_TILED):
            region.resample_set_path(path)
            dev = region.resample_csr(*batch, ta_t0, ta_dt, T, mode)
            assert region.resample_last_path() == path
            bad = np.argwhere(~((np.isnan(dev) & np.isnan(host)) | (dev.view(np.uint64) == host.view(np.uint64))))
            assert rc.same_bits(dev, host), (mode, path, len(bad), bad[:4].tolist())


def test_auto_takes_the_tiled_shape_from_64_intervals_on(region):
    t0, dt = rc.EPOCHS[0]
    batch = rc.make_batch(5, t0, dt, 3)
    region.resample_set_path(region.RESAMPLE_PATH_AUTO)
    region.resample_csr(*batch, t0, dt, 63)
    assert region.resample_last_path() == region.RESAMPLE_PATH_DIRECT
    region.resample_csr(*batch, t0, dt, 64)
    assert region.resample_last_path() == region.RESAMPLE_PATH_TILED


def test_calls_count_device_launches_only(region):
    t0, dt = rc.EPOCHS[0]
    batch = rc.make_batch(9, t0, dt, 4)
    n0 = region.resample_calls()
    region.resample_csr(*batch, t0, dt, 10, 2)
    assert region.resample_calls() == n0 + 1
    region.resample_csr(*batch, t0, dt, 10, 2, host=True)
    region.resample_csr(*batch, t0, dt, 0)                         # T == 0 launches nothing
    region.resample_csr(np.zeros(1, np.int64), [], [], [], [], t0, dt, 10)  # S == 0 neither
    assert region.resample_calls() == n0 + 1
    assert region.resample_last_ms() > 0.0


def test_a_refused_batch_launches_nothing(region):
    from shyft_amd._native import ShyftHipError
    t0, dt = rc.EPOCHS[0]
    n0 = region.resample_calls()
    with pytest.raises(ShyftHipError, match="needs time-points in increasing order"):
        region.resample_csr([0, 2], [t0 + dt, t0], [1.0, 2.0], [t0 + 2 * dt], [0], t0, dt, 4)
    with pytest.raises(ShyftHipError, match="one-point series"):
        region.resample_csr([0, 1], [t0 + dt // 2], [1.0], [t0 + dt], [0], t0, dt, 4)
    assert region.resample_calls() == n0


def test_ts_vector_methods_run_on_the_device_and_equal_the_host_series(region):
    """TsVector.average(ta) equals the per-series TimeSeries.average(ta) exactly; integral and accumulate equal the
    host methods; one device call each"""
    from shyft_amd import api
    rng = np.random.default_rng(11)
    t0 = 1451606400
    tsv = api.TsVector()
    for k in range(7):
        n = (5, 40, 64, 90)[k % 4]
        times = t0 + 10800 * np.arange(n) + np.concatenate([[0], rng.integers(0, 10000, n - 1)])
        values = rng.normal(3.0, 2.0, n)
        values[rng.random(n) < 0.2] = np.nan
        fx = api.POINT_INSTANT_VALUE if k % 2 else api.POINT_AVERAGE_VALUE
        tsv.append(api.TsFactory().create_time_point_ts(api.UtcPeriod(int(times[0]), int(times[-1]) + 10800),
                                                        times.tolist(), values.tolist(), fx))
    ta = api.TimeAxis(t0 - 7200, 3600, 200)
    region.resample_set_path(region.RESAMPLE_PATH_AUTO)
    for name, fx in (("average", api.POINT_AVERAGE_VALUE), ("integral", api.POINT_AVERAGE_VALUE),
                     ("accumulate", api.POINT_INSTANT_VALUE)):
        n0 = region.resample_calls()
        dev = getattr(tsv, name)(ta)
        assert region.resample_calls() == n0 + 1
        assert isinstance(dev, api.TsVector) and len(dev) == len(tsv)
        for ts, d in zip(tsv, dev):
            one = getattr(ts, name)(ta)
            assert d.point_interpretation() == fx and d.size() == ta.size()
            assert rc.same_bits(np.asarray(d.values), np.asarray(one.values)), name
        free = getattr(api, name)(tsv, ta)
        assert region.resample_calls() == n0 + 2
        assert all(rc.same_bits(np.asarray(a.values), np.asarray(b.values)) for a, b in zip(free, dev))


def test_run_interpolation_resamples_on_the_device_and_keeps_the_forcing(region):
    """A small region with irregular 3-hourly sources: run_interpolation (sources onto the axis by one
    shyft_hip_resample call per variable) gives forcing equal bit for bit to region.interpolate / interpolate_btk fed
    with the host's averages."""
    from shyft_amd import api
    from shyft_amd.api import pt_gs_k
    rng = np.random.default_rng(21)
    n, n_src, T, t0 = 200, 5, 48, 1451606400
    geo = np.zeros((n, 11))
    gcds = api.GeoCellDataVector()
    for i in range(n):
        geo[i] = (500.0 + 1000.0 * (i % 20), 500.0 + 1000.0 * (i // 20), 1000.0 * rng.random(), 1e6, 1, 0.9,
                  0.01, 0.05, 0.19, 0.3, 0.45)
        gcds.append(api.GeoCellData(api.GeoPoint(*geo[i, :3]), 1e6, 1, 0.9,
                                    api.LandTypeFractions(0.01, 0.05, 0.19, 0.3, 0.45)))
    ta = api.TimeAxis(t0, 3600, T)

    def sources(vec, src_t, base, span):
        xyz = np.column_stack([20000.0 * rng.random(n_src), 10000.0 * rng.random(n_src), 1000.0 * rng.random(n_src)])
        for k in range(n_src):
            m = 20
            times = t0 - 3600 + 10800 * np.arange(m) + np.concatenate([[0], rng.integers(0, 9000, m - 1)])
            values = base + span * rng.random(m)
            if k == 1:
                values[rng.random(m) < 0.2] = np.nan
            fx = api.POINT_INSTANT_VALUE if k % 2 == 0 else api.POINT_AVERAGE_VALUE
            ts = api.TsFactory().create_time_point_ts(api.UtcPeriod(int(times[0]), int(times[-1]) + 10800),
                                                      times.tolist(), values.tolist(), fx)
            vec.append(src_t(api.GeoPoint(*xyz[k]), ts))
        return xyz, np.column_stack([np.asarray(s.ts.average(ta).values) for s in vec])

    env = api.ARegionEnvironment()
    env.radiation = api.RadiationSourceVector()
    src = {region.TEMPERATURE: sources(env.temperature, api.TemperatureSource, 2.0, 8.0),
           region.PRECIPITATION: sources(env.precipitation, api.PrecipitationSource, 0.0, 2.0),
           region.RADIATION: sources(env.radiation, api.RadiationSource, 100.0, 200.0),
           region.WIND_SPEED: sources(env.wind_speed, api.WindSpeedSource, 1.0, 4.0),
           region.REL_HUM: sources(env.rel_hum, api.RelHumSource, 0.4, 0.5)}
    assert any(np.isnan(v).any() for _, v in src.values())

    ref = region.HipRegion(region.PT_GS_K, n)
    ref.set_geo(geo)
    ref.set_time_axis(t0 * 10**6, 3600 * 10**6, T)
    for use_idw in (True, False):
        ip = api.InterpolationParameter()
        ip.use_idw_for_temperature = use_idw
        ip.temperature_idw.max_distance = ip.precipitation.max_distance = ip.radiation.max_distance = 1e6
        ip.wind_speed.max_distance = ip.rel_hum.max_distance = 1e6
        model = pt_gs_k.PTGSKModel(gcds, pt_gs_k.PTGSKParameter())
        n0 = region.resample_calls()
        assert model.run_interpolation(ip, ta, env, best_effort=False)
        assert region.resample_calls() == n0 + 5  # one per variable, no per-series host pass
        for var, (xyz, vals) in src.items():
            p = {region.TEMPERATURE: ip.temperature_idw, region.PRECIPITATION: ip.precipitation,
                 region.RADIATION: ip.radiation, region.WIND_SPEED: ip.wind_speed, region.REL_HUM: ip.rel_hum}[var]
            if var == region.TEMPERATURE and not use_idw:
                b = ip.temperature
                prior = [b.temperature_gradient(ta.period(i)) for i in range(T)]
                ref.interpolate_btk(xyz, vals, 0, [b.temperature_gradient_sd(), b.sill(), b.nug(), b.range(),
                                                   b.zscale()], prior)
            else:
                gradient, by_eq, scale = -0.006, 0.0, 1.02
                if var == region.TEMPERATURE:
                    gradient, by_eq = p.default_temp_gradient, float(p.gradient_by_equation)
                if var == region.PRECIPITATION:
                    scale = p.scale_factor
                ref.interpolate(var, xyz, vals, 0, [p.max_members, p.max_distance, p.distance_measure_factor, p.zscale,
                                                    gradient, by_eq, scale])
            want = ref.get_forcing(var, 0, T)
            got = np.column_stack([np.asarray(model._cell_series(region.SERIES_FORCING + var, c)) for c in range(n)])
            assert want.shape == got.shape == (T, n)
            assert rc.same_bits(got, want), (use_idw, var)
    ref.close()
