"""The batched Kalman kernel on the GPU: shyft_hip_kalman_run is bit-identical to shyft_hip_kalman_run_host over the
shapes at which the lane mapping of kernels/kalman.hip can go wrong, then the layout with an asymmetric P and
KalmanBiasPredictorVector on the three points of the reference's shyft/tests/api/test_grid_pp.py.

The kernel gives a point G lanes, G the power of two >= n, in workgroups of 256 lanes: n in {1, 2, 3, 4, 6, 8, 12,
24, 32} is every G with and without padded rows; for each G, M in {1, 64/G - 1, 64/G, 64/G + 1, 256/G + 1, 257, 1000}
is a partial group, a wave boundary, a workgroup boundary and several workgroups; T in {1, 8, 9, 80}. Axes: 3-hourly
from midnight, 3-hourly from 07:00 (fold and the profile anchor are not 0), hourly (repeated fold index, one-piece
average (v 3600) / 3600) and 6-hourly (two-piece average at n = 8)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 4, 6, 8, 12, 24, 32)
TS = (1, 8, 9, 80)
AXES = {"3h": (0, 3), "3h@07": (7, 3), "1h": (0, 1), "6h": (0, 6)}  # start hour, step hours
FILTER, PREDICTOR, RUNNING = 0, 1, 2
T0 = 1451606400  # 2016-01-01


def _group(n):
    g = 1
    while g < n:
        g *= 2
    return g


def _ms(n):
    g = _group(n)
    return sorted({m for m in (1, 64 // g - 1, 64 // g, 64 // g + 1, 256 // g + 1, 257, 1000) if m > 0})


def _sampled_cases():
    """every (n, M of that n's G) pair once, T, the mode and the axis cycling through them; then every axis and every
    T with the running bias at n = 8, and the corners"""
    cases, c = [], 0
    axes = list(AXES)
    for n in NS:
        for m in _ms(n):
            cases.append((n, m, TS[c % 4], (FILTER, PREDICTOR, RUNNING)[c % 3], axes[(c // 3) % 4]))
            c += 1
    for a in axes:
        for t in TS:
            cases.append((8, 65, t, RUNNING, a))
    cases += [(32, 1000, 80, RUNNING, "3h@07"), (24, 257, 80, FILTER, "1h"), (1, 1000, 80, RUNNING, "6h"),
              (6, 257, 9, RUNNING, "3h@07"), (12, 17, 80, PREDICTOR, "6h"), (3, 1000, 9, RUNNING, "1h")]
    assert {x[0] for x in cases} == set(NS) and {x[2] for x in cases} == set(TS) and {x[4] for x in cases} == set(AXES)
    for n in NS:
        assert {x[1] for x in cases if x[0] == n} >= set(_ms(n))
    return sorted(set(cases))


def _inputs(n, M, T, axis):
    """the library's own start matrices, distinct x per point, about 20 % NaN placed per point, one all-NaN step
    (when T > 2) and one all-NaN point (when M > 2)"""
    from shyft_amd import api, region
    rng = np.random.default_rng(1000 * n + 10 * M + T)
    f = api.KalmanFilter(api.KalmanParameter(n_daily_observations=n))
    s0 = f.create_initial_state()
    h0, dh = AXES[axis]
    t = f._tables(api.TimeAxis(T0 + 3600 * h0, 3600 * dh, T), True)
    bias = rng.normal(2.0, 1.5, (T, M))
    bias[rng.random((T, M)) < 0.2] = np.nan
    if T > 2:
        bias[T // 2, :] = np.nan
    if M > 2:
        bias[:, M // 2] = np.nan
    x = rng.normal(0.0, 1.0, (n, M))
    k = rng.normal(0.0, 0.1, (n, M))
    P = np.repeat(np.asarray(s0.P).reshape(n * n, 1), M, axis=1) * rng.uniform(0.5, 1.5, (1, M))
    return region, t, np.asarray(s0.W)[0, :n // 2 + 1].copy(), bias, x, k, P


def _both(region, t, w, bias, x, k, P, mode):
    running = (t["save_every"], t["piece_begin"], t["piece_ix"], t["piece_seconds"]) if mode == RUNNING else None
    kw = dict(mode=FILTER if mode == FILTER else PREDICTOR, running=running)
    host = region.kalman_run(bias, t["fold"], w, t["v2"], x, k, P, host=True, **kw)
    dev = region.kalman_run(bias, t["fold"], w, t["v2"], x, k, P, **kw)
    return host, dev


@pytest.mark.parametrize("n,M,T,mode,axis", _sampled_cases())
def test_device_is_bit_identical_to_host(n, M, T, mode, axis):
    region, t, w, bias, x, k, P = _inputs(n, M, T, axis)
    x0, P0 = x.copy(), P.copy()
    host, dev = _both(region, t, w, bias, x, k, P, mode)
    for name, h, d in zip(("x", "k", "P"), host, dev):
        assert d.shape == h.shape, name
        assert np.array_equal(d, h, equal_nan=True), name
    if mode == RUNNING:
        assert dev[3].shape == (T, M)
        assert np.array_equal(dev[3], host[3], equal_nan=True)
        assert np.isfinite(dev[3]).all()
    else:
        assert dev[3] is None
    assert np.array_equal(x, x0) and np.array_equal(P, P0)  # the wrapper works on copies
    if M > 2:  # the all-NaN point: untouched in predictor mode, only P grown in filter mode
        j = M // 2
        assert np.array_equal(dev[0][:, j], x0[:, j])
        grown = not np.array_equal(dev[2][:, :, j].reshape(-1), P0[:, j])
        assert grown == (mode == FILTER)
    assert np.isfinite(dev[0]).all() and np.isfinite(dev[2]).all()


def test_layout_with_asymmetric_p():
    """a deliberately asymmetric P and distinct values per point against the numpy statement of the host tests: a
    transposed row / column or a swapped broadcast cannot hide behind symmetry"""
    from shyft_amd import region
    from tests.test_kalman_host import np_update
    n, M, T = 6, 67, 7
    rng = np.random.default_rng(42)
    P0 = rng.uniform(0.1, 1.0, (n, n, M)) + 2.0 * np.eye(n)[:, :, None]
    assert not np.allclose(P0[:, :, 0], P0[:, :, 0].T)
    _, W = region.kalman_initial_state(n, 0.5, 0.93, 0.3)
    x0, k0 = rng.normal(size=(n, M)), np.zeros((n, M))
    bias = rng.normal(2.0, 1.0, (T, M))
    bias[3, ::5] = np.nan
    fold = np.array([4, 1, 5, 0, 2, 3, 1], dtype=np.int32)
    for mode in (FILTER, PREDICTOR):
        x, k, P, _ = region.kalman_run(bias, fold, W[0, :n // 2 + 1], 4.0, x0, k0, P0, mode=mode)
        for m in range(M):
            xs, ks, Ps = x0[:, m].copy(), k0[:, m].copy(), P0[:, :, m].copy()
            for t in range(T):
                xs, ks, Ps = np_update(xs, ks, Ps, W, 4.0, bias[t, m], fold[t], mode == PREDICTOR)
            assert np.array_equal(xs, x[:, m]), (mode, m)
            assert np.array_equal(ks, k[:, m]), (mode, m)
            assert np.array_equal(Ps, P[:, :, m]), (mode, m)


def test_last_ms_reports_the_kernel():
    from shyft_amd import region
    region_, t, w, bias, x, k, P = _inputs(8, 1000, 80, "3h")
    region.kalman_run(bias, t["fold"], w, t["v2"], x, k, P)
    assert 0.0 < region.kalman_last_ms() < 1000.0


def test_predictor_vector_on_the_grid_pp_points():
    """test_grid_pp.py:12-71: three points, a constant hourly observation over ten days (15.0, here moved by
    0.25 per point so the points differ), forecast = observation + 2.0. The
    vector is bitwise three single predictors and bitwise its host restatement, and every x[i] - 2.0 < 0.2."""
    from shyft_amd import api
    t0 = api.Calendar().time(2016, 1, 1)
    ta = api.TimeAxis(t0, api.deltahours(1), 24 * 10)
    points = [api.GeoPoint(100, 100, 1000), api.GeoPoint(5100, 100, 1150), api.GeoPoint(100, 5100, 850)]
    obs_set, fc_set = api.TemperatureSourceVector(), api.TemperatureSourceVector()
    for j, gp in enumerate(points):
        obs = api.TimeSeries(ta, [15.0 + 0.25 * j] * ta.size(), api.POINT_AVERAGE_VALUE)  # distinct per point
        obs_set.append(api.TemperatureSource(gp, obs))
        fc_set.append(api.TemperatureSource(gp, api.TimeSeries(ta, [v + 2.0 for v in obs.values],
                                                               api.POINT_AVERAGE_VALUE)))
    kta = api.TimeAxis(t0, api.deltahours(3), 8)
    cycles = [fc_set, fc_set, fc_set]  # the reference's loop feeds the forecast set once per observation
    dev = api.KalmanBiasPredictorVector(api.KalmanFilter(), 3)
    dev.update_with_forecast(cycles, obs_set, kta)
    host = api.KalmanBiasPredictorVector(api.KalmanFilter(), 3)
    host.update_with_forecast(cycles, obs_set, kta, host=True)
    assert np.array_equal(dev.x, host.x) and np.array_equal(dev.k, host.k) and np.array_equal(dev.P, host.P)
    for j in range(3):
        bp = api.KalmanBiasPredictor(api.KalmanFilter())
        bp.update_with_forecast(api.TemperatureSourceVector(c[j] for c in cycles), obs_set[j].ts, kta)
        assert np.array_equal(dev.x[j], bp.state.x) and np.array_equal(dev.k[j], bp.state.k)
        assert np.array_equal(dev.P[j], bp.state.P)
        assert np.array_equal(dev[j].state.x, bp.state.x)
        for b in api.KalmanState.get_x(bp.state):
            assert b - 2.0 < 0.2
    assert (dev.x - 2.0 < 0.2).all()
    # the running bias through the same two paths, on a ten-day axis
    kta10 = api.TimeAxis(t0, api.deltahours(3), 80)
    rd = dev.compute_running_bias(fc_set, obs_set, kta10)
    rh = host.compute_running_bias(fc_set, obs_set, kta10, host=True)
    assert isinstance(rd, api.TemperatureSourceVector) and len(rd) == 3
    for j in range(3):
        assert np.array_equal(np.array(rd[j].ts.values), np.array(rh[j].ts.values))
        assert rd[j].mid_point().z == points[j].z
    assert np.array_equal(dev.x, host.x)
