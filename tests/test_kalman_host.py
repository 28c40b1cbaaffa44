"""Kalman bias prediction on the host path (no GPU): the cases of the reference's shyft/tests/api/test_kalman.py and
test/kalman_test.cpp (its signal generator at noise 0; its random stream cannot be reproduced) with the
reference's own bounds, the host restatement shyft_hip_kalman_run_host bit for bit against a numpy statement of
core/kalman.h:127-145 written here, fold_to_daily_observation's integer arithmetic, and the refusals."""
import math

import numpy as np
import pytest

NAN = float("nan")
PATTERN = (2.0, 1.9, 1.8, 1.7, 1.8, 1.8, 1.9, 2.0)  # kalman_test.cpp:20


@pytest.fixture(scope="module")
def api():
    from shyft_amd import api
    return api


def _const_ts(api, ta, x, fx=None):
    v = np.arange(ta.size())
    v.fill(x)
    return api.TimeSeries(ta=ta, values=api.DoubleVector.from_numpy(v),
                          point_fx=api.point_interpretation_policy.POINT_AVERAGE_VALUE if fx is None else fx)


def _forecast_set(api, vec, n_fc, t0, dt, n_steps, dt_fc, x):
    for i in range(n_fc):
        ts = _const_ts(api, api.TimeAxis(t0 + i * dt_fc, dt, n_steps), x)
        vec.append(api.TemperatureSource(api.GeoPoint(0.0, 0.0, 0.0), ts) if hasattr(vec, "values_at_time") else ts)
    return vec


# ---- shyft/tests/api/test_kalman.py ----------------------------------------------------------------------------------
def test_parameter(api):
    p = api.KalmanParameter()
    assert p.n_daily_observations == 8
    assert p.hourly_correlation == pytest.approx(0.93)
    assert p.covariance_init == pytest.approx(0.5)
    assert p.std_error_bias_measurements == pytest.approx(2.0)
    assert p.ratio_std_w_over_v == pytest.approx(0.15)
    p = api.KalmanParameter(n_daily_observations=6, hourly_correlation=0.9, covariance_init=0.4,
                            std_error_bias_measurements=1.0, ratio_std_w_over_v=0.05)
    assert p.n_daily_observations == 6
    assert p.ratio_std_w_over_v == pytest.approx(0.05)
    assert p.hourly_correlation == pytest.approx(0.9)
    assert p.covariance_init == pytest.approx(0.4)
    assert p.std_error_bias_measurements == pytest.approx(1.0)
    p.n_daily_observations = 8
    assert p.n_daily_observations == 8
    q = api.KalmanParameter(p)
    assert (q.n_daily_observations, q.hourly_correlation, q.covariance_init, q.std_error_bias_measurements,
            q.ratio_std_w_over_v) == (8, p.hourly_correlation, p.covariance_init, p.std_error_bias_measurements,
                                      p.ratio_std_w_over_v)
    q.covariance_init = 0.1  # a copy, not a reference
    assert p.covariance_init == pytest.approx(0.4)


def test_state(api):
    s = api.KalmanState()
    assert s.size() == 0
    s = api.KalmanState(n_daily_observations=8, covariance_init=0.5, hourly_correlation=0.93, process_noise_init=0.06)
    assert s.size() == 8
    assert len(api.KalmanState.get_x(s)) == 8 and len(api.KalmanState.get_k(s)) == 8
    assert len(api.KalmanState.get_P(s)) == 64 and len(api.KalmanState.get_W(s)) == 64
    assert np.array_equal(np.array(api.KalmanState.get_P(s)).reshape(8, 8), s.P)  # flattened row by row
    assert api.KalmanState(s).size() == 8


def test_filter(api):
    f = api.KalmanFilter()
    assert f.parameter.n_daily_observations == 8
    s = f.create_initial_state()
    assert s.size() == 8
    ta = api.TimeAxis(api.Calendar().time(2015, 1, 1), api.deltahours(3), 8)
    for i in range(ta.size()):
        f.update(2.0, ta.time(i), s)
    assert len(s.x) == 8 and len(s.k) == 8
    assert s.P.shape == (8, 8) and s.W.shape == (8, 8)


def test_initial_state_rule_for_zero_measurement_error(api):
    """create_initial_state (kalman.h:109-111): process noise ratio * std_error, or 100.0 when std_error is 0"""
    w = api.KalmanFilter(api.KalmanParameter(std_error_bias_measurements=0.0)).create_initial_state().W
    assert w[0, 0] == 100.0 * 100.0
    w = api.KalmanFilter().create_initial_state().W
    assert w[0, 0] == (0.15 * 2.0) * (0.15 * 2.0)


@pytest.mark.parametrize("as_sources_first", [True, False])
def test_bias_predictor(api, as_sources_first):
    bp = api.KalmanBiasPredictor(api.KalmanFilter())
    assert bp.filter.parameter.n_daily_observations == 8
    t0 = api.Calendar().time(2016, 1, 1)
    dt = api.deltahours(1)
    obs_ts = api.TimeSeries(api.TimeAxis(t0, dt, 24), fill_value=0.0, point_fx=api.POINT_INSTANT_VALUE)
    kalman_ta = api.TimeAxis(t0, api.deltahours(3), 8)
    kinds = [api.TemperatureSourceVector, api.TsVector]
    for kind in kinds if as_sources_first else kinds[::-1]:
        bp.update_with_forecast(_forecast_set(api, kind(), 8, t0, dt, 36, api.deltahours(6), 2.0), obs_ts, kalman_ta)
    bias_pattern = bp.state.x
    assert len(bias_pattern) == 8
    for b in bias_pattern:
        assert abs(b - 2.0) < 0.2


def test_bias_predictor_static_forms_equal_the_methods(api):
    t0 = api.Calendar().time(2016, 1, 1)
    dt = api.deltahours(1)
    obs_ts = api.TimeSeries(api.TimeAxis(t0, dt, 24), fill_value=0.0, point_fx=api.POINT_INSTANT_VALUE)
    kalman_ta = api.TimeAxis(t0, api.deltahours(3), 8)
    geo = _forecast_set(api, api.TemperatureSourceVector(), 8, t0, dt, 36, api.deltahours(6), 2.0)
    tsv = _forecast_set(api, api.TsVector(), 8, t0, dt, 36, api.deltahours(6), 2.0)
    a, b, c = (api.KalmanBiasPredictor(api.KalmanFilter()) for _ in range(3))
    a.update_with_forecast(geo, obs_ts, kalman_ta)
    api.KalmanBiasPredictor.update_with_geo_forecast(b, geo, obs_ts, kalman_ta)
    api.KalmanBiasPredictor.update_with_forecast_vector(c, tsv, obs_ts, kalman_ta)
    assert np.array_equal(a.state.x, b.state.x) and np.array_equal(a.state.x, c.state.x)
    assert np.array_equal(a.state.P, c.state.P)
    fc = _const_ts(api, api.TimeAxis(t0, dt, 24), 2.0)
    r1 = a.compute_running_bias(fc, obs_ts, kalman_ta)
    r2 = api.KalmanBiasPredictor.compute_running_bias_ts(b, fc, obs_ts, kalman_ta)
    assert np.array_equal(np.array(r1.values), np.array(r2.values))
    # a predictor built from a filter and a state starts from a copy of that state
    d = api.KalmanBiasPredictor(a.filter, a.state)
    assert np.array_equal(d.state.x, a.state.x)


def test_compute_running_bias(api):
    bp = api.KalmanBiasPredictor(api.KalmanFilter())
    t0 = api.Calendar().time(2016, 1, 1)
    dt = api.deltahours(1)
    n = 24 * 10
    obs_ts = api.TimeSeries(api.TimeAxis(t0, dt, n), fill_value=0.0, point_fx=api.POINT_INSTANT_VALUE)
    kalman_ta = api.TimeAxis(t0, api.deltahours(3), n // 3)
    fc_ts = _forecast_set(api, api.TsVector(), 1, t0, dt, n, api.deltahours(6), 2.0)[0]
    bias_ts = bp.compute_running_bias(fc_ts, obs_ts, kalman_ta)
    assert bias_ts.size() == kalman_ta.size()
    assert bias_ts.point_interpretation() == api.POINT_AVERAGE_VALUE
    bias_pattern = bp.state.x
    assert len(bias_pattern) == 8
    for b in bias_pattern:
        assert abs(b - 2.0) < 0.2
    for i in range(8):
        assert bias_ts.value(i) == 0.0  # a snapshot of the zero start state
    for i in range(8):
        assert abs(bias_ts.value(bias_ts.size() - i - 1) - 2.0) < 0.2


# ---- test/kalman_test.cpp, signal generator at noise 0 ---------------------------------------------------------------
def _observation(t):  # kalman_test.cpp:13-16, 32-34 (t0 = 1970)
    return 10.0 + 2.0 * math.sin(2 * 3.1415 / (24.0 * 3600.0) * t + (-2 * 3.1415 * 8 / 24))


def _bias_offset(t):
    return PATTERN[(int(t) // 3600) % 24 // 3]


def _signal_ts(api, ta, with_bias):
    v = [_observation(ta.time(i)) + (_bias_offset(ta.time(i)) if with_bias else 0.0) for i in range(ta.size())]
    return api.TimeSeries(ta, v, api.POINT_INSTANT_VALUE)  # point_ts(ta, fill)'s default policy


def test_cpp_filter(api):
    """three days of the pattern: within 0.21; then 24 missing observations leave x unchanged (the reference's 0.01)"""
    f = api.KalmanFilter(api.KalmanParameter())
    s = f.create_initial_state()
    for i in range(8 * 3):
        t = api.deltahours(3 * i)
        f.update(_bias_offset(t), t, s)
    worst = max(abs(_bias_offset(api.deltahours(3 * i)) - s.x[i]) for i in range(8))
    print("cpp test_filter worst", worst)
    assert worst <= 0.21
    x_known, p_known = s.x.copy(), s.P.copy()
    for i in range(8 * 3):
        f.update(NAN, api.deltahours(3 * (8 * 3 + i)), s)
    assert np.abs(s.x - x_known).max() <= 0.01
    assert np.array_equal(s.x, x_known)  # in fact untouched
    assert (s.P > p_known).all()  # only the error covariance has grown


def test_cpp_bias_predictor(api):
    t0 = api.Calendar().time(2000, 1, 1)
    dt = api.deltahours(1)
    observation = _signal_ts(api, api.TimeAxis(t0, dt, 24), False)
    fc_set = api.TsVector(_signal_ts(api, api.TimeAxis(t0 + api.deltahours(6 * i), dt, 36), True) for i in range(4))
    bp = api.KalmanBiasPredictor(api.KalmanFilter(api.KalmanParameter(8, 0.93, 0.5, 2.0, 0.22)))
    bp.update_with_forecast(fc_set, observation, api.TimeAxis(t0, api.deltahours(3), 8))
    worst = max(abs(_bias_offset(api.deltahours(3 * i)) - bp.state.x[i]) for i in range(8))
    print("cpp test_bias_predictor worst", worst)
    assert worst <= 0.4


def test_cpp_running_predictor(api):
    t0 = api.Calendar().time(2000, 1, 1)
    ta = api.TimeAxis(t0, api.deltahours(1), 240)
    bp = api.KalmanBiasPredictor(api.KalmanFilter(api.KalmanParameter()))
    pred_ta = api.TimeAxis(t0, api.deltahours(3), 80)
    bias_ts = bp.compute_running_bias(_signal_ts(api, ta, True), _signal_ts(api, ta, False), pred_ta)
    assert bias_ts.size() == pred_ta.size()
    first = max(abs(bias_ts.value(i)) for i in range(8))
    last = max(abs(_bias_offset(bias_ts.time(i)) - bias_ts.value(i)) for i in range(72, 80))
    print("cpp test_running_predictor first", first, "last", last)
    assert first <= 1e-4
    assert last <= 0.2


# ---- the host path against a numpy statement of kalman.h:127-145 -----------------------------------------------------
def np_update(x, k, P, W, v2, b, ix, predictor):
    """filter::update, element by element (every entry of the new P one product, one quotient, one difference)"""
    fin = np.isfinite(b)
    if fin or not predictor:
        P = P + W
    if not fin:
        return x, k, P
    tmp = P[ix, ix] + v2
    col, row = P[:, ix].copy(), P[ix, :].copy()
    k = col / tmp
    P = P - (col[:, None] * row[None, :]) / tmp
    x = x + k * (b - x[ix])
    return x, k, P


def mixed_bias(T, M, seed=5):
    rng = np.random.default_rng(seed)
    b = rng.normal(2.0, 1.5, (T, M))
    b[rng.random((T, M)) < 0.2] = NAN
    return b


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [8, 5])
def test_host_is_bit_identical_to_numpy(n, mode):
    from shyft_amd import region
    T, M = 80, 3
    P0, W = region.kalman_initial_state(n, 0.5, 0.93, 0.3)
    bias = mixed_bias(T, M)
    fold = np.array([(3 * t) % 24 * n // 24 for t in range(T)], dtype=np.int32)
    x, k, P, out = region.kalman_run(bias, fold, W[0, :n // 2 + 1], 4.0, np.zeros((n, M)), np.zeros((n, M)),
                                     np.repeat(P0.reshape(n * n, 1), M, axis=1), mode=mode, host=True)
    assert out is None
    for m in range(M):
        xs, ks, Ps = np.zeros(n), np.zeros(n), P0.copy()
        for t in range(T):
            xs, ks, Ps = np_update(xs, ks, Ps, W, 4.0, bias[t, m], fold[t], mode == 1)
        assert np.array_equal(xs, x[:, m]) and np.array_equal(ks, k[:, m]) and np.array_equal(Ps, P[:, :, m])
        assert np.array_equal(P[:, :, m], P[:, :, m].T)  # a symmetric P stays bit-symmetric


def test_predictor_mode_leaves_the_state_bitwise_unchanged_on_missing_bias():
    from shyft_amd import region
    n, M = 8, 2
    rng = np.random.default_rng(3)
    P0, W = region.kalman_initial_state(n, 0.5, 0.93, 0.3)
    x0, k0 = rng.normal(size=(n, M)), rng.normal(size=(n, M))
    Pm = np.repeat(P0.reshape(n * n, 1), M, axis=1)
    Pm[3, 0] = -0.0  # P + 0 would lose the sign
    bias = np.full((5, M), NAN)
    bias[2, 1] = float("inf")
    fold = np.arange(5, dtype=np.int32)
    x, k, P, _ = region.kalman_run(bias, fold, W[0, :5], 4.0, x0, k0, Pm, mode=region.KALMAN_PREDICTOR, host=True)
    assert x.tobytes() == x0.tobytes() and k.tobytes() == k0.tobytes() and P.tobytes() == Pm.tobytes()
    x, k, P, _ = region.kalman_run(bias, fold, W[0, :5], 4.0, x0, k0, Pm, mode=region.KALMAN_FILTER, host=True)
    assert x.tobytes() == x0.tobytes() and k.tobytes() == k0.tobytes()
    expect = P0
    for _ in range(5):
        expect = expect + W
    assert np.array_equal(P[:, :, 1], expect)


@pytest.mark.parametrize("n", [1, 6, 8, 24, 32])
def test_initial_matrices(n):
    """P = c r^(d 24/n), W = q^2 r^(d 24/n) over the folded distance d (kalman.h:37-50), against numpy's
    c * r ** (d 24/n). The bound is the one tests/test_detmath.py states for detmath::pow against the libm pow
    (test_exp_log_pow_within_one_ulp_of_glibc and test_edges_against_mpmath: <= 2 ulp; detmath/detmath.h:9) plus
    one ulp for the libm pow that numpy calls: 3 ulp."""
    from shyft_amd import region
    c, r, q = 0.5, 0.93, 0.3
    P, W = region.kalman_initial_state(n, c, r, q)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    d = np.minimum(np.abs(i - j), n - np.abs(i - j))
    for got, scale in ((P, c), (W, q * q)):
        want = scale * r ** (d * (24.0 / n))
        assert got.shape == (n, n)
        assert (np.abs(got - want) <= 3 * np.spacing(want)).all()
        assert np.array_equal(got, got.T)
        assert np.array_equal(got[0, 1:], got[0, 1:][::-1])  # circulant in the folded distance


def test_running_bias_tables_and_values(api):
    """a 6 h axis from 07:00 with n = 8: pieces of 2 h + 3 h + 1 h, profile anchored at midnight; the value is
    sum(v * seconds) / sum(seconds) in piece order over the snapshot taken every 4 steps"""
    from shyft_amd import region
    f = api.KalmanFilter()
    t0 = api.Calendar().time(2016, 1, 1, 7)
    ta = api.TimeAxis(t0, api.deltahours(6), 9)
    t = f._tables(ta, True)
    assert t["save_every"] == 4
    assert t["fold"].tolist() == [2, 4, 6, 0, 2, 4, 6, 0, 2]
    assert t["piece_begin"].tolist() == list(range(0, 28, 3))
    assert t["piece_ix"][:6].tolist() == [2, 3, 4, 4, 5, 6]
    assert t["piece_seconds"][:6].tolist() == [7200.0, 10800.0, 3600.0, 7200.0, 10800.0, 3600.0]
    s0 = f.create_initial_state()
    n, M, T = 8, 2, 9
    bias = mixed_bias(T, M, seed=9)
    x0 = np.random.default_rng(2).normal(size=(n, M))
    run = (t["save_every"], t["piece_begin"], t["piece_ix"], t["piece_seconds"])
    x, k, P, out = region.kalman_run(bias, t["fold"], s0.W[0, :5], t["v2"], x0, np.zeros((n, M)),
                                     np.repeat(s0.P.reshape(64, 1), M, axis=1), running=run, host=True)
    for m in range(M):
        xs, ks, Ps = x0[:, m].copy(), np.zeros(n), s0.P.copy()
        for i in range(T):
            if i % 4 == 0:
                snap = xs.copy()
            area = tsum = 0.0
            for p in range(t["piece_begin"][i], t["piece_begin"][i + 1]):
                area += snap[t["piece_ix"][p]] * t["piece_seconds"][p]
                tsum += t["piece_seconds"][p]
            assert out[i, m] == area / tsum
            xs, ks, Ps = np_update(xs, ks, Ps, s0.W, t["v2"], bias[i, m], t["fold"][i], True)
        assert np.array_equal(xs, x[:, m]) and np.array_equal(Ps, P[:, :, m])


def test_running_bias_profile_is_periodic_past_the_second_midnight(api):
    """An axis from 07:00 with fifteen 3 h steps (45 h) and n = 8: the profile bins are 3 h from midnight, so every
    step is 2 h of bin b and 1 h of bin b + 1, b = (7 + 3 i) // 3 mod 8, also for the steps after the second
    midnight (i >= 14), where the profile wraps to bin 0 again. (The reference's profile_accessor counts
    1 + 45 h / 24 h = 2 periods from midnight and would hold bin 7 flat past them; the staircase here is periodic
    on every step) No bias is observed, so the snapshot stays the start x."""
    from shyft_amd import region
    f = api.KalmanFilter()
    ta = api.TimeAxis(api.Calendar().time(2016, 1, 1, 7), api.deltahours(3), 17)
    t = f._tables(ta, True)
    s0 = f.create_initial_state()
    x0 = np.array([[1.0], [2.0], [4.0], [8.0], [16.0], [32.0], [64.0], [128.0]])
    run = (t["save_every"], t["piece_begin"], t["piece_ix"], t["piece_seconds"])
    x, k, P, out = region.kalman_run(np.full((17, 1), NAN), t["fold"], s0.W[0, :5], t["v2"], x0, np.zeros((8, 1)),
                                     s0.P.reshape(64, 1), running=run, host=True)
    assert np.array_equal(x, x0)
    for i in range(17):
        b = (7 + 3 * i) // 3 % 8
        assert out[i, 0] == (x0[b, 0] * 7200.0 + x0[(b + 1) % 8, 0] * 3600.0) / 10800.0, i
    # steps 14..16 start at 01:00, 04:00 and 07:00 of the third day: bins 0/1, 1/2 and 2/3 again
    assert out[14:, 0].tolist() == [(1.0 * 2 + 2.0) / 3, (2.0 * 2 + 4.0) / 3, (4.0 * 2 + 8.0) / 3]
    assert out[16, 0] == out[0, 0] == out[8, 0]


# ---- fold_to_daily_observation (kalman.h:114-116) ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 8, 24])
def test_fold(api, n):
    f = api.KalmanFilter(api.KalmanParameter(n_daily_observations=n))
    utc = api.Calendar()

    def ref(t):  # C++ integer division truncates towards zero
        hours = int(int(t) / 3600) if t >= 0 else -int(-int(t) // 3600)
        return (hours + 200 * 24 * 365) % 24 * n // 24

    midnight = utc.time(2016, 3, 1)
    assert f._fold_to_daily_observation(midnight) == 0
    assert f._fold_to_daily_observation(midnight + 86399) == n - 1  # 23:59:59
    assert f._fold_to_daily_observation(midnight + 12 * 3600) == n // 2
    for h in range(24):
        assert f._fold_to_daily_observation(midnight + h * 3600 + 1799) == h * n // 24
    # before 1970: the + 200 years keep the hour count positive; 1969-12-31 21:00 is hour 21 of its day
    assert f._fold_to_daily_observation(-3 * 3600) == 21 * n // 24
    assert f._fold_to_daily_observation(utc.time(1950, 6, 1, 7)) == 7 * n // 24
    for t in (-1, -3599, -3600, -3601, -86400, -86401, utc.time(1901, 1, 1, 13), utc.time(1969, 12, 31, 23, 59, 59)):
        assert f._fold_to_daily_observation(t) == ref(t), t
    # whole seconds truncate towards zero like the reference's to_seconds64: one second before 1970 counts as hour 0
    assert f._fold_to_daily_observation(-1) == 0
    ta = api.TimeAxis(midnight + 7 * 3600, api.deltahours(3), 9)
    assert f._tables(ta)["fold"].tolist() == [((7 + 3 * i) % 24) * n // 24 for i in range(9)]


# ---- refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 33])
def test_device_entry_refuses_n_outside_1_to_32(n):
    """refused before any device call, so this needs no GPU"""
    from shyft_amd import region
    from shyft_amd._native import ShyftHipError
    M = 2
    with pytest.raises(ShyftHipError, match=r"kalman: n_daily_observations must be in 1\.\.32 on the device"):
        region.kalman_run(np.zeros((1, M)), [0], np.zeros(n // 2 + 1), 4.0, np.zeros((n, M)), np.zeros((n, M)),
                          np.zeros((n * n, M)))


def test_host_entry_takes_n_above_32():
    from shyft_amd import region
    n = 33
    P0, W = region.kalman_initial_state(n, 0.5, 0.93, 0.3)
    x, k, P, _ = region.kalman_run([[1.0]], [4], W[0, :n // 2 + 1], 4.0, np.zeros((n, 1)), np.zeros((n, 1)),
                                   P0.reshape(n * n, 1), mode=0, host=True)
    xs, ks, Ps = np_update(np.zeros(n), np.zeros(n), P0, W, 4.0, 1.0, 4, False)
    assert np.array_equal(xs, x[:, 0]) and np.array_equal(Ps, P[:, :, 0])


def test_empty_batches_write_nothing():
    from shyft_amd import region
    n = 8
    P0, W = region.kalman_initial_state(n, 0.5, 0.93, 0.3)
    for host in (True, False):  # M == 0 or T == 0 returns before any device call
        x, k, P, _ = region.kalman_run(np.empty((0, 3)), [], W[0, :5], 4.0, np.ones((n, 3)), np.ones((n, 3)),
                                       np.ones((n * n, 3)), host=host)
        assert (x == 1).all() and (k == 1).all() and (P == 1).all()
        x, k, P, _ = region.kalman_run(np.empty((4, 0)), [0, 1, 2, 3], W[0, :5], 4.0, np.ones((n, 0)), np.ones((n, 0)),
                                       np.ones((n * n, 0)), host=host)
        assert x.shape == (n, 0)


@pytest.mark.parametrize("hours", [5, 48])
def test_running_bias_refuses_a_dt_that_does_not_divide_a_day(api, hours):
    t0 = api.Calendar().time(2016, 1, 1)
    hourly = api.TimeAxis(t0, api.deltahours(1), 24 * 10)
    fc, obs = _const_ts(api, hourly, 2.0), _const_ts(api, hourly, 0.0)
    ta = api.TimeAxis(t0, api.deltahours(hours), 4)
    bp = api.KalmanBiasPredictor(api.KalmanFilter())
    with pytest.raises(RuntimeError, match="delta-t that divides 24 hours"):
        bp.compute_running_bias(fc, obs, ta)
    assert np.array_equal(bp.state.x, np.zeros(8))  # refused before any update
    bp.update_with_forecast(api.TsVector([fc]), obs, ta)  # the plain update takes any axis
    v = api.KalmanBiasPredictorVector(api.KalmanFilter(), 1)
    with pytest.raises(RuntimeError, match="delta-t that divides 24 hours"):
        v.compute_running_bias(api.TsVector([fc]), api.TsVector([obs]), ta, host=True)


def test_vector_refusals(api):
    t0 = api.Calendar().time(2016, 1, 1)
    hourly = api.TimeAxis(t0, api.deltahours(1), 48)
    shifted = api.TimeAxis(t0 + 3600, api.deltahours(1), 48)
    kta = api.TimeAxis(t0, api.deltahours(3), 8)
    obs3 = api.TsVector(_const_ts(api, hourly, 0.0) for _ in range(3))
    v = api.KalmanBiasPredictorVector(api.KalmanFilter(), 3)
    good = api.TsVector(_const_ts(api, hourly, 2.0) for _ in range(3))
    mixed = api.TsVector([_const_ts(api, hourly, 2.0), _const_ts(api, shifted, 2.0), _const_ts(api, hourly, 2.0)])
    with pytest.raises(RuntimeError, match="forecast cycle 1 differ in time axis"):
        v.update_with_forecast([good, mixed], obs3, kta, host=True)
    with pytest.raises(RuntimeError, match="forecast cycle 0 holds 2 series, the vector has 3 points"):
        v.update_with_forecast([api.TsVector(list(good)[:2])], obs3, kta, host=True)
    with pytest.raises(RuntimeError, match="obs_set holds 2 series"):
        v.update_with_forecast([good], api.TsVector(list(obs3)[:2]), kta, host=True)
    with pytest.raises(RuntimeError, match="fc_set holds 4 series"):
        v.compute_running_bias(api.TsVector(list(good) + [good[0]]), obs3, kta, host=True)
    assert np.array_equal(v.x, np.zeros((3, 8)))  # nothing was updated by a refused call


def test_vector_on_the_host_equals_single_predictors(api):
    """host=True needs no device: every point equals a single KalmanBiasPredictor fed the series of that point"""
    t0 = api.Calendar().time(2016, 1, 1)
    dt = api.deltahours(1)
    kta = api.TimeAxis(t0, api.deltahours(3), 16)
    rng = np.random.default_rng(11)
    n_points, n_cycles = 4, 3
    obs = api.TsVector(api.TimeSeries(api.TimeAxis(t0, dt, 48), rng.normal(5, 1, 48), api.POINT_INSTANT_VALUE)
                       for _ in range(n_points))
    cycles = [api.TsVector(api.TimeSeries(api.TimeAxis(t0 + c * api.deltahours(6), dt, 36), rng.normal(7, 1, 36),
                                          api.POINT_AVERAGE_VALUE) for _ in range(n_points)) for c in range(n_cycles)]
    v = api.KalmanBiasPredictorVector(api.KalmanFilter(), n_points)
    v.update_with_forecast(cycles, obs, kta, host=True)
    assert v.x.shape == (n_points, 8) and v.k.shape == (n_points, 8) and v.P.shape == (n_points, 8, 8)
    merged = api.TsVector(api.TimeSeries(api.TimeAxis(t0, dt, 48), rng.normal(7, 1, 48), api.POINT_AVERAGE_VALUE)
                          for _ in range(n_points))
    singles = []
    for j in range(n_points):
        bp = api.KalmanBiasPredictor(api.KalmanFilter())
        bp.update_with_forecast(api.TsVector(c[j] for c in cycles), obs[j], kta)
        assert np.array_equal(v.x[j], bp.state.x) and np.array_equal(v.k[j], bp.state.k)
        assert np.array_equal(v.P[j], bp.state.P)
        assert np.array_equal(v[j].state.x, bp.state.x) and np.array_equal(v[j].state.P, bp.state.P)
        singles.append(bp)
    out = v.compute_running_bias(merged, obs, kta, host=True)
    assert isinstance(out, api.TsVector) and len(out) == n_points
    for j, bp in enumerate(singles):
        r = bp.compute_running_bias(merged[j], obs[j], kta)
        assert np.array_equal(np.array(out[j].values), np.array(r.values))
        assert np.array_equal(v.x[j], bp.state.x)


def test_entries_refuse_a_batch_whose_byte_counts_overflow():
    """T x M and n x n x M are checked before any pointer is touched"""
    from shyft_amd import _native
    L = _native.lib()
    for M, T in ((1 << 62, 8), (1 << 55, 1)):  # T x M x 8 bytes, n x n x M x 8 bytes
        args = (8, M, T, None, None, None, 4.0, 1, None, None, None, None, 1, None, None, None)
        assert L.shyft_hip_kalman_run_host(*args) != 0
        assert b"batch is too large" in L.shyft_hip_last_error(None)
        assert L.shyft_hip_kalman_run(-1, *args) != 0
        assert b"batch is too large" in L.shyft_hip_last_error(None)
