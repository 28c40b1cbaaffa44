"""Quantile mapping on the host path (no GPU): shyft_hip_quantile_map_host against the literal Python restatement of
core/time_series_qm.h in tests/qm_cases.py, exactly; the reference's known answers of test/qm_test.cpp with its
values restated; and the restated accumulate_stair_case / accumulate_linear (core/time_series_average.h:105-275)."""
import numpy as np
import pytest

from tests import qm_cases as qc

NAN = float("nan")
SIZES = (1, 2, 3, 5, 64, 65)


@pytest.fixture(scope="module")
def api():
    from shyft_amd import api
    return api


@pytest.fixture(scope="module")
def region():
    from shyft_amd import region
    return region


# ---- host entry == literal restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("interpolated", (False, True), ids=("plain", "interp"))
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("F", SIZES)
def test_host_equals_literal_restatement(region, F, P, interpolated):
    """T = 9 holds every mode three times and every hazard step of qc.make_case; B = 2"""
    fc, w, pri, mode, iw = qc.make_case(2, 9, F, P, 7000 + 100 * F + P)
    got = qc.branches(fc, pri, mode)
    assert {"prior", "no_forecast", "no_scenario", "qm", "qm_blend", "one_scenario"} <= got, got
    assert set(mode.tolist()) == {qc.PRIOR, qc.QM, qc.QM_BLEND}
    if F >= 2:
        assert fc[0, 4, 0] == fc[0, 4, F - 1] and w[0] != w[F - 1]  # a value tie with unequal weights
        assert np.signbit(fc[0, 6, F - 1]) and not np.signbit(fc[0, 6, 0]) and fc[0, 6, 0] == 0.0  # -0.0 and +0.0
    if F >= 3:
        assert np.isinf(fc[:, 7]).any() and np.isnan(fc[:, 7]).any() and np.isfinite(fc[:, 7]).any()
    if P >= 3:
        assert np.isinf(pri[:, 7]).any() and np.isnan(pri[:, 7]).any()
    want = qc.quantile_mapping(fc, w, pri, mode, iw, interpolated)
    have = region.quantile_map(fc, w, pri, mode, iw, interpolated=interpolated, host=True)
    assert np.array_equal(have, want, equal_nan=True)
    # zeros tie: the sign of a copied or mapped zero is that of the literal restatement too
    assert np.array_equal(np.signbit(have), np.signbit(want))


def test_two_dimensional_input_is_one_problem(region):
    fc, w, pri, mode, iw = qc.make_case(1, 9, 5, 7, 1)
    a = region.quantile_map(fc, w, pri, mode, iw, host=True)
    b = region.quantile_map(fc[0], w, pri[0], mode, iw, host=True)
    assert a.shape == (1, 9, 7) and b.shape == (9, 7)
    assert np.array_equal(a[0], b, equal_nan=True)


def test_empty_batches_and_refusals(region):
    from shyft_amd._native import ShyftHipError
    fc, w, pri, mode, iw = qc.make_case(1, 3, 4, 5, 2)
    assert region.quantile_map(fc[:, :0], w, pri[:, :0], mode[:0], iw[:0], host=True).shape == (1, 0, 5)
    assert region.quantile_map(fc, w, pri[:, :, :0], mode, iw, host=True).shape == (1, 3, 0)
    # no forecast at all: every step keeps its scenarios
    out = region.quantile_map(fc[:, :, :0], w[:0], pri, mode, iw, host=True)
    assert np.array_equal(out, pri, equal_nan=True)
    for bad in (0.0, -1.0, NAN, float("inf")):
        w2 = w.copy()
        w2[2] = bad
        with pytest.raises(ShyftHipError, match="every weight must be finite and > 0"):
            region.quantile_map(fc, w2, pri, mode, iw, host=True)
    with pytest.raises(ShyftHipError, match="mode must be"):
        region.quantile_map(fc, w, pri, [0, 3, 1], iw, host=True)
    with pytest.raises(ValueError):
        region.quantile_map(fc, w[:3], pri, mode, iw, host=True)
    with pytest.raises(ValueError):
        region.quantile_map(fc, w, pri, mode[:2], iw, host=True)


# ---- test/qm_test.cpp, values restated -------------------------------------------------------------------------------
FC4 = np.array([[14.2, 13.0, 15.8, 9.1], [4.1, 2.9, 20.4, 11.2]])  # qm_test.cpp:69-72, [step][forecast]
W4 = [5.0, 2.0, 2.0, 1.0]


def _quantiles(region, fc, w, n_q, interpolated):
    """n_q quantiles per step: scenario i has rank i, so a QM step returns quantile i at i"""
    T = fc.shape[0]
    pri = np.tile(np.arange(n_q, dtype=np.float64), (T, 1))
    return region.quantile_map(fc, w, pri, [qc.QM] * T, [0.0] * T, interpolated=interpolated, host=True)


def test_compute_weighted_quantiles(region):
    """qm_test.cpp:60-114"""
    q = _quantiles(region, FC4, W4, 100, False)
    for i in range(100):
        assert q[0, i] == (9.1 if i <= 9 else 13.0 if i <= 29 else 14.2 if i <= 79 else 15.8), i
        assert q[1, i] == (2.9 if i <= 19 else 4.1 if i <= 69 else 11.2 if i <= 79 else 20.4), i


def test_interpolated_weighted_quantiles(region):
    """qm_test.cpp:116-152: ends exact, interior to the reference's delta"""
    q = _quantiles(region, FC4, W4, 5, True)
    want = ((9.1, 13.171428571428571, 14.028571428571428, 15.114285714285714, 15.8),
            (2.9, 3.4142857142857141, 5.2833333333333332, 11.2, 20.4))
    for t in range(2):
        assert q[t, 0] == want[t][0] and q[t, 4] == want[t][4]
        for i in (1, 2, 3):
            assert abs(q[t, i] - want[t][i]) <= 1e-15, (t, i, q[t, i])


def test_quantile_mapping(region):
    """qm_test.cpp:154-227: 43 priors of random values, five weighted forecasts"""
    fc = np.array([[32.1, 21.0, 10.2, 71.0, 35.4], [1.2, 34.2, 12.4, 89.2, 83.4]])
    w = [39.0, 32.0, 8.0, 73.0, 14.0]
    pri = np.random.default_rng(43).random((2, 43)) * 50.0
    out = region.quantile_map(fc, w, pri, [qc.QM, qc.QM], [0.0, 0.0], host=True)
    o0, o1 = np.argsort(pri[0], kind="stable"), np.argsort(pri[1], kind="stable")
    for i in range(43):
        assert out[0, o0[i]] == (10.2 if i < 3 else 21.0 if i < 11 else 32.1 if i < 20 else 35.4 if i < 24 else 71.0), i
        assert out[1, o1[i]] == (1.2 if i < 10 else 12.4 if i < 12 else 34.2 if i < 20 else 83.4 if i < 24 else 89.2), i


def _const_tsv(api, ta, values):
    tsv = api.TsVector()
    for v in values:
        tsv.append(api.TimeSeries(ta, float(v), api.POINT_AVERAGE_VALUE))
    return tsv


def test_quantile_mapping_interp(api):
    """qm_test.cpp:229-301: two unit-weight forecasts 5 and 20, 18 priors of value i, interpolation from step 9 to
    the last step of the axis: the blend (1 - w) q + w i with w = (t - 9) / 4, exact"""
    ta = api.TimeAxis(api.Calendar().time(2017, 1, 1), api.deltahours(24), 14)
    sets = api.TsVectorSet()
    sets.append(_const_tsv(api, ta, (5.0, 20.0)))
    result = api.quantile_map_forecast(sets, [1.0], _const_tsv(api, ta, range(18)), ta, ta.time(9), host=True)
    assert len(result) == 18
    for i in range(18):
        q = 5.0 if i < 9 else 20.0
        for t in range(14):
            if t < 9:
                assert result[i].value(t) == q, (i, t)
            else:
                weight = (t - 9) / 4.0
                assert result[i].value(t) == (1.0 - weight) * q + weight * i, (i, t)


def test_qm_partial_prognoses(api):
    """qm_test.cpp:303-383: forecasts of length 2, 3 and 4 on a 6-step axis, no interpolation"""
    t0 = api.Calendar().time(2017, 1, 1)
    day = api.deltahours(24)
    sets = api.TsVectorSet()
    fcs = api.TsVector()
    for i, n in enumerate((2, 3, 4)):
        fcs.append(api.TimeSeries(api.TimeAxis(t0, day, n), float(i + 1), api.POINT_AVERAGE_VALUE))
    sets.append(fcs)
    ta = api.TimeAxis(t0, day, 6)
    result = api.quantile_map_forecast(sets, [1.0], _const_tsv(api, ta, range(9)), ta, api.no_utctime, host=True)
    for i in range(9):
        for t in range(2):
            assert result[i].value(t) == (1.0 if i < 3 else 2.0 if i < 6 else 3.0), (i, t)
        assert result[i].value(2) == (2.0 if i < 5 else 3.0), i
        assert result[i].value(3) == 3.0, i
        for t in (4, 5):  # past every forecast: the scenario itself
            assert result[i].value(t) == float(i), (i, t)


# ---- accumulate_stair_case / accumulate_linear, avg ------------------------------------------------------------------
T0, H = 1483228800, 3600  # 2017-01-01
# accumulate_linear evaluates a*t + b at absolute tick times: t is about 1.5e15 microseconds and a = dv / 3.6e9 per
# tick, so a*t is about 4e5 * dv and one rounding of it is 4e5 * dv * 2.2e-16 = 1e-10 * dv; dv <= 12 here and a value
# takes fewer than ten such roundings
LINEAR_ATOL = 1e-8


@pytest.mark.parametrize("fx", ("POINT_AVERAGE_VALUE", "POINT_INSTANT_VALUE"))
def test_accumulate_on_the_series_own_axis(api, fx):
    """stair-case: its own values; linear: the mean of the two ends of each interval, NaN in the last (no right end)"""
    ta = api.TimeAxis(T0, H, 6)
    v = [1.0, 3.0, 2.0, 8.0, -4.0, 0.5]
    got = api._api._accumulate(api.TimeSeries(ta, v, getattr(api, fx))._ts, ta, True)
    if fx == "POINT_AVERAGE_VALUE":
        assert got.tolist() == v
    else:
        assert np.allclose(got[:5], [(v[i] + v[i + 1]) / 2 for i in range(5)], rtol=0, atol=LINEAR_ATOL)
        assert np.isnan(got[5])


def test_accumulate_two_to_one_coarsening(api):
    ta = api.TimeAxis(T0, H, 6)
    v = [1.0, 3.0, 2.0, 8.0, -4.0, 0.5]
    got = api._api._accumulate(api.TimeSeries(ta, v, api.POINT_AVERAGE_VALUE)._ts, api.TimeAxis(T0, 2 * H, 3), True)
    assert got.tolist() == [2.0, 5.0, -1.75]
    got = api._api._accumulate(api.TimeSeries(ta, v, api.POINT_INSTANT_VALUE)._ts, api.TimeAxis(T0, 2 * H, 3), True)
    # pieces (1+3)/2, (3+2)/2 | (2+8)/2, (8-4)/2 | (-4+0.5)/2 over the one hour that has a right end
    assert np.allclose(got, [2.25, 3.5, -1.75], rtol=0, atol=LINEAR_ATOL)


def test_accumulate_nan_point_shortens_the_span(api):
    """time_series_average.h:56-78: a NaN point contributes nothing, and for a linear series the piece before it has
    no right end either; the average is over what remains"""
    ta = api.TimeAxis(T0, H, 6)
    v = [1.0, 3.0, NAN, 8.0, -4.0, 0.5]
    coarse = api.TimeAxis(T0, 3 * H, 2)
    got = api._api._accumulate(api.TimeSeries(ta, v, api.POINT_AVERAGE_VALUE)._ts, coarse, True)
    assert got.tolist() == [2.0, 1.5]  # (1 + 3) / 2 over two hours; (8 - 4 + 0.5) / 3
    got = api._api._accumulate(api.TimeSeries(ta, v, api.POINT_INSTANT_VALUE)._ts, coarse, True)
    assert np.allclose(got, [2.0, (2.0 - 1.75) / 2], rtol=0, atol=LINEAR_ATOL)  # [0,1h): 2; [3h,4h): 2, [4h,5h): -1.75
    # integral instead of average: seconds
    got = api._api._accumulate(api.TimeSeries(ta, v, api.POINT_AVERAGE_VALUE)._ts, coarse, False)
    assert np.allclose(got, [4.0 * H, 4.5 * H], rtol=0, atol=LINEAR_ATOL)


@pytest.mark.parametrize("fx", ("POINT_AVERAGE_VALUE", "POINT_INSTANT_VALUE"))
def test_accumulate_series_ending_inside_the_axis(api, fx):
    ts = api.TimeSeries(api.TimeAxis(T0, H, 3), [1.0, 2.0, 4.0], getattr(api, fx))
    got = api._api._accumulate(ts._ts, api.TimeAxis(T0, H, 6), True)
    assert np.isnan(got[3:]).all()
    if fx == "POINT_AVERAGE_VALUE":
        assert got[:3].tolist() == [1.0, 2.0, 4.0]
    else:
        assert np.allclose(got[:2], [1.5, 3.0], rtol=0, atol=LINEAR_ATOL) and np.isnan(got[2])
    # entirely before or after the axis
    assert np.isnan(api._api._accumulate(ts._ts, api.TimeAxis(T0 + 10 * H, H, 2), True)).all()
    assert np.isnan(api._api._accumulate(ts._ts, api.TimeAxis(T0 - 10 * H, H, 2), True)).all()
