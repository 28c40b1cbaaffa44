"""api.quantile_map_forecast and api.TsVectorSet on the host path (no GPU): qm_main of the reference's
test/qm_test.cpp:385-513, its shyft/tests/api/test_quantile_mapping.py::test_forecast, the argument checks of
core/time_series_dd.cpp:1176-1197 plus the weight check, and the 5- and 6-argument forms."""
import numpy as np
import pytest

from tests import qm_cases as qc


@pytest.fixture(scope="module")
def api():
    from shyft_amd import api
    return api


@pytest.fixture(scope="module")
def main(api):
    return qc.qm_main_inputs(api, np.random.default_rng(56))


def test_qm_main(api, main):
    """qm_test.cpp:441-504: start = end = time(4) of the 6-step axis; four mapped steps, then the scenarios"""
    sets, weights, historical, tah, hist = main
    assert isinstance(sets, api.TsVectorSet) and sets.size() == 3 and [len(s) for s in sets] == [2, 3, 4]
    result = api.quantile_map_forecast(sets, weights, historical, tah, tah.time(4), tah.time(4), False, host=True)
    assert isinstance(result, api.TsVector) and len(result) == 56
    for ts in result:
        assert ts.size() == 6 and ts.point_interpretation() == api.POINT_AVERAGE_VALUE
        assert ts.time(0) == tah.time(0) and ts.time(5) == tah.time(5)
    qc.check_qm_main(result, hist)


def test_qm_main_interpolated_quantiles(api, main):
    """qm_test.cpp:505-512: both interpolated-quantile calls keep the scenarios after the mapped period"""
    sets, weights, historical, tah, hist = main
    result = api.quantile_map_forecast(sets, weights, historical, tah, tah.time(4), tah.time(4), True, host=True)
    qc.check_historical_tail(result, hist)
    # the lowest and the highest rank are flat: the lowest and the highest forecast of the step
    lo, hi = int(np.argmin(hist[:, 0])), int(np.argmax(hist[:, 0]))
    assert result[lo].value(0) == -45.2 and result[hi].value(0) == 83.1
    result = api.quantile_map_forecast(sets, weights, historical, tah, tah.time(3), tah.time(4), True, host=True)
    qc.check_historical_tail(result, hist)
    assert all(np.isfinite(ts.value(t)) for ts in result for t in range(6))


def test_forecast_shapes(api, main):
    """shyft/tests/api/test_quantile_mapping.py::test_forecast: scenarios on the 4-step forecast axis"""
    sets, weights, _, _, _ = main
    ta = api.TimeAxis(api.Calendar().time(2017, 1, 1), api.deltahours(24), 4)
    historical = api.TsVector()
    rng = np.random.default_rng(4)
    for _ in range(56):
        historical.append(api.TimeSeries(ta, api.DoubleVector.from_numpy(rng.random(ta.size()) * 50.0),
                                         api.point_interpretation_policy.POINT_AVERAGE_VALUE))
    result = api.quantile_map_forecast(sets, weights, historical, ta, ta.time(2), ta.time(3), False, host=True)
    assert result is not None
    assert len(result) == 56
    for ts in result:
        assert ts.size() == ta.size()


def test_five_and_six_argument_forms(api, main):
    sets, weights, historical, tah, hist = main
    full = api.quantile_map_forecast(sets, weights, historical, tah, tah.time(2), api.no_utctime, False, host=True)
    five = api.quantile_map_forecast(sets, weights, historical, tah, tah.time(2), host=True)
    for a, b in zip(full, five):
        assert np.array_equal(a.values.to_numpy(), b.values.to_numpy(), equal_nan=True)
    seven = api.quantile_map_forecast(sets, weights, historical, tah, tah.time(1), tah.time(3), False, host=True)
    six = api.quantile_map_forecast(sets, weights, historical, tah, tah.time(1), tah.time(3), host=True)
    for a, b in zip(seven, six):
        assert np.array_equal(a.values.to_numpy(), b.values.to_numpy(), equal_nan=True)
    # the end of the interpolation period defaults to the end of the forecasts (time(4)): steps 2 and 3 blend with
    # weights 0 and 1/2, and step 4 on is the scenario
    plain = api.quantile_map_forecast(sets, weights, historical, tah, api.no_utctime, host=True)
    for k in range(56):
        own = historical[k].average(tah)  # the scenario as the mapping sees it
        assert five[k].value(2) == (1.0 - 0.0) * plain[k].value(2) + 0.0 * own.value(2)
        assert five[k].value(3) == (1.0 - 0.5) * plain[k].value(3) + 0.5 * own.value(3)
    qc.check_historical_tail(five, hist)
    assert not np.array_equal(six[0].values.to_numpy(), five[0].values.to_numpy())


def test_ts_vector_set(api, main):
    sets = main[0]
    clone = api.TsVectorSet(sets)
    assert clone.size() == 3 and all(isinstance(x, api.TsVector) for x in clone)
    assert clone[0] is not sets[0] and clone[0][0] is sets[0][0]
    clone.append(api.TsVector())
    assert len(clone) == 4 and len(sets) == 3
    assert api.TsVectorSet().size() == 0


def test_argument_errors(api, main):
    """time_series_dd.cpp:1176-1197, same conditions; then the weight check"""
    sets, weights, historical, tah, _ = main
    t = tah.time(2)
    with pytest.raises(RuntimeError, match="forecast_set must contain at least one forecast"):
        api.quantile_map_forecast(api.TsVectorSet(), api.DoubleVector(), historical, tah, t, host=True)
    with pytest.raises(RuntimeError, match="historical_data should have more than one time-series"):
        api.quantile_map_forecast(sets, weights, api.TsVector(historical[:1]), tah, t, host=True)
    with pytest.raises(RuntimeError, match=r"The size of weights \(2\), must match number of forecast-sets \(3\)"):
        api.quantile_map_forecast(sets, api.DoubleVector([1.0, 2.0]), historical, tah, t, host=True)
    with pytest.raises(RuntimeError, match="time-axis should have at least one step"):
        api.quantile_map_forecast(sets, weights, historical, api.TimeAxis(tah.time(0), 3600, 0), t, host=True)
    end = tah.total_period()[1]
    for bad in (tah.time(0) - 1, end):  # the period is half open
        with pytest.raises(RuntimeError, match="interpolation_start .* is not within time_axis period"):
            api.quantile_map_forecast(sets, weights, historical, tah, bad, host=True)
        with pytest.raises(RuntimeError, match="interpolation_end .* is not within time_axis period"):
            api.quantile_map_forecast(sets, weights, historical, tah, t, bad, host=True)
    # an end outside the axis is not looked at without a start (:1184)
    api.quantile_map_forecast(sets, weights, historical, tah, api.no_utctime, end, host=True)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="every set weight must be finite and > 0"):
            api.quantile_map_forecast(sets, api.DoubleVector([5.0, bad, 3.0]), historical, tah, t, host=True)
