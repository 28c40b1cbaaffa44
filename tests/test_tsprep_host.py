"""Rating curve, ice packing, ice-packing recession and min-max linear fill on the host entries
(shyft_hip_ts_*_host, host=True; host/ts_prep.hpp): the reference's own test numbers restated as data, the host
against the plain-Python transcriptions of tests/tsprep_cases.py on random batches, and the refusals. No GPU."""
import math

import numpy as np
import pytest

from shyft_amd import api, region
from tests import resample_cases as rc
from tests import tsprep_cases as tc

NAN = float("nan")


def _nan_places(x):
    return [i for i, y in enumerate(x) if not math.isfinite(y)]


# ---- the reference's numbers ---------------------------------------------------------------------------------------------
def _ice_case_temperature():
    """test/test_ice_packing.cpp:22-27, 80-85"""
    ta = api.TimeAxis(0, 3600, 24)
    v = [0.0] * 24
    v[2], v[3], v[4], v[10] = -10.0, -20.0, -15.0, NAN
    return api.TimeSeries(ta, v, api.POINT_AVERAGE_VALUE)


def test_ice_packing_detection_cases_of_the_reference():
    """test/test_ice_packing.cpp:19-70"""
    temperature = _ice_case_temperature()
    ipp = api.IcePackingParameters(api.deltahours(2), -10.0)
    pol = api.ice_packing_temperature_policy
    disallow = temperature.ice_packing(ipp, pol.DISALLOW_MISSING).values
    initial = temperature.ice_packing(ipp, pol.ALLOW_INITIAL_MISSING).values
    any_missing = temperature.ice_packing(ipp, pol.ALLOW_ANY_MISSING).values
    assert len(disallow) == 24
    assert _nan_places(disallow) == [0, 1, 11, 12]
    assert disallow[13] == 0.0
    assert initial[:7] == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0]
    assert initial[9] == 0.0 and initial[10] == 0.0
    assert _nan_places(initial) == [11, 12]
    assert initial[13] == 0.0 and initial[23] == 0.0
    assert any_missing[0] == 0.0 and any_missing[1] == 0.0
    assert any_missing[11] == 0.0 and any_missing[12] == 0.0
    assert temperature.ice_packing(ipp, pol.DISALLOW_MISSING).point_interpretation() == api.POINT_AVERAGE_VALUE


def test_ice_packing_recession_case_of_the_reference():
    """test/test_ice_packing.cpp:71-117"""
    temperature = _ice_case_temperature()
    ice_pack = temperature.ice_packing(api.IcePackingParameters(api.deltahours(2), -10.0),
                                       api.ice_packing_temperature_policy.ALLOW_ANY_MISSING)
    flow = api.TimeSeries(api.TimeAxis(0, 3600, 24), [10.0 + i for i in range(24)], api.POINT_AVERAGE_VALUE)
    ipr = api.IcePackingRecessionParameters(1 / 3600.0, 0.75)
    fixed = flow.ice_packing_recession(ice_pack, ipr)
    assert fixed.point_interpretation() == api.POINT_AVERAGE_VALUE
    for i in range(24):
        e = 10.0 + i
        if i == 4:
            e = 0.75 + ((10.0 + (i - 1)) - 0.75) * math.exp(-ipr.alpha * 3600.0)
        elif i == 5:
            e = 0.75 + ((10.0 + (i - 2)) - 0.75) * math.exp(-ipr.alpha * 7200.0)
        assert fixed.value(i) == pytest.approx(e, rel=1e-12), i


def test_ice_packing_of_an_instant_value_series():
    """shyft/tests/api/test_time_series.py:1103-1130"""
    t0 = api.Calendar().time(2018, 1, 1)
    ta = api.TimeAxis(t0, api.deltaminutes(30), 10)
    data = np.linspace(-5, 5, len(ta))
    data[len(ta) // 2] = NAN
    ts = api.TimeSeries(ta, data, api.POINT_INSTANT_VALUE)
    ipp = api.IcePackingParameters(threshold_window=api.deltahours(1), threshold_temperature=0.0)
    got = ts.ice_packing(ipp, api.ice_packing_temperature_policy.ALLOW_INITIAL_MISSING)
    assert len(got) == len(ts)
    assert [got.time(i) for i in range(10)] == [ts.time(i) for i in range(10)]
    expected = np.array([0, 1, 1, 1, 1, NAN, NAN, NAN, 0, 0])
    assert np.array_equal(expected, np.asarray(got.values), equal_nan=True)


def test_rating_curve_ts_with_two_curves():
    """shyft/tests/api/test_time_series.py:1031-1067, exact equality"""
    t0 = api.Calendar().time(2018, 7, 1)
    ta = api.TimeAxis(t0, api.deltaminutes(30), 48 * 2)
    data = np.linspace(0, 10, ta.size())
    ts = api.TimeSeries(ta, data, api.POINT_INSTANT_VALUE)
    rcf1 = api.RatingCurveFunction()
    rcf1.add_segment(0, 1, 0, 1)
    rcf1.add_segment(api.RatingCurveSegment(5, 2, 0, 1))
    rcf2 = api.RatingCurveFunction()
    rcf2.add_segment(0, 3, 0, 1)
    rcf2.add_segment(api.RatingCurveSegment(8, 4, 0, 1))
    rcp = api.RatingCurveParameters()
    rcp.add_curve(t0, rcf1)
    assert rcp.add_curve(t0 + api.deltahours(24), rcf2) is rcp
    got = ts.rating_curve(rcp)
    assert len(got) == len(ts) and got.point_interpretation() == api.POINT_INSTANT_VALUE
    for i in range(got.size()):
        v, t = ts.value(i), ts.time(i)
        expected = (1 * v if v < 5 else 2 * v) if t < t0 + api.deltahours(24) else (3 * v if v < 8 else 4 * v)
        assert got.time(i) == t
        assert got.value(i) == expected
        assert rcp.flow(t, v) == expected
    assert list(rcp.flow(ts)) == list(got.values)
    assert math.isnan(rcp.flow(t0 - 1, 3.0))                  # before the first curve
    assert math.isnan(api.RatingCurveParameters().flow(t0, 3.0))  # no curves
    assert all(math.isnan(x) for x in ts.rating_curve(api.RatingCurveParameters()).values)


def test_min_max_check_linear_fill_case_of_the_reference():
    """shyft/tests/api/test_time_series.py:1295-1305"""
    ta = api.TimeAxis(0, 1, 5)
    ts_src = api.TimeSeries(ta, values=api.DoubleVector([1.0, -1.0, 2.0, NAN, 4.0]), point_fx=api.POINT_AVERAGE_VALUE)
    ts_qac = ts_src.min_max_check_linear_fill(v_max=10.0, v_min=-10.0, dt_max=300)
    assert ts_qac.value(3) == pytest.approx(3.0)
    assert ts_qac.point_interpretation() == api.POINT_AVERAGE_VALUE
    ts_qac = ts_src.min_max_check_linear_fill(v_max=10.0, v_min=0.0, dt_max=300)
    assert ts_qac.value(1) == pytest.approx(1.5)
    assert ts_qac.value(3) == pytest.approx(3.0)
    ts_qac = ts_src.min_max_check_linear_fill(v_max=10.0, v_min=0.0, dt_max=0)
    assert not math.isfinite(ts_qac.value(3))
    assert not math.isfinite(ts_qac.value(1))
    ts_qac = ts_src.min_max_check_linear_fill(v_min=0.0, v_max=10.0)  # the default dt_max is max_utctime, clamped
    assert ts_qac.value(1) == pytest.approx(1.5)


def test_parameter_classes():
    """shyft/tests/api/test_time_series.py:1072-1100"""
    p = api.IcePackingParameters(3600 * 24 * 7, -15.0)
    assert p.threshold_window == 3600 * 24 * 7 and p.threshold_temperature == -15.0
    q = api.IcePackingParameters(threshold_temperature=-10.2, threshold_window=3600 * 24 * 10)
    assert q.threshold_window == 3600 * 24 * 10 and q.threshold_temperature == -10.2
    assert not q == p and p == p and p != q
    q.threshold_temperature = p.threshold_temperature
    q.threshold_window = p.threshold_window
    assert p == q and not p != q
    iprp = api.IcePackingRecessionParameters(alpha=0.0001, recession_minimum=0.25)
    assert iprp.alpha == 0.0001 and iprp.recession_minimum == 0.25
    iprp.alpha *= 2
    iprp.recession_minimum *= 4
    assert iprp.alpha == 0.0001 * 2 and iprp.recession_minimum == 0.25 * 4
    iprp2 = api.IcePackingRecessionParameters(alpha=0.0001, recession_minimum=0.25)
    assert iprp != iprp2 and not iprp == iprp2 and iprp == iprp and not iprp != iprp
    pol = api.ice_packing_temperature_policy
    assert (int(pol.DISALLOW_MISSING), int(pol.ALLOW_INITIAL_MISSING), int(pol.ALLOW_ANY_MISSING)) == (0, 1, 2)


def test_rating_curve_segment():
    """shyft/tests/api/test_rating_curve.py:10-24"""
    rcs = api.RatingCurveSegment(lower=0.0, a=1.0, b=2.0, c=3.0)
    assert (rcs.lower, rcs.a, rcs.b, rcs.c) == (0.0, 1.0, 2.0, 3.0)
    assert rcs.valid(0.0) and rcs.valid(1.0) and not rcs.valid(-0.1)
    for level in range(10):
        assert rcs.flow(level) == pytest.approx(1.0 * pow(level - 2.0, 3.0), rel=1e-14, abs=1e-300)
    flows = rcs.flow([i for i in range(10)])
    for i in range(10):
        assert flows[i] == pytest.approx(pow(float(i) - 2.0, 3.0), rel=1e-14, abs=1e-300)
    assert list(rcs.flow(list(range(10)), 2, 5)) == list(flows[2:5])
    assert rcs == api.RatingCurveSegment(0.0, 1.0, 2.0, 3.0) and rcs != api.RatingCurveSegment(0.0, 1.0, 2.0, 3.5)


def test_rating_curve_function():
    """shyft/tests/api/test_rating_curve.py:26-44"""
    rcf = api.RatingCurveFunction()
    assert rcf.size() == 0
    rcf.add_segment(api.RatingCurveSegment(lower=0.0, a=1.0, b=2.0, c=3.0))
    rcf.add_segment(10.0, 1.0, 2.0, 3.0)
    assert rcf.size() == 2
    assert rcf.flow(4.0) == pytest.approx(8.0, rel=1e-14)
    assert rcf.flow([4.0])[0] == pytest.approx(8.0, rel=1e-14)
    assert len(str(rcf)) > 10
    assert sum(s.lower for s in rcf) == 10.0
    assert math.isnan(rcf.flow(-1.0)) and math.isnan(rcf.flow(NAN))   # below the first segment
    rcf.add_segment(5.0, 2.0, 0.0, 1.0)                              # inserted by upper_bound
    assert [s.lower for s in rcf] == [0.0, 5.0, 10.0]
    assert rcf.flow(5.0) == 10.0 and rcf.flow(7.0) == 14.0           # exactly on a lower, and inside
    unsorted = api.RatingCurveFunction([api.RatingCurveSegment(5, 2, 0, 1), api.RatingCurveSegment(0, 1, 0, 1)], False)
    assert [s.lower for s in unsorted] == [0.0, 5.0]


# ---- the host against the transcriptions ---------------------------------------------------------------------------------
BATCHES = [(11, rc.EPOCHS[0], 1), (9, rc.EPOCHS[1], 2), (10, rc.EPOCHS[2], 3)]


@pytest.mark.parametrize("S,epoch,seed", BATCHES)
def test_ice_packing_equals_the_transcription_bit_for_bit(S, epoch, seed):
    t0, dt = epoch
    batch = rc.make_batch(S, t0, dt, seed, lengths=(0, 1, 2, 3, 17, 40), min_points=0)
    row, t = batch[0], batch[1]
    for w, window in enumerate((0, dt // 3, dt, 5 * dt // 2, 100 * dt)):
        policy = np.array([(s + w) % 3 for s in range(S)], np.int32)
        # a one-point series under DISALLOW_MISSING with a window over its point is refused (point_dt::time throws)
        for s in range(S):
            if row[s + 1] - row[s] == 1 and policy[s] == 0:
                policy[s] = 1
        thr = np.array([0.0, 5.0, -3.0][w % 3] + np.zeros(S))
        win = np.full(S, window, np.int64)
        got = region.ts_ice_packing_csr(*batch, row, t, win, thr, policy, host=True)
        assert rc.same_bits(got, tc.ice_packing(batch, row, t, win, thr, policy))
        # a foreign axis shifted by a quarter spacing, from before the series to past its end
        qrow, qt = [0], []
        for s in range(S):
            n = int(row[s + 1] - row[s])
            qt.extend(t0 - 2 * dt + dt // 4 + dt * k for k in range(n + 5))
            qrow.append(len(qt))
        got = region.ts_ice_packing_csr(*batch, qrow, qt, win, thr, policy, host=True)
        assert rc.same_bits(got, tc.ice_packing(batch, qrow, qt, win, thr, policy))


@pytest.mark.parametrize("S,epoch,seed", BATCHES)
def test_min_max_fill_equals_the_transcription_bit_for_bit(S, epoch, seed):
    t0, dt = epoch
    batch = rc.make_batch(S, t0, dt, seed, lengths=(0, 1, 2, 3, 17, 64, 150))
    for lo, hi, span in ((NAN, NAN, 10**18), (-2.0, 12.0, 3 * dt), (0.0, NAN, 2 * dt), (NAN, 8.0, 0), (-5.0, 15.0, dt)):
        args = (np.full(S, lo), np.full(S, hi), np.full(S, span, np.int64))
        got = region.ts_min_max_fill_csr(*batch, *args, host=True)
        assert rc.same_bits(got, tc.min_max_fill(batch, *args))


@pytest.mark.parametrize("S,epoch,seed", BATCHES)
def test_rating_curve_is_within_4_ulp_of_the_transcription(S, epoch, seed):
    """detmath::pow is within 2 ulp of the true power and the libm within 1 ulp; the product rounds once in each"""
    t0, dt = epoch
    batch = rc.make_batch(S, t0, dt, seed, lengths=(0, 1, 2, 3, 17, 64, 150))
    packs = tc.make_packs(4, t0, dt, seed)
    pack_of = np.arange(S) % 4
    got = region.ts_rating_curve_csr(*batch, *tc.packs_csr(packs), pack_of, host=True)
    row, t, v = batch[0], batch[1], batch[2]
    n_flow = 0
    for s in range(S):
        for k in range(int(row[s]), int(row[s + 1])):
            seg = tc.rating_segment(packs[pack_of[s]], int(t[k]), float(v[k]))
            if seg is None:
                assert math.isnan(got[k]), (s, k)
                continue
            lower, a, b, c = seg
            base = float(v[k]) - b
            if base < 0 and c != int(c):
                assert math.isnan(got[k]), (s, k)  # a negative base with a fractional exponent
                continue
            e = a * math.pow(base, c)
            if math.isinf(e) or e == 0.0:
                assert got[k] == e, (s, k)
            else:
                assert tc.ulp_distance(got[k], e) <= 4, (s, k, got[k], e)
                n_flow += 1
    assert n_flow > 20


@pytest.mark.parametrize("S,epoch,seed", BATCHES)
def test_recession_is_within_the_bound_of_the_transcription(S, epoch, seed):
    """exp within 1 ulp on each side, one product and one sum: 4 * 2**-52 * (|qbf| + |qs - qbf|)"""
    t0, dt = epoch
    batch = rc.make_batch(S, t0, dt, seed, lengths=(0, 1, 2, 3, 17, 64, 150, 257))
    ice = tc.indicator(batch, seed)
    row, t_end = batch[0], batch[3]
    starts = np.array([batch[1][row[s]] if row[s + 1] > row[s] else 0 for s in range(S)], np.int64)
    for alpha, qbf in ((1 / (7 * 86400.0), 0.75), (0.0, 2.0), (1 / 3600.0, 1e3)):
        got = region.ts_ice_packing_recession_csr(*batch, ice, starts, t_end, alpha, qbf, host=True)
        for s in range(S):
            t, v, _, fx = tc.series(batch, s)
            x = [float(y) for y in ice[row[s]:row[s + 1]]]
            for i in range(len(t)):
                e, qs = tc.recession_terms(t, v, fx, x, alpha, qbf, i)
                g = got[row[s] + i]
                if qs is None or not math.isfinite(e):
                    assert rc.same_bits(np.array([g]), np.array([e])), (s, i, g, e)
                else:
                    assert abs(g - e) <= 4 * 2.0**-52 * (abs(qbf) + abs(qs - qbf)), (s, i, g, e)


# ---- refusals ------------------------------------------------------------------------------------------------------------
ONE_CURVE = ([0, 1], [0], [0, 1], [[0.0, 1.0, 0.0, 1.0]])


def test_refusals_and_their_texts():
    two = ([0, 2], [0, 10], [1.0, 2.0], [20], [0])
    decreasing = ([0, 2], [10, 0], [1.0, 2.0], [20], [0])
    text = "needs time-points in increasing order"
    with pytest.raises(RuntimeError, match=text):
        region.ts_min_max_fill_csr(*decreasing, NAN, NAN, 10, host=True)
    with pytest.raises(RuntimeError, match=text):
        region.ts_rating_curve_csr(*decreasing, *ONE_CURVE, host=True)
    with pytest.raises(RuntimeError, match=text):
        region.ts_ice_packing_csr(*decreasing, [0, 2], [10, 0], 5, 0.0, 0, host=True)
    with pytest.raises(RuntimeError, match=text):
        region.ts_ice_packing_recession_csr(*decreasing, [0.0, 0.0], 0, 20, 0.0, 0.0, host=True)
    with pytest.raises(RuntimeError, match="illegal end-of-axis"):
        region.ts_min_max_fill_csr([0, 2], [0, 10], [1.0, 2.0], [10], [0], NAN, NAN, 10, host=True)
    with pytest.raises(RuntimeError, match="row must not decrease"):
        region.ts_min_max_fill_csr([0, 2, 1, 2], [0, 10], [1.0, 2.0], [20, 20, 20], [0, 0, 0], NAN, NAN, 10, host=True)
    with pytest.raises(RuntimeError, match="quarter of the 64-bit range"):
        region.ts_min_max_fill_csr([0, 2], [0, 2**62], [1.0, 2.0], [2**62 + 1], [0], NAN, NAN, 10, host=True)
    with pytest.raises(RuntimeError, match="total period of flow ts should equal or be contained in ice packing ts"):
        region.ts_ice_packing_recession_csr(*two, [0.0, 1.0], 0, 19, 0.0, 0.0, host=True)
    with pytest.raises(RuntimeError, match="total period of flow ts should equal or be contained in ice packing ts"):
        region.ts_ice_packing_recession_csr(*two, [0.0, 1.0], 1, 20, 0.0, 0.0, host=True)
    with pytest.raises(RuntimeError, match="no rating-curve segments"):
        region.ts_rating_curve_csr(*two, [0, 1], [0], [0, 0], np.empty((0, 4)), host=True)
    # an empty curve that no point of the series uses is not asked, as in the reference
    ok = region.ts_rating_curve_csr(*two, [0, 2], [0, 11], [0, 1, 1], [[0.0, 2.0, 0.0, 1.0]], host=True)
    assert list(ok) == [2.0, 4.0]
    with pytest.raises(RuntimeError, match="no rating-curve segments"):
        api.RatingCurveFunction().flow(1.0)
    with pytest.raises(RuntimeError, match="equal lower"):
        api.RatingCurveFunction([api.RatingCurveSegment(1, 2, 0, 1), api.RatingCurveSegment(1, 3, 0, 1)], False)
    with pytest.raises(RuntimeError, match="a one-point series cannot be integrated"):
        region.ts_ice_packing_csr([0, 1], [10], [1.0], [20], [1], [0, 1], [15], 10, 0.0, 0, host=True)


def test_parameter_sequences_of_the_wrong_length_are_refused():
    ta = api.TimeAxis(0, 3600, 4)
    tsv = api.TsVector(api.TimeSeries(ta, [1.0, 2.0, 3.0, 4.0], api.POINT_AVERAGE_VALUE) for _ in range(3))
    ipp = api.IcePackingParameters(3600, 0.0)
    text = "one per series"
    with pytest.raises(RuntimeError, match=text):
        tsv.ice_packing([ipp, ipp], api.ice_packing_temperature_policy.DISALLOW_MISSING, host=True)
    with pytest.raises(RuntimeError, match=text):
        tsv.rating_curve([api.RatingCurveParameters()] * 4, host=True)
    with pytest.raises(RuntimeError, match=text):
        tsv.min_max_check_linear_fill([0.0, 1.0], 10.0, host=True)
    ice = tsv.ice_packing(ipp, api.ice_packing_temperature_policy.ALLOW_ANY_MISSING, host=True)
    with pytest.raises(RuntimeError, match=text):
        tsv.ice_packing_recession(ice, [api.IcePackingRecessionParameters(0.0, 0.0)] * 2, host=True)
    with pytest.raises(RuntimeError, match="ip_ts holds 2 series"):
        tsv.ice_packing_recession(api.TsVector(ice[:2]), api.IcePackingRecessionParameters(0.0, 0.0), host=True)


def test_empty_batches():
    assert region.ts_min_max_fill_csr([0], [], [], [], [], [], [], [], host=True).shape == (0,)
    assert region.ts_min_max_fill_csr([0, 0], [], [], [5], [0], NAN, NAN, 1, host=True).shape == (0,)
    assert region.ts_ice_packing_csr([0, 2], [0, 10], [1.0, 2.0], [20], [0], [0, 0], [], 5, 0.0, 0, host=True).shape == (0,)
    assert len(api.TsVector().rating_curve(api.RatingCurveParameters(), host=True)) == 0
