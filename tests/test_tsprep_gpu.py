"""The observation-preparation kernels on the GPU (kernels/tsprep.hip): every shyft_hip_ts_* device entry is
bit-identical, NaN matching NaN, to its _host twin (which runs host/ts_prep.hpp and is itself pinned by
tests/test_tsprep_host.py), then the counters and the TsVector methods.

Batches are those of tests/resample_cases.py (S = 1 / 63 / 64 / 65 / 257, lengths rotating over 0, 1, 2, 3, 63, 64, 65,
257, 1000, three time bases, both point types, NaN / inf hazards), so the flat point array spans many scan workgroups
(1024 keys each) and a series starts at every kind of offset; where S allows, series 8 is replaced by one of 3,300
points, more than three workgroup spans, so aggregates are carried over more than one boundary inside one series."""
import numpy as np
import pytest

from tests import resample_cases as rc
from tests import tsprep_cases as tc

pytestmark = pytest.mark.gpu

SS = (1, 63, 64, 65, 257)
N_LONG = 3 * tc.SCAN_SPAN + 228
NAN = float("nan")


@pytest.fixture(scope="module")
def region():
    from shyft_amd import region
    return region


def _batch(S, k):
    t0, dt = rc.EPOCHS[k % len(rc.EPOCHS)]
    if S > 8:
        return t0, dt, tc.long_batch(S, t0, dt, 9100 + S, 8, N_LONG)
    return t0, dt, rc.make_batch(S, t0, dt, 9100 + S, first=7)  # S == 1: one series of 257 points


def _same(dev, host, what):
    bad = np.argwhere(~((np.isnan(dev) & np.isnan(host)) | (dev.view(np.uint64) == host.view(np.uint64))))
    assert rc.same_bits(dev, host), (what, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("k,S", list(enumerate(SS)))
def test_ice_packing_is_bit_identical_to_host(region, k, S):
    t0, dt, batch = _batch(S, k)
    row, t = batch[0], batch[1]
    queries = ((row, t), tc.foreign_axis(batch, t0, dt))
    for w, window in enumerate(tc.ice_windows(dt)):
        policy = tc.ice_policies(batch, w)
        thr = np.full(S, (0.0, 5.0, -3.0)[w % 3])
        for qrow, qt in queries:
            host = region.ts_ice_packing_csr(*batch, qrow, qt, window, thr, policy, host=True)
            dev = region.ts_ice_packing_csr(*batch, qrow, qt, window, thr, policy)
            assert dev.shape == (len(qt),)
            _same(dev, host, (window, len(qt)))
        assert set(np.unique(host[~np.isnan(host)])) <= {0.0, 1.0}


@pytest.mark.parametrize("k,S", list(enumerate(SS)))
def test_recession_is_bit_identical_to_host(region, k, S):
    t0, dt, batch = _batch(S, k)
    row, t_end = batch[0], batch[3]
    ice = tc.indicator(batch, 40 + S)
    if S > 8:  # series 8 is the long one and h == 8: one run of ice over more than two workgroup spans
        assert np.all(ice[row[8] + 3:row[9] - 2] == 1.0) and row[9] - row[8] - 5 > 2 * tc.SCAN_SPAN
    starts = np.array([batch[1][row[s]] if row[s + 1] > row[s] else 0 for s in range(S)], np.int64)
    flows = np.abs(batch[2]) if k % 2 else batch[2]
    b = (batch[0], batch[1], flows, batch[3], batch[4])
    # the reference's parameters, no recession at all (alpha 0), a minimum above every flow
    for alpha, qbf in ((1 / (7 * 86400.0), 0.75), (0.0, 2.0), (1 / 3600.0, 1e3)):
        host = region.ts_ice_packing_recession_csr(*b, ice, starts, t_end, alpha, qbf, host=True)
        dev = region.ts_ice_packing_recession_csr(*b, ice, starts, t_end, alpha, qbf)
        _same(dev, host, (alpha, qbf))
    for ind in (np.zeros_like(ice), np.ones_like(ice)):  # no ice anywhere, ice everywhere
        host = region.ts_ice_packing_recession_csr(*b, ind, starts, t_end, 1e-5, 0.5, host=True)
        _same(region.ts_ice_packing_recession_csr(*b, ind, starts, t_end, 1e-5, 0.5), host, ind[:1])


def test_recession_falls_back_to_the_series_own_first_point(region):
    """ice from point 0 of the second series, whose predecessor ends without ice: qs is its own point 0"""
    hour = rc.HOUR
    row = [0, 3, 7]
    t = [0, hour, 2 * hour, 0, hour, 2 * hour, 3 * hour]
    v = [100.0, 200.0, 300.0, 8.0, 9.0, 10.0, 11.0]
    ice = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0]
    args = (row, t, v, [3 * hour, 4 * hour], [1, 1], ice, 0, 4 * hour, 0.0, 0.0)
    dev = region.ts_ice_packing_recession_csr(*args)
    _same(dev, region.ts_ice_packing_recession_csr(*args, host=True), "fallback")
    assert dev.tolist() == [100.0, 200.0, 300.0, 8.0, 8.0, 8.0, 11.0]  # alpha 0: the flow where the ice began


# One series longer than 256 scan spans: tp_scan_agg_kernel scans the span aggregates 256 at a time and carries the
# running maximum into its second round, which starts at flat position ROUND.
ROUND = 256 * tc.SCAN_SPAN
NP_ROUNDS = ROUND + 1500


def _two_round_series(seed):
    rng = np.random.default_rng(seed)
    t = rc.HOUR * np.arange(NP_ROUNDS, dtype=np.int64)
    return [0, NP_ROUNDS], t, rng.uniform(0.5, 10.0, NP_ROUNDS), [rc.HOUR * NP_ROUNDS], [1]


def test_recession_carries_the_stop_index_into_the_second_round_of_the_aggregate_scan(region):
    """ice runs whose stop index lies in the first 256 spans and whose points lie behind them. One indicator cannot
    hold a run across ROUND and another that starts at ROUND, so there are two; every other run is short, the host walks
    a run of n points in about n^2 / 2 steps."""
    assert tc.SCAN_SPAN == 1024 and ROUND == 262144
    series = _two_round_series(77)
    a = np.zeros(NP_ROUNDS)
    a[261000:263500] = 1.0  # over the span boundaries 255 and 257 and over ROUND; stops at 260999
    a[99] = NAN             # just before a short run: every point of it is lost
    a[100:140] = 1.0
    a[263600:] = 1.0        # to the last point
    b = np.zeros(NP_ROUNDS)
    b[ROUND:ROUND + 60] = 1.0   # starts exactly at ROUND: stops at the last key of the first round
    b[261000:ROUND - 1] = 1.0   # ends one short of it
    b[262999] = NAN
    b[263000:263300] = 1.0      # lost, behind ROUND
    for ice in (a, b):
        args = (*series, ice, 0, rc.HOUR * NP_ROUNDS, 1 / (7 * 86400.0), 0.75)
        dev = region.ts_ice_packing_recession_csr(*args)
        _same(dev, region.ts_ice_packing_recession_csr(*args, host=True), int(ice[ROUND]))
    assert np.isfinite(dev[ROUND:ROUND + 60]).all() and np.isnan(dev[263000:263300]).all()


@pytest.mark.parametrize("k,S", list(enumerate(SS)))
def test_min_max_fill_is_bit_identical_to_host(region, k, S):
    t0, dt, batch = _batch(S, k)
    row, v = batch[0], batch[2].copy()
    if S > 8:  # an invalid run over two workgroup boundaries of the flat array, inside the long series
        a, b = max(int(row[8]) + 1, tc.SCAN_SPAN - 24), min(int(row[9]) - 1, 2 * tc.SCAN_SPAN + 52)
        assert a < tc.SCAN_SPAN and b > 2 * tc.SCAN_SPAN
        v[a:b] = np.nan
    batch = (batch[0], batch[1], v, batch[3], batch[4])
    for lo, hi, span in ((NAN, NAN, 10**18), (-2.0, 12.0, 3 * dt), (0.0, NAN, 2 * dt), (NAN, 8.0, 0), (-5.0, 15.0, dt),
                         (-5.0, 15.0, 1200 * dt)):
        host = region.ts_min_max_fill_csr(*batch, lo, hi, span, host=True)
        _same(region.ts_min_max_fill_csr(*batch, lo, hi, span), host, (lo, hi, span))
    per_series = (np.where(np.arange(S) % 2, NAN, -1.0), np.where(np.arange(S) % 3, 9.0, NAN),
                  (dt * (1 + np.arange(S) % 5)).astype(np.int64))
    host = region.ts_min_max_fill_csr(*batch, *per_series, host=True)
    _same(region.ts_min_max_fill_csr(*batch, *per_series), host, "per series")


def test_min_max_fill_edges(region):
    """the span test is `>`; nothing leaks into or out of a series without a valid point"""
    row = [0, 3, 7, 10, 14]
    t = [0, 10, 20, 0, 10, 20, 30, 0, 10, 20, 0, 10, 20, 30]
    v = [1.0, 2.0, 3.0, NAN, NAN, NAN, NAN, 4.0, 5.0, 6.0, 1.0, NAN, NAN, 4.0]
    series = (row, t, v, [30, 40, 30, 40], [0, 1, 0, 1])
    for span, filled in ((30, [1.0, 2.0, 3.0, 4.0]), (29, [1.0, NAN, NAN, 4.0]), (0, [1.0, NAN, NAN, 4.0])):
        dev = region.ts_min_max_fill_csr(*series, NAN, NAN, span)
        _same(dev, region.ts_min_max_fill_csr(*series, NAN, NAN, span, host=True), span)
        assert np.array_equal(dev[:3], [1.0, 2.0, 3.0]) and np.all(np.isnan(dev[3:7]))
        assert np.array_equal(dev[7:10], [4.0, 5.0, 6.0])
        assert np.array_equal(np.isnan(dev[10:]), np.isnan(filled)), span
        assert np.allclose(dev[10:], filled, rtol=1e-12, atol=0.0, equal_nan=True), span
    edge = region.ts_min_max_fill_csr([0, 4], [0, 10, 20, 30], [50.0, 1.0, 2.0, -50.0], [40], [0], 0.0, 10.0, 1000)
    assert np.array_equal(edge, [NAN, 1.0, 2.0, NAN], equal_nan=True)  # invalid at index 0 and n - 1


def test_min_max_fill_over_the_second_round_of_the_aggregate_scan(region):
    """Invalid runs over flat position ROUND and over NP_ROUNDS - 1 - ROUND, where the mirrored scan meets the same
    boundary; max_timespan fills the shorter of a pair and refuses the longer. The runs of a few hundred points find
    their neighbours through the last aggregate of the first round or inside their own span. The two runs longer than
    a span are the ones that need the carry: each covers the whole first span of the second round of its scan and
    reaches into the next one, so the points there have no key in their own span nor in the aggregate before it and
    get their neighbour from the first round through the carried maximum alone."""
    row, t, v, t_end, fx = _two_round_series(78)
    mirror = NP_ROUNDS - 1 - ROUND
    short = v.copy()
    short[ROUND - 144:ROUND + 156] = 50.0   # 300 points above max_x: neighbours 301 steps apart
    short[mirror - 99:mirror + 101] = NAN   # 200 points: neighbours 201 steps apart
    short[ROUND - 1000:ROUND - 990] = NAN   # short runs on either side, and at both ends of the series
    short[ROUND + 1000:ROUND + 1003] = -50.0
    short[:2] = NAN
    short[-3:] = NAN
    for span in (250 * rc.HOUR, 301 * rc.HOUR, 10 * rc.HOUR):
        host = region.ts_min_max_fill_csr(row, t, short, t_end, fx, -1.0, 11.0, span, host=True)
        _same(region.ts_min_max_fill_csr(row, t, short, t_end, fx, -1.0, 11.0, span), host, span)
        assert np.isnan(host[ROUND]) == (span < 301 * rc.HOUR) and np.isnan(host[mirror]) == (span < 201 * rc.HOUR)
    long = v.copy()
    assert ROUND + tc.SCAN_SPAN + 132 < NP_ROUNDS and mirror - tc.SCAN_SPAN - 95 > 0
    long[ROUND - 44:ROUND + tc.SCAN_SPAN + 132] = NAN        # 1200 points, over spans 256 and 257 of the scan
    long[mirror - tc.SCAN_SPAN - 95:mirror + 101] = 50.0     # 1220 points, over spans 256 and 257 of the mirrored scan
    for span in (1210 * rc.HOUR, 1221 * rc.HOUR):
        host = region.ts_min_max_fill_csr(row, t, long, t_end, fx, -1.0, 11.0, span, host=True)
        _same(region.ts_min_max_fill_csr(row, t, long, t_end, fx, -1.0, 11.0, span), host, span)
        assert not np.isnan(host[ROUND + tc.SCAN_SPAN + 100])
        assert np.isnan(host[mirror - tc.SCAN_SPAN - 50]) == (span < 1221 * rc.HOUR)


@pytest.mark.parametrize("k,S", list(enumerate(SS)))
def test_rating_curve_is_bit_identical_to_host(region, k, S):
    t0, dt, batch = _batch(S, k)
    v = batch[2].copy()
    v[::5] = np.round(v[::5] * 2) / 2  # levels exactly on the `lower` grid of make_packs
    batch = (batch[0], batch[1], v, batch[3], batch[4])
    packs = tc.make_packs(6, t0, dt, 70 + S)
    assert {len(p) for p in packs} == {1, 3} and {len(c[1]) for p in packs for c in p} >= {1, 2, 9}
    csr = tc.packs_csr(packs)
    hit = 0
    for pack_of in (np.arange(S) % 6, np.zeros(S, np.int64), np.full(S, 3)):  # per series, and shared packs
        host = region.ts_rating_curve_csr(*batch, *csr, pack_of, host=True)
        _same(region.ts_rating_curve_csr(*batch, *csr, pack_of), host, pack_of[:3])
        hit += int(np.sum(np.isfinite(host)))
    assert hit > 0
    empty_pack = ([0, 0], [], [0], np.empty((0, 4)))  # a pack without curves: NaN everywhere
    assert np.all(np.isnan(region.ts_rating_curve_csr(*batch, *empty_pack, 0)))


def test_rating_curve_edges(region):
    """a time before the first curve and exactly on a start, a level on a lower, below the first and NaN, a
    negative base with a fractional exponent"""
    packs = [[(100, [(0.0, 2.0, 0.0, 1.0), (5.0, 3.0, 0.0, 1.0)]), (200, [(1.0, 1.0, 4.0, 1.5)])]]
    t = [99, 100, 150, 199, 200, 201, 300, 400, 500]
    v = [1.0, 1.0, 5.0, -0.5, 1.0, 8.0, 0.5, NAN, 3.0]
    args = ([0, 9], t, v, [600], [0], *tc.packs_csr(packs), 0)
    dev = region.ts_rating_curve_csr(*args)
    _same(dev, region.ts_rating_curve_csr(*args, host=True), "edges")
    assert np.isnan(dev).tolist() == [True, False, False, True, True, False, True, True, True]
    assert dev[1] == 2.0 and dev[2] == 15.0 and dev[5] == pytest.approx(8.0, rel=1e-15)  # 4 ** 1.5 within 2 ulp


def test_counters(region):
    from shyft_amd._native import ShyftHipError
    t0, dt = rc.EPOCHS[0]
    batch = rc.make_batch(9, t0, dt, 4)
    row, t = batch[0], batch[1]
    one_curve = ([0, 1], [t0], [0, 1], [[0.0, 1.0, 0.0, 1.0]])
    calls = (lambda **kw: region.ts_rating_curve_csr(*batch, *one_curve, **kw),
             lambda **kw: region.ts_ice_packing_csr(*batch, row, t, dt, 0.0, 2, **kw),
             lambda **kw: region.ts_ice_packing_recession_csr(*batch, np.ones(len(t)), t0, t0 + 2000 * dt, 1e-6, 0.0, **kw),
             lambda **kw: region.ts_min_max_fill_csr(*batch, 0.0, 10.0, 3 * dt, **kw))
    for call in calls:
        n0 = region.tsprep_calls()
        call()
        assert region.tsprep_calls() == n0 + 1 and region.tsprep_last_ms() > 0.0
        call(host=True)
        assert region.tsprep_calls() == n0 + 1
    n0 = region.tsprep_calls()
    none = (np.zeros(1, np.int64), [], [], [], [])                 # S == 0
    no_points = ([0, 0, 0], [], [], [5, 5], [0, 1])               # two series without points
    for b in (none, no_points):
        region.ts_min_max_fill_csr(*b, NAN, NAN, 5)
        region.ts_ice_packing_recession_csr(*b, [], 0, 10, 0.0, 0.0)
        region.ts_rating_curve_csr(*b, *one_curve)
    region.ts_ice_packing_csr(*batch, np.zeros(10, np.int64), [], dt, 0.0, 0)  # no queries
    bad = ([0, 2], [t0 + dt, t0], [1.0, 2.0], [t0 + 2 * dt], [0])
    with pytest.raises(ShyftHipError, match="needs time-points in increasing order"):
        region.ts_min_max_fill_csr(*bad, NAN, NAN, 5)
    with pytest.raises(ShyftHipError, match="needs time-points in increasing order"):
        region.ts_rating_curve_csr(*bad, *one_curve)
    with pytest.raises(ShyftHipError, match="total period of flow ts"):
        region.ts_ice_packing_recession_csr(*batch, np.ones(len(t)), t0 + 1, t0 + 2000 * dt, 0.0, 0.0)
    with pytest.raises(ShyftHipError, match="no rating-curve segments"):
        region.ts_rating_curve_csr(*batch, [0, 1], [t0], [0, 0], np.empty((0, 4)))
    with pytest.raises(ShyftHipError, match="one-point series"):
        region.ts_ice_packing_csr([0, 1], [10], [1.0], [20], [1], [0, 1], [15], 10, 0.0, 0)
    assert region.tsprep_calls() == n0


def _mixed_series(api, rng, k, t0, step, n, nan_share, lo, hi):
    times = t0 + step * np.arange(n) + np.concatenate([[0], rng.integers(0, step // 2, n - 1)]) * (k % 2)
    values = rng.uniform(lo, hi, n)
    values[rng.random(n) < nan_share] = np.nan
    fx = api.POINT_INSTANT_VALUE if k % 3 else api.POINT_AVERAGE_VALUE
    return api.TsFactory().create_time_point_ts(api.UtcPeriod(int(times[0]), int(times[-1]) + step), times.tolist(),
                                                values.tolist(), fx)


def test_ts_vector_methods_equal_the_per_series_methods(region):
    """each TsVector method is one device call (the recession two) and equals the TimeSeries method bit for bit; then
    the chain level -> fill -> rating -> recession on 7 mixed series, the indicator from TsVector.ice_packing on
    temperature series of another spacing"""
    from shyft_amd import api
    rng = np.random.default_rng(23)
    t0 = 1514764800
    levels, temps = api.TsVector(), api.TsVector()
    for k in range(7):
        n = (5, 40, 64, 90, 300, 2, 1100)[k]
        levels.append(_mixed_series(api, rng, k, t0, 3600, n, 0.05, -1.0, 12.0))
        temps.append(_mixed_series(api, rng, k + 1, t0 - 86400, 7200, n // 2 + 30, 0.1, -25.0, 5.0))
    rcf1, rcf2 = api.RatingCurveFunction(), api.RatingCurveFunction()
    for seg in ((0.0, 1.5, -0.2, 1.7), (4.0, 2.0, 0.5, 2.0), (9.0, 0.7, 1.0, 2.6)):
        rcf1.add_segment(*seg)
        rcf2.add_segment(seg[0] + 0.5, seg[1] * 1.1, seg[2], seg[3])
    rcp = api.RatingCurveParameters().add_curve(t0 - 10, rcf1).add_curve(t0 + 30 * 3600, rcf2)
    ipp = [api.IcePackingParameters(3600 * (6 + 12 * (k % 3)), -8.0 - k) for k in range(7)]
    ipr = api.IcePackingRecessionParameters(1 / (7 * 86400.0), 0.3)
    pol = api.ice_packing_temperature_policy.ALLOW_ANY_MISSING

    def check(dev, per_series, fx_of, what):
        assert isinstance(dev, api.TsVector) and len(dev) == 7
        for k, (d, one) in enumerate(zip(dev, per_series)):
            assert d.point_interpretation() == fx_of(k) == one.point_interpretation(), (what, k)
            assert d.size() == one.size()
            assert rc.same_bits(np.asarray(d.values), np.asarray(one.values)), (what, k)

    n0 = region.tsprep_calls()
    filled = levels.min_max_check_linear_fill(0.0, 11.0, 5 * 3600)
    assert region.tsprep_calls() == n0 + 1
    check(filled, [ts.min_max_check_linear_fill(0.0, 11.0, 5 * 3600) for ts in levels],
          lambda k: levels[k].point_interpretation(), "fill")
    flow = filled.rating_curve(rcp)
    assert region.tsprep_calls() == n0 + 2
    check(flow, [ts.rating_curve(rcp) for ts in filled], lambda k: levels[k].point_interpretation(), "rating")
    ice = temps.ice_packing(ipp, pol)
    assert region.tsprep_calls() == n0 + 3
    check(ice, [ts.ice_packing(p, pol) for ts, p in zip(temps, ipp)], lambda k: api.POINT_AVERAGE_VALUE, "ice")
    fixed = flow.ice_packing_recession(ice, ipr)
    assert region.tsprep_calls() == n0 + 5  # the indicators at the flow's points, then the scan
    check(fixed, [f.ice_packing_recession(i, ipr) for f, i in zip(flow, ice)],
          lambda k: levels[k].point_interpretation(), "recession")
    check(fixed, flow.ice_packing_recession(ice, ipr, host=True), lambda k: levels[k].point_interpretation(), "host")
    changed = sum(int(np.sum(np.asarray(a.values) != np.asarray(b.values))) for a, b in zip(fixed, flow))
    assert changed > 0  # some ice was found, so the chain exercised the recession
    # an indicator that is an ordinary series is sampled by its own f(t): one device call
    plain = api.TsVector(api.TimeSeries(_impl=i._ts._with_values(np.asarray(i.values), i.point_interpretation()))
                         for i in ice)
    n1 = region.tsprep_calls()
    sampled = flow.ice_packing_recession(plain, ipr)
    assert region.tsprep_calls() == n1 + 1
    check(sampled, [f.ice_packing_recession(i, ipr) for f, i in zip(flow, plain)],
          lambda k: levels[k].point_interpretation(), "sampled")
