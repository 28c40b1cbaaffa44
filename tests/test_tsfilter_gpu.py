"""The point-wise filter kernels on the GPU (kernels/tsfilter.hip): every device entry is bit-identical, NaN matching
NaN, to its _host twin (which runs host/ts_filter.hpp and is itself pinned by tests/test_tsfilter_host.py), then the
counters and the TsVector methods.

Batches are those of tests/tsfilter_cases.py: S = 1 / 63 / 64 / 65 / 257, lengths rotating over 0, 1, 2, 3, 63, 64, 65,
257, 1000, three time bases, both point types, NaN / inf hazards; where S > 8 one series of 3 * TILE + 228 points spans
more than three tiles of the tiled convolution, and most series start in the middle of a tile of the flat array."""
import numpy as np
import pytest

from tests import resample_cases as rc
from tests import tsfilter_cases as fc

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def region():
    from shyft_amd import region
    yield region
    region.tsfilter_set_path(region.TSFILTER_PATH_AUTO)


def _both_paths(region, host, *args):
    """the convolution with the path forced DIRECT and forced TILED, each asserted equal to the host"""
    try:
        for path in (region.TSFILTER_PATH_DIRECT, region.TSFILTER_PATH_TILED):
            region.tsfilter_set_path(path)
            dev = region.ts_convolve_w_csr(*args)
            assert region.tsfilter_last_path() == path
            fc.same(dev, host, ("path", path))
    finally:
        region.tsfilter_set_path(region.TSFILTER_PATH_AUTO)
    return dev


@pytest.mark.parametrize("k,S", list(enumerate(fc.SS)))
def test_convolve_w_is_bit_identical_to_host_on_both_paths(region, k, S):
    _, _, b, _ = fc.batch(S, k)
    if S > fc.LONG_AT:
        assert b[0][fc.LONG_AT + 1] - b[0][fc.LONG_AT] == 3 * fc.TILE + 228 and b[0][fc.LONG_AT] % fc.TILE != 0
    # one shared profile per K, the policy rotating over the series
    for n, K in enumerate(fc.KS):
        w_row, w = fc.profiles([K], 100 + K, nan_in=(0,) if K == 65 else ())
        policy = np.array([(s + n) % 3 for s in range(S)], np.int32)
        host = region.ts_convolve_w_csr(*b, w_row, w, 0, policy, host=True)
        _both_paths(region, host, *b, w_row, w, 0, policy)
    # per-series profiles of mixed K, one of them with a NaN weight, under each single policy
    w_row, w = fc.profiles(fc.KS, 7, nan_in=(4,))
    assert np.any(w == 0.0) and np.any(w < 0.0) and np.isnan(w).sum() == 1
    w_of = (np.arange(S) * 5 + 3) % len(fc.KS)
    for policy in (fc.USE_FIRST, fc.USE_ZERO, fc.USE_NAN):
        host = region.ts_convolve_w_csr(*b, w_row, w, w_of, policy, host=True)
        _both_paths(region, host, *b, w_row, w, w_of, policy)


def test_convolve_w_start_zone_of_a_series_in_the_middle_of_the_flat_array(region):
    """row = [0, 3, 7]: the second series starts at flat point 3; nothing of the first may leak into its start zone"""
    hour = rc.HOUR
    b = ([0, 3, 7], [0, hour, 2 * hour, 0, hour, 2 * hour, 3 * hour], [100.0, 200.0, 300.0, 1.0, 2.0, 4.0, 8.0],
         [3 * hour, 4 * hour], [1, 0])
    w = [1.0, 10.0, 1000.0]
    expected = {fc.USE_FIRST: [101100.0, 101200.0, 102300.0, 1011.0, 1012.0, 1024.0, 2048.0],
                fc.USE_ZERO: [100.0, 1200.0, 102300.0, 1.0, 12.0, 1024.0, 2048.0],
                fc.USE_NAN: [NAN, NAN, 102300.0, NAN, NAN, 1024.0, 2048.0]}
    for policy, want in expected.items():
        host = region.ts_convolve_w_csr(*b, [0, 3], w, 0, policy, host=True)
        dev = _both_paths(region, host, *b, [0, 3], w, 0, policy)
        assert np.array_equal(dev, want, equal_nan=True), (policy, dev.tolist())
    # a profile longer than the chunk over the same two series: still only the series' own values
    w_row, w = fc.profiles([fc.CHUNK + 5], 11)
    host = region.ts_convolve_w_csr(*b, w_row, w, 0, fc.USE_FIRST, host=True)
    _both_paths(region, host, *b, w_row, w, 0, fc.USE_FIRST)


def test_convolve_w_auto_threshold(region):
    t0, dt = rc.EPOCHS[0]
    b = rc.make_batch(4, t0, dt, 5, lengths=(1000,))
    for K, path in ((0, region.TSFILTER_PATH_DIRECT), (1, region.TSFILTER_PATH_DIRECT), (2, region.TSFILTER_PATH_TILED),
                    (300, region.TSFILTER_PATH_TILED)):
        w_row, w = fc.profiles([K], K)
        dev = region.ts_convolve_w_csr(*b, w_row, w)
        assert region.tsfilter_last_path() == path, K
        fc.same(dev, region.ts_convolve_w_csr(*b, w_row, w, host=True), K)
    short = rc.make_batch(40, t0, dt, 6, lengths=(3,))  # tiles of 3 points: nearly empty, so DIRECT
    w_row, w = fc.profiles([64], 1)
    fc.same(region.ts_convolve_w_csr(*short, w_row, w), region.ts_convolve_w_csr(*short, w_row, w, host=True), "short")
    assert region.tsfilter_last_path() == region.TSFILTER_PATH_DIRECT


@pytest.mark.parametrize("k,S", list(enumerate(fc.SS)))
def test_derivative_is_bit_identical_to_host(region, k, S):
    _, _, b, fixed = fc.batch(S, k)
    runs = fc.with_nan_runs(b)
    if len(b[2]) > fc.BLOCK + 3:
        assert np.all(np.isnan(runs[2][fc.BLOCK - 3:fc.BLOCK + 3]))  # a NaN run over a workgroup boundary
    stair = (runs[0], runs[1], runs[2], runs[3], np.ones(S, np.int32))
    for bb in (b, runs, stair):
        for method in (fc.DEFAULT, fc.FORWARD, fc.BACKWARD, fc.CENTER):
            for fdt in (fixed, 0):  # the fixed step given for the evenly spaced series, and the variable branch for all
                host = region.ts_derivative_csr(*bb, fdt, method, host=True)
                fc.same(region.ts_derivative_csr(*bb, fdt, method), host, (method, np.max(fdt)))
    per_series = np.arange(S, dtype=np.int32) % 4
    fc.same(region.ts_derivative_csr(*stair, fixed, per_series),
            region.ts_derivative_csr(*stair, fixed, per_series, host=True), "per series")


def test_derivative_reads_nothing_of_a_neighbouring_series(region):
    """three stair-case series back to back: the edge branches at every first and last point"""
    hour = rc.HOUR
    t = [0, hour, 2 * hour, 0, hour, 0, hour, 2 * hour, 3 * hour]
    v = [1.0, 2.0, 4.0, 1e6, -1e6, 8.0, 16.0, 32.0, 64.0]
    b = ([0, 3, 5, 9], t, v, [3 * hour, 2 * hour, 4 * hour], [1, 1, 1])
    s = 3600.0
    want = {fc.FORWARD: [1 / s, 2 / s, 0.0, -2e6 / s, 0.0, 8 / s, 16 / s, 32 / s, 0.0],
            fc.BACKWARD: [0.0, 1 / s, 2 / s, 0.0, -2e6 / s, 0.0, 8 / s, 16 / s, 32 / s],
            fc.CENTER: [1 / (2 * s), 3 / (2 * s), 2 / (2 * s), -2e6 / (2 * s), -2e6 / (2 * s), 8 / (2 * s), 24 / (2 * s),
                        48 / (2 * s), 32 / (2 * s)]}
    for method, expected in want.items():
        for fdt in (hour, 0):
            dev = region.ts_derivative_csr(*b, fdt, method)
            fc.same(dev, region.ts_derivative_csr(*b, fdt, method, host=True), (method, fdt))
            assert dev.tolist() == expected, (method, fdt, dev.tolist())


@pytest.mark.parametrize("k,S", list(enumerate(fc.SS)))
def test_inside_and_decode_are_bit_identical_to_host(region, k, S):
    _, _, b, _ = fc.batch(S, k)
    v = b[2].copy()
    v[::7] = 2.0   # exactly on min_x
    v[3::7] = 9.0  # exactly on max_x
    b = (b[0], b[1], v, b[3], b[4])
    ix = np.arange(S)
    per_series = (np.where(ix % 3, 2.0, NAN), np.where(ix % 2, 9.0, NAN), np.where(ix % 4, NAN, -1.0), 1.0 + ix, -1.0 - ix)
    for p in (per_series, (2.0, 9.0), (NAN, NAN, 0.5, 2.0, 3.0), (9.0, 2.0)):
        host = region.ts_inside_csr(*b, *p, host=True)
        fc.same(region.ts_inside_csr(*b, *p), host, "inside")
    on_limits = region.ts_inside_csr([0, 4], [0, 1, 2, 3], [2.0, 9.0, np.nextafter(9.0, 0.0), np.nextafter(2.0, 0.0)], [4], [1],
                                     2.0, 9.0)
    assert on_limits.tolist() == [1.0, 0.0, 1.0, 0.0]  # [min_x, max_x)
    d = fc.decode_values(b, 80 + S)
    start, bits = (ix % 50).astype(np.int32), (1 + ix % 2).astype(np.int32)
    bits[0], start[0] = 51, 0
    for sb, nb in ((start, bits), (0, 1), (0, 51), (50, 1), (13, 7)):
        host = region.ts_decode_csr(*d, sb, nb, host=True)
        fc.same(region.ts_decode_csr(*d, sb, nb), host, ("decode", np.max(sb)))
    got = region.ts_decode_csr([0, 6], np.arange(6), [2.0**52, 2.0**52 + 2, 5.75, -1.0, NAN, 2.0**52 - 1], [6], [0], 0, 51)
    assert np.array_equal(got, [0.0, NAN, 5.0, NAN, NAN, 2.0**51 - 1], equal_nan=True)


def test_counters(region):
    from shyft_amd._native import ShyftHipError
    t0, dt = rc.EPOCHS[0]
    b = rc.make_batch(9, t0, dt, 4)
    calls = (lambda **kw: region.ts_convolve_w_csr(*b, [0, 3], [0.25, 0.5, 0.25], **kw),
             lambda **kw: region.ts_derivative_csr(*b, **kw),
             lambda **kw: region.ts_inside_csr(*b, 0.0, 10.0, **kw),
             lambda **kw: region.ts_decode_csr(*b, 0, 4, **kw))
    for call in calls:
        n0 = region.tsfilter_calls()
        call()
        assert region.tsfilter_calls() == n0 + 1 and region.tsfilter_last_ms() > 0.0
        call(host=True)
        assert region.tsfilter_calls() == n0 + 1
    n0 = region.tsfilter_calls()
    none = (np.zeros(1, np.int64), [], [], [], [])   # S == 0
    no_points = ([0, 0, 0], [], [], [5, 5], [0, 1])  # two series without points
    for e in (none, no_points):
        region.ts_convolve_w_csr(*e, [0, 1], [1.0])
        region.ts_derivative_csr(*e)
        region.ts_inside_csr(*e, NAN, NAN)
        region.ts_decode_csr(*e, 0, 1)
    bad = ([0, 2], [t0 + dt, t0], [1.0, 2.0], [t0 + 2 * dt], [0])
    with pytest.raises(ShyftHipError, match="needs time-points in increasing order"):
        region.ts_inside_csr(*bad, NAN, NAN)
    with pytest.raises(ShyftHipError, match="convolve_w: policy must be"):
        region.ts_convolve_w_csr(*b, [0, 1], [1.0], 0, 3)
    with pytest.raises(ShyftHipError, match="derivative: fixed_dt is not the spacing"):
        region.ts_derivative_csr(*b, dt // 2)
    with pytest.raises(ShyftHipError, match="start_bit must be in range"):
        region.ts_decode_csr(*b, 52, 1)
    with pytest.raises(ShyftHipError, match="more than 65536 weights"):
        region.ts_convolve_w_csr(*b, [0, 65537], np.zeros(65537))
    assert region.tsfilter_calls() == n0


def _mixed_series(api, rng, k, t0, step, n, nan_share, lo, hi):
    times = t0 + step * np.arange(n) + np.concatenate([[0], rng.integers(0, step // 2, n - 1)]) * (k % 2)
    values = rng.uniform(lo, hi, n)
    values[rng.random(n) < nan_share] = np.nan
    fx = api.POINT_INSTANT_VALUE if k % 3 else api.POINT_AVERAGE_VALUE
    return api.TsFactory().create_time_point_ts(api.UtcPeriod(int(times[0]), int(times[-1]) + step), times.tolist(),
                                                values.tolist(), fx)


def test_ts_vector_methods_equal_the_per_series_methods(region):
    """each TsVector method is one device call and equals the TimeSeries method bit for bit, and host=True; then the
    chain status -> decode -> inside -> (flow * mask).convolve_w -> derivative on 7 mixed series"""
    from shyft_amd import api
    rng = np.random.default_rng(29)
    t0 = 1514764800
    flows, status = api.TsVector(), api.TsVector()
    for k in range(7):
        n = (5, 40, 64, 90, 300, 2, 1100)[k]
        f = _mixed_series(api, rng, k, t0, 3600, n, 0.05, 0.0, 12.0)
        if k in (1, 4):  # two series on a fixed axis: derivative takes the fixed-step branch for them
            f = api.TimeSeries(api.TimeAxis(t0, 3600, n), list(f.values), api.POINT_AVERAGE_VALUE)
        flows.append(f)
        bits = rng.integers(0, 16, n).astype(np.float64)
        bits[rng.random(n) < 0.05] = np.nan
        status.append(api.TimeSeries(_impl=f._ts._with_values(bits, f.point_interpretation())))
    assert [f._ts._fixed_dt_us for f in flows] == [0, 3600 * 10**6, 0, 0, 3600 * 10**6, 0, 0]

    def check(dev, per_series, fx_of, what):
        assert isinstance(dev, api.TsVector) and len(dev) == 7
        for k, (d, one) in enumerate(zip(dev, per_series)):
            assert d.point_interpretation() == fx_of(k) == one.point_interpretation(), (what, k)
            assert d.size() == one.size()
            assert rc.same_bits(np.asarray(d.values), np.asarray(one.values)), (what, k)

    same_fx = lambda k: flows[k].point_interpretation()  # noqa: E731
    n0 = region.tsfilter_calls()
    flag = status.decode(1, 2)
    assert region.tsfilter_calls() == n0 + 1
    check(flag, [ts.decode(1, 2) for ts in status], same_fx, "decode")
    check(flag, status.decode(1, 2, host=True), same_fx, "decode host")
    mask = flag.inside(NAN, 2.0, 0.0, 1.0, 0.0)
    assert region.tsfilter_calls() == n0 + 2
    check(mask, [ts.inside(NAN, 2.0, 0.0, 1.0, 0.0) for ts in flag], same_fx, "inside")
    check(mask, flag.inside(NAN, 2.0, 0.0, 1.0, 0.0, host=True), same_fx, "inside host")
    profile, wide = [0.1, 0.2, 0.4, 0.2, 0.1], list(np.linspace(0.0, 1.0, 70) / 35.0)
    weights = [profile, wide, profile, profile, wide, profile, wide]
    policies = [api.USE_FIRST, api.USE_ZERO, api.USE_NAN, api.USE_FIRST, api.USE_ZERO, api.USE_NAN, api.USE_FIRST]
    masked = flows * mask  # lazy expressions: evaluated first
    n1 = region.tsfilter_calls()
    shaped = masked.convolve_w(weights, policies)
    assert region.tsfilter_calls() == n1 + 1
    check(shaped, [ts.convolve_w(w, p) for ts, w, p in zip(masked, weights, policies)], same_fx, "convolve")
    check(shaped, masked.convolve_w(weights, policies, host=True), same_fx, "convolve host")
    one_for_all = flows.convolve_w(profile, api.USE_FIRST)
    assert region.tsfilter_calls() == n1 + 2
    check(one_for_all, [ts.convolve_w(profile, api.USE_FIRST) for ts in flows], same_fx, "one profile")
    methods = [api.DEFAULT, api.FORWARD, api.BACKWARD, api.CENTER, api.FORWARD, api.DEFAULT, api.BACKWARD]
    n2 = region.tsfilter_calls()
    slope = shaped.derivative(methods)
    assert region.tsfilter_calls() == n2 + 1
    check(slope, [ts.derivative(m) for ts, m in zip(shaped, methods)], lambda k: api.POINT_AVERAGE_VALUE, "derivative")
    check(slope, shaped.derivative(methods, host=True), lambda k: api.POINT_AVERAGE_VALUE, "derivative host")
    check(shaped.derivative(), [ts.derivative() for ts in shaped], lambda k: api.POINT_AVERAGE_VALUE, "default")
    assert sum(int(np.sum(np.isfinite(np.asarray(s.values)))) for s in slope) > 100  # the chain produced numbers
