"""The fused percentile kernel on the GPU: shyft_hip_ts_percentiles is bit-identical to shyft_hip_ts_percentiles_host
(host/ts_percentiles.hpp, itself held to the independent restatement by tests/test_ts_percentiles_host.py) on both
launch shapes, over the sizes at which kernels/ts_percentiles.hip can go wrong, then api.percentiles on the device.

S in {1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096}: one lane, a partial and a full wavefront on the WAVE path; one
more than a wavefront, one less than, exactly and one more than a workgroup's stride, a non power of two and the limit
on the LDS path. T in {1, 3, 4, 5, 64, 65}: 3, 4 and 5 leave partial four-interval workgroups on the WAVE path. S and
T rotate over the eleven axis kinds and three epochs of tests/resample_cases.py; every case runs every percentile
list. Row lengths are mixed as in the host test; S = 4096 uses rows of at most 8 points.

Everywhere two values agree when their bits are equal, both are NaN or both are zero (cases.same); no tolerance."""
import numpy as np
import pytest

from tests import ts_percentiles_cases as cases

pytestmark = pytest.mark.gpu

SS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096)
TS = (1, 3, 4, 5, 64, 65)
PCT_LISTS = ([50],
             [0, 10, 25, -1, 50, 50, 75, 90, 100, -1000, 1000, 101, -1, 33, 66, 1000],  # 16: the device's limit
             [0, 10, 25, -1, 50, 75, 90, 100],                                          # no extremes: nothing folded
             [-1000, 1000])                                                             # extremes alone: nothing sorted
NaN, INF = float("nan"), float("inf")


def _cases():
    out = []
    for i in range(len(cases.AXES) * 3):
        out.append((SS[i % len(SS)], TS[(i + i // len(SS)) % len(TS)], cases.AXES[i % len(cases.AXES)], i % 3))
    return out


@pytest.fixture(scope="module")
def region():
    from shyft_amd import region
    yield region
    region.ts_percentiles_set_path(region.TS_PERCENTILES_PATH_AUTO)


def legal_paths(region, S):
    """(forced path, the path it must report)"""
    W, L, A = region.TS_PERCENTILES_PATH_WAVE, region.TS_PERCENTILES_PATH_LDS, region.TS_PERCENTILES_PATH_AUTO
    return ((A, W), (W, W), (L, L)) if S <= 64 else ((A, L), (L, L))


def device_equals_host(region, batch, src, shift, ta_t0, ta_dt, T, lists=PCT_LISTS):
    for pcts in lists:
        host = region.ts_percentiles_csr(*batch, src, shift, ta_t0, ta_dt, T, pcts, host=True)
        assert host.shape == (len(pcts), T)
        for forced, reported in legal_paths(region, len(src)):
            region.ts_percentiles_set_path(forced)
            dev = region.ts_percentiles_csr(*batch, src, shift, ta_t0, ta_dt, T, pcts)
            assert region.ts_percentiles_last_path() == reported
            bad = np.argwhere(~((np.isnan(dev) & np.isnan(host)) | (dev == host)))
            assert cases.same(dev, host), (pcts, forced, len(bad), bad[:4].tolist())
    region.ts_percentiles_set_path(region.TS_PERCENTILES_PATH_AUTO)


def test_the_rotation_covers_every_size_axis_epoch_and_list():
    c = _cases()
    assert {x[0] for x in c} == set(SS) and {x[1] for x in c} == set(TS)
    assert {x[2] for x in c} == set(cases.AXES) and {x[3] for x in c} == {0, 1, 2}
    assert {(x[2], x[3]) for x in c} == {(k, e) for k in cases.AXES for e in range(3)}
    assert len(PCT_LISTS[1]) == 16 and not set(PCT_LISTS[2]) & {-1000, 1000}


@pytest.mark.parametrize("S,T,kind,epoch", _cases())
def test_device_is_bit_identical_to_host(region, S, T, kind, epoch):
    t0, dt = cases.EPOCHS[epoch]
    seed = 9000 + 10 * SS.index(S) + TS.index(T)
    batch = cases.batch_for(kind, S, epoch, seed, lengths=cases.SHORT_LENGTHS if S == 4096 else cases.LENGTHS)
    if S >= 8:
        assert len(set(np.diff(batch[0]).tolist())) > 3  # mixed row lengths: the CSR offsets matter
    device_equals_host(region, batch, *cases.identity_views(batch), *cases.axis(kind, t0, dt, T), T)


def test_views_of_two_stored_series(region):
    """R = 2 (a linear and a stair-case row), 80 views with 80 distinct shifts on the LDS path; 64 equal views, where
    all keys tie, on both"""
    t0, dt = cases.EPOCHS[0]
    batch = cases.make_batch(4, t0, dt, 11, lengths=(1000,))
    batch = cases.materialise(batch, [0, 2], [0, 0])  # series 0 and 2: plain values and a NaN run; linear and stair-case
    assert batch[4].tolist() == [0, 1]
    src = np.arange(80, dtype=np.int32) % 2
    shift = (np.arange(80, dtype=np.int64) - 40) * (7 * dt) + np.arange(80) % 5
    assert len(set(shift.tolist())) == 80
    for kind, T in (("own", 65), ("x24", 5)):
        device_equals_host(region, batch, src, shift, *cases.axis(kind, t0 + 300 * dt, dt, T), T)
    src, shift = np.ones(64, dtype=np.int32), np.full(64, 3 * dt + 1, dtype=np.int64)
    device_equals_host(region, batch, src, shift, *cases.axis("x2", t0 + 100 * dt, dt, 5), 5)
    one = region.ts_percentiles_csr(*batch, src[:1], shift[:1], *cases.axis("x2", t0 + 100 * dt, dt, 5), 5, PCT_LISTS[1])
    all_equal = region.ts_percentiles_csr(*batch, src, shift, *cases.axis("x2", t0 + 100 * dt, dt, 5), 5, PCT_LISTS[1])
    keep = [k for k, p in enumerate(PCT_LISTS[1]) if p != -1]  # the average of 64 equal samples rounds
    assert cases.same(one[keep], all_equal[keep])


SECOND = 10**6
ONE_UP = float(np.nextafter(1.0, 2.0))
HAZARDS = np.array([
    [NaN, INF, -INF, NaN, NaN, INF],                                     # nothing finite
    [NaN, NaN, -2.5, INF, NaN, -INF],                                    # exactly one finite
    [NaN, 4.0, NaN, NaN, 1.0, NaN],                                      # nf = 2: p = 50 lies between them
    [0.0, -0.0, 0.0, -0.0, NaN, -0.0],                                   # zeros of both signs
    [INF, -INF, 1.0, 2.0, NaN, 3.0],                                     # infinite points among finite ones
    [5e-324, -5e-324, 1e-310, 0.0, 2.2250738585072014e-308, -1e-320],    # denormals
    [1.0, ONE_UP, float(np.nextafter(1.0, 0.0)), 1.0, ONE_UP, float(np.nextafter(ONE_UP, 2.0))],  # the last bit
])


def test_sample_hazards(region):
    """six stair-case series of one point per second on their own axis: the sample of (series, interval) is the value
    itself (to_seconds of one second is 1.0), so every interval is one row of HAZARDS"""
    T, S = HAZARDS.shape
    t = np.tile(np.arange(T, dtype=np.int64) * SECOND, S)
    batch = (np.arange(S + 1, dtype=np.int64) * T, t, HAZARDS.T.reshape(-1).copy(), np.full(S, T * SECOND, np.int64),
             np.ones(S, np.int32))
    src, shift = cases.identity_views(batch)
    samples = region.resample_csr(*batch, 0, SECOND, T, 0, host=True)
    # an infinite point counts as missing, and the area 0.0 + 1.0 * -0.0 is +0.0: negative zeros reach the extremes only
    assert cases.same(samples, np.where(np.isinf(HAZARDS), NaN, HAZARDS))
    lists = PCT_LISTS + (list(range(0, 101, 7)) + [100],)
    device_equals_host(region, batch, src, shift, 0, SECOND, T, lists)
    r = region.ts_percentiles_csr(*batch, src, shift, 0, SECOND, T, [0, 50, 100, -1, -1000, 1000])
    assert np.isnan(r[:, 0]).all()
    assert (r[:, 1] == -2.5).all()
    assert r[:, 2].tolist() == [1.0, 2.5, 4.0, 2.5, 1.0, 4.0]
    assert (r[:, 3] == 0.0).all()
    assert r[:, 4].tolist() == [1.0, 2.0, 3.0, 2.0, 1.0, 3.0]
    assert r[[0, 2, 4, 5], 5].tolist() == [-1e-320, 2.2250738585072014e-308, -1e-320, 2.2250738585072014e-308]
    assert r[[0, 2, 4, 5], 6].tolist() == [float(np.nextafter(1.0, 0.0)), float(np.nextafter(ONE_UP, 2.0))] * 2
    # the same rows among 70 views, the others without a finite sample: the LDS shape with nf far below S
    pad = np.concatenate([src, np.zeros(64, np.int32)])
    pad_shift = np.concatenate([shift, np.full(64, 100 * SECOND, np.int64)])  # moved past the axis
    device_equals_host(region, batch, pad, pad_shift, 0, SECOND, T, lists)
    padded = region.ts_percentiles_csr(*batch, pad, pad_shift, 0, SECOND, T, [0, 50, 100, -1, -1000, 1000])
    assert region.ts_percentiles_last_path() == region.TS_PERCENTILES_PATH_LDS
    assert cases.same(padded, r)


def test_infinite_averages_are_dropped(region):
    """finite points whose area overflows: the averages are +inf and -inf and are not samples, the points still are
    the extremes"""
    big = 1.7e308
    batch = (np.array([0, 4, 8, 12]), np.tile(np.arange(4, dtype=np.int64) * SECOND, 3),
             np.array([big] * 4 + [-big] * 4 + [1.0, 2.0, 3.0, 4.0]), np.full(3, 4 * SECOND, np.int64), np.ones(3, np.int32))
    src, shift = cases.identity_views(batch)
    samples = region.resample_csr(*batch, 0, 2 * SECOND, 2, 0, host=True)
    assert samples.tolist() == [[INF, -INF, 1.5], [INF, -INF, 3.5]]
    device_equals_host(region, batch, src, shift, 0, 2 * SECOND, 2)
    r = region.ts_percentiles_csr(*batch, src, shift, 0, 2 * SECOND, 2, [0, 50, 100, -1, -1000, 1000])
    assert r.tolist() == [[1.5, 3.5]] * 4 + [[-big, -big], [big, big]]


def test_paths_limits_and_counters(region):
    from shyft_amd._native import ShyftHipError
    t0, dt = cases.EPOCHS[0]
    W, L, A = region.TS_PERCENTILES_PATH_WAVE, region.TS_PERCENTILES_PATH_LDS, region.TS_PERCENTILES_PATH_AUTO
    ta = cases.axis("own", t0, dt, 5)
    b64, b65 = cases.make_batch(64, t0, dt, 21, lengths=(8,)), cases.make_batch(65, t0, dt, 22, lengths=(8,))
    region.ts_percentiles_set_path(A)
    region.ts_percentiles_csr(*b64, *cases.identity_views(b64), *ta, 5, [50])
    assert region.ts_percentiles_last_path() == W
    assert region.ts_percentiles_last_ms() > 0
    region.ts_percentiles_csr(*b65, *cases.identity_views(b65), *ta, 5, [50])
    assert region.ts_percentiles_last_path() == L
    assert region.ts_percentiles_last_ms() > 0
    calls = region.ts_percentiles_calls()
    region.ts_percentiles_csr(*b65, *cases.identity_views(b65), *ta, 5, [50, -1000])
    assert region.ts_percentiles_calls() == calls + 1
    calls += 1
    try:
        region.ts_percentiles_set_path(W)
        with pytest.raises(ShyftHipError, match="WAVE path takes at most 64 series"):
            region.ts_percentiles_csr(*b65, *cases.identity_views(b65), *ta, 5, [50])
    finally:
        region.ts_percentiles_set_path(A)
    with pytest.raises(ShyftHipError, match="path must be AUTO, WAVE or LDS"):
        region.ts_percentiles_set_path(3)
    src = np.zeros(4097, np.int32)
    with pytest.raises(ShyftHipError, match="SHYFT_HIP_TS_PERCENTILES_MAX_SERIES = 4096"):
        region.ts_percentiles_csr(*b64, src, np.zeros(4097, np.int64), *ta, 5, [50])
    with pytest.raises(ShyftHipError, match="SHYFT_HIP_PERCENTILES_MAX = 16"):
        region.ts_percentiles_csr(*b64, *cases.identity_views(b64), *ta, 5, list(range(17)))
    with pytest.raises(ShyftHipError, match="view 0 has src 64 outside the 64 series"):
        region.ts_percentiles_csr(*b64, [64], [0], *ta, 5, [50])
    assert np.isnan(region.ts_percentiles_csr(*b64, [], [], *ta, 5, [50])).all()
    assert region.ts_percentiles_csr(*b64, *cases.identity_views(b64), *ta, 0, [50]).shape == (1, 0)
    assert region.ts_percentiles_csr(*b64, *cases.identity_views(b64), *ta, 5, []).shape == (0, 5)
    assert region.ts_percentiles_calls() == calls  # a refused and an empty call launch nothing
    # the host twin has no limits
    assert region.ts_percentiles_csr(*b64, src, np.zeros(4097, np.int64), *ta, 5, list(range(17)), host=True).shape == (17, 5)


def as_arrays(tsv):
    return np.array([ts.values for ts in tsv])


def test_api_percentiles_on_the_device(region):
    """the shrunk partition scenario of shyft/tests/api/test_time_series.py:485-523, and a vector that mixes a concrete
    series, a pending expression and a view: host=False equals host=True"""
    from shyft_amd import api
    c = api.Calendar()
    t0, common_t0, dt = c.time(2010, 9, 1), c.time(2016, 9, 1), api.deltahours(1)
    n = c.diff_units(t0, common_t0, dt)
    pcts = [0, 10, 25, -1, 50, 75, 90, 100, -1000, 1000]
    ta = api.TimeAxis(common_t0, api.deltahours(24), 365)
    for fx in (api.POINT_AVERAGE_VALUE, api.POINT_INSTANT_VALUE):
        v = np.sin(np.arange(n) / 50.0) * 30 + np.arange(n) % 17
        v[1000:1100] = np.nan
        src = api.TimeSeries(api.TimeAxis(t0, dt, n), v, fx)
        parts = src.partition_by(c, t0, api.Calendar.YEAR, 5, common_t0)
        calls = region.ts_percentiles_calls()
        dev = api.percentiles(parts, ta, pcts, host=False)
        assert region.ts_percentiles_calls() == calls + 1 and all(ts._impl is None for ts in parts)
        assert cases.same(as_arrays(dev), as_arrays(api.percentiles(parts, ta, pcts)))
        assert cases.same(as_arrays(dev), as_arrays(parts.percentiles(ta, pcts, host=False)))
        assert all(ts.point_interpretation() == fx and ts.size() == 365 for ts in dev)

    ta_src = api.TimeAxis(common_t0, dt, 240)
    concrete = api.TimeSeries(ta_src, np.arange(240.0) % 13, api.POINT_AVERAGE_VALUE)

    def mixed():
        return api.TsVector([concrete, concrete * 2.0 + 1.0, src.partition_by(c, t0, api.Calendar.YEAR, 5, common_t0)[2]])

    ta10 = api.TimeAxis(common_t0, api.deltahours(24), 10)
    tsv = mixed()
    dev = api.percentiles(tsv, ta10, pcts, host=False)
    assert tsv[1]._impl is not None and tsv[2]._impl is None
    assert cases.same(as_arrays(dev), as_arrays(api.percentiles(mixed(), ta10, pcts, host=True)))
    # beyond the device's limits the host twin answers
    calls = region.ts_percentiles_calls()
    many = api.percentiles(tsv, ta10, list(range(17)), host=False)
    assert len(many) == 17 and region.ts_percentiles_calls() == calls
