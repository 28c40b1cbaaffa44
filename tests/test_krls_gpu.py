"""The KRLS kernels on the GPU: region.krls_train_csr and krls_predict are bit-identical to their host=True twins
(csrc/host/krls.hpp) in d, alpha, Kinv, P, mse and every predicted value, and every series comes back by the path its
dictionary size calls for.

Training cases are grow-only (gamma 0.5 on unit spacing: every valid point joins, tests/test_krls_host.py shows it), so
the dictionary size is known before the run: C = KRLS_LDS_CAPACITY entries fit the LDS storage, KRLS_MAX_DICT the
workspace. Valid points in {1, 2, 3, 63, 64, 65, C-1, C} are a single entry, the wavefront boundary of the strided
sums and the last LDS sizes, {SMALL-1, SMALL, SMALL+1} the step from the small LDS storage to the large one;
{C+1, 2C+5} overflow the LDS storage and are retrained in the workspace, and {256, 300} are there the last size with
one row per lane and one where some lanes own two. Only KRLS_MAX_DICT + 3 valid points and size=8 (an entry must be
removed) may come back by the host path; test_host_path_share holds the whole file to that."""
import numpy as np
import pytest

from shyft_amd import api, region
from tests.krls_cases import GROW, HOUR, MIXED, T0, US, csr, grow_series, noisy_sine, same_bits, same_state

pytestmark = pytest.mark.gpu

C = region.KRLS_LDS_CAPACITY
SMALL = region.KRLS_LDS_SMALL_CAPACITY  # the LDS storage tried first; SMALL + 1 valid points are retrained at capacity C
LDS, WS, HOST = region.KRLS_PATH_LDS, region.KRLS_PATH_WORKSPACE, region.KRLS_PATH_HOST
_HOST_PATH_CASES = []  # the kind of every case in which a series came back by the host path


def _both(kind, series, dt, **kw):
    """the device and the host result of one batch; the device's paths are recorded"""
    args = csr(series)
    dev = region.krls_train_csr(*args, dt, **kw)
    host = region.krls_train_csr(*args, dt, host=True, **kw)
    if (dev[6] == HOST).any():
        _HOST_PATH_CASES.append(kind)
    assert (host[6] == HOST).all()
    return dev, host


@pytest.mark.parametrize("valid", [1, 2, 3, SMALL - 1, SMALL, SMALL + 1, 63, 64, 65, C - 1, C, C + 1, 2 * C + 5, 256, 300])
def test_valid_points_and_paths(valid):
    dev, host = _both("valid points", [grow_series(valid, valid)], HOUR, **GROW)
    assert host[0].tolist() == [0, valid]
    assert dev[6].tolist() == [LDS if valid <= C else WS]
    assert same_state(dev, host)


def test_beyond_max_dict_comes_back_by_the_host():
    valid = region.KRLS_MAX_DICT + 3
    dev, host = _both("beyond KRLS_MAX_DICT", [grow_series(valid, 1)], HOUR, **GROW)
    assert host[0].tolist() == [0, valid] and dev[6].tolist() == [HOST]
    assert same_state(dev, host)


def test_size_8_comes_back_by_the_host():
    dev, host = _both("size=8", [grow_series(40, 2)], HOUR, size=8, **GROW)
    assert host[0].tolist() == [0, 8] and dev[6].tolist() == [HOST]
    assert same_state(dev, host)


@pytest.mark.parametrize("batch", [1, 2, 5, 257])
def test_batches_of_mixed_series_and_parameters(batch):
    """one workgroup, a few, and more than the CU count; lengths mixed, an empty and an all-NaN series among them,
    every series with parameters of its own"""
    valid = [5, 0, -1, 17, 64, C + 3, 33][:batch] if batch <= 5 else [(7 * k) % 41 - 1 for k in range(batch)]
    if batch > 5:
        valid[100], valid[200] = C + 1, 2 * C
    series = []
    for k, n in enumerate(valid):
        if n < 0:
            series.append((T0 + HOUR * np.arange(6, dtype=np.int64), np.full(6, np.nan)))
        elif n == 0:
            series.append((np.empty(0, np.int64), np.empty(0)))
        else:
            series.append(grow_series(n, 1000 + k))
    S = len(series)
    kw = dict(gamma=0.5 + 0.001 * np.arange(S), tolerance=0.001 + 1e-5 * np.arange(S), size=1000 + np.arange(S),
              iterations=1 + np.arange(S) % 2, mse_tol=0.0)
    dev, host = _both("batch", series, HOUR, **kw)
    assert np.diff(host[0]).tolist() == [max(n, 0) for n in valid]
    assert dev[6].tolist() == [LDS if n <= C else WS for n in valid]
    assert same_state(dev, host)


@pytest.mark.parametrize("iterations", [1, 3])
def test_mixed_branches(iterations):
    dev, host = _both("mixed", [noisy_sine(400, 4, holes=(0, 50, 51, 399))], 3 * HOUR, iterations=iterations, mse_tol=0.0,
                      **MIXED)
    assert 1 < host[0][1] < C and dev[6].tolist() == [LDS]
    assert same_state(dev, host)


@pytest.mark.parametrize("storage", ["lds", "workspace"])
def test_training_further_from_a_non_symmetric_p(storage):
    """a trained state goes in and is trained further; its P is made visibly non-symmetric first, so that a product over
    rows where one over columns belongs (or the reverse) changes the result"""
    t, v = noisy_sine(400, 6)
    first = region.krls_train_csr(*csr([(t[:200], v[:200])]), 3 * HOUR, host=True, **MIXED)
    m = int(first[0][1])
    P = first[4][0] + 1e-3 * np.triu(np.random.default_rng(0).normal(size=(m, m)), 1)
    assert np.abs(P - P.T).max() > 1e-4
    state = (first[0], first[1], first[2], first[3], [P])
    series = [(t[200:], v[200:])]
    if storage == "workspace":  # a second predictor whose start is beyond the LDS capacity: the workspace from the start
        t2, v2 = grow_series(C + 40, 7)
        big = region.krls_train_csr(*csr([(t2[:130], v2[:130])]), HOUR, host=True, **GROW)
        assert C < big[0][1] < C + 40
        state = (np.array([0, m, m + big[0][1]]), np.concatenate([first[1], big[1]]), np.concatenate([first[2], big[2]]),
                 [first[3][0], big[3][0]], [P, big[4][0] + 1e-3 * np.tril(np.ones_like(big[4][0]), -1)])
        series.append((t2[130:], v2[130:]))
        kw = dict(gamma=[MIXED["gamma"], GROW["gamma"]], tolerance=[MIXED["tolerance"], 0.9])  # 0.9: updates, so P is read
        dev, host = _both("further", series, [3 * HOUR, HOUR], state=state, **kw)
        assert dev[6].tolist() == [LDS, WS]
    else:
        dev, host = _both("further", series, 3 * HOUR, state=state, **MIXED)
        assert dev[6].tolist() == [LDS]
    assert same_state(dev, host)
    sym = region.krls_train_csr(*csr(series[:1]), 3 * HOUR, state=(first[0], first[1], first[2], first[3], [P.T]), host=True,
                                **MIXED)
    assert not same_bits(sym[2], host[2][:len(sym[2])])  # the transposed start gives other weights: the case can tell


def test_prediction_shapes():
    """every output count with every dictionary size, as one batch of 24 predictors with parameters of their own; then
    the residuals of the same batch"""
    rng = np.random.default_rng(5)
    counts, sizes = (1, 63, 64, 65, 257, 1000), (1, 64, 65, 300)
    shapes = [(n, m) for n in counts for m in sizes]
    d_row = np.concatenate([[0], np.cumsum([m for _, m in shapes])])
    q_row = np.concatenate([[0], np.cumsum([n for n, _ in shapes])])
    dt = HOUR + US * np.arange(len(shapes))
    gamma = 0.01 + 0.001 * np.arange(len(shapes))
    # dictionaries among the output times, which lie 20 minutes apart from T0 on, in each predictor's own dt units
    d = np.concatenate([(T0 / 1e6) * (1.0 / (dt[k] / 1e6)) + np.sort(rng.uniform(0, max(n / 3.0, 2.0), m))
                        for k, (n, m) in enumerate(shapes)])
    alpha = rng.normal(size=d.shape[0])
    q_t = np.concatenate([T0 + (HOUR // 3) * np.arange(n, dtype=np.int64) for n, _ in shapes])
    got = region.krls_predict(d_row, d, alpha, dt, gamma, q_row, q_t)
    want = region.krls_predict(d_row, d, alpha, dt, gamma, q_row, q_t, host=True)
    assert np.isfinite(want).all()
    assert all(np.abs(want[q_row[k]:q_row[k + 1]]).max() > 1e-3 for k in range(len(shapes)))
    assert same_bits(got, want)
    q_v = rng.normal(size=q_t.shape[0])
    q_v[::5] = np.nan
    got = region.krls_predict(d_row, d, alpha, dt, gamma, q_row, q_t, q_v=q_v)
    assert same_bits(got, region.krls_predict(d_row, d, alpha, dt, gamma, q_row, q_t, q_v=q_v, host=True))
    assert np.isnan(got[::5]).all() and np.isfinite(np.delete(got, np.s_[::5])).all()
    empty = region.krls_predict([0, 0], [], [], HOUR, 0.5, [0, 70], q_t[:70])
    assert same_bits(empty, np.zeros(70))


def _api_series(t, v):
    return api.TimeSeries(api.TimeAxis(int(t[0]) // US, int(t[1] - t[0]) // US, len(t)), v, api.POINT_INSTANT_VALUE)


def test_ts_vector_interpolation_equals_the_single_series_calls():
    series = [noisy_sine(n, 30 + n, holes=(3, n // 2)) for n in (30, 200, 64, 500, 129)]
    tsv = api.TsVector([_api_series(t, v) for t, v in series])
    dts, gammas = [3 * 3600, 2 * 3600, 3600, 3 * 3600, 4 * 3600], [1e-3, 2e-3, 5e-3, 1e-3, 1e-2]
    got = tsv.krls_interpolation(dts, gammas, 0.01)
    assert len(got) == 5
    for k, ts in enumerate(tsv):
        want = ts.krls_interpolation(dts[k], gammas[k], 0.01)
        assert same_bits(got[k].values, want.values)
        assert got[k].point_interpretation() == api.POINT_INSTANT_VALUE and got[k].time(7) == ts.time(7)
    predictors = tsv.get_krls_predictors(dts, gammas, 0.01)
    assert [p.dictionary_size for p in predictors] == [ts.get_krls_predictor(dts[k], gammas[k], 0.01).dictionary_size
                                                        for k, ts in enumerate(tsv)]


def test_reference_sine_through_the_device():
    ta = api.TimeAxis(T0 // US, api.deltahours(1), 30 * 24)
    data = np.sin(np.linspace(0, 2 * np.pi, ta.size()))
    ts = api.TimeSeries(ta, data, api.POINT_INSTANT_VALUE)
    got = api.TsVector([ts]).krls_interpolation(api.deltahours(3))[0]
    assert np.abs(np.array(got.values) - data).max() < 0.05
    assert same_bits(got.values, ts.krls_interpolation(api.deltahours(3)).values)
    row, t, v, t_end, fx = csr([(T0 + HOUR * np.arange(720, dtype=np.int64), data)])
    assert region.krls_train_csr(row, t, v, t_end, fx, 3 * HOUR)[6].tolist() == [LDS]


def test_last_ms_is_positive_after_a_run():
    region.krls_train_csr(*csr([grow_series(20, 3)]), HOUR, **GROW)
    assert region.krls_last_ms() > 0.0


def test_host_path_share():
    """across this file only the two kinds of case that must may have come back by the host path"""
    assert set(_HOST_PATH_CASES) <= {"beyond KRLS_MAX_DICT", "size=8"}
