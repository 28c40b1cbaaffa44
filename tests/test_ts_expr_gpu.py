"""Time-series arithmetic on the GPU (kernels/ts_expr.hip): region.ts_expr_csr on the device is bit-identical, NaN
matching NaN, to host=True (which runs host/ts_expr.hpp and is itself pinned by tests/test_ts_expr_host.py), then the
TsVector path, the host fall-back beyond the device's limits, and the counters.

Batches are those of tests/ts_expr_cases.py over tests/resample_cases.py: E = 1 / 63 / 64 / 65 / 257 expressions,
terminal lengths rotating over 0, 1, 2, 3, 63, 64, 65, 257, 1000, three time bases, both point types, NaN / inf
hazards, every expression shape the device takes; where E allows, expression 8 has a root axis of 3,300 points, so one
expression spans 52 wavefronts and the expressions after it start at every kind of offset inside a workgroup."""
import numpy as np
import pytest

from tests import resample_cases as rc
from tests import ts_expr_cases as xc

pytestmark = pytest.mark.gpu

ES = (1, 63, 64, 65, 257)
N_LONG = 3300


@pytest.fixture(scope="module")
def region():
    from shyft_amd import region
    return region


def _same(dev, host, what):
    bad = np.argwhere(~((np.isnan(dev) & np.isnan(host)) | (dev.view(np.uint64) == host.view(np.uint64))))
    assert rc.same_bits(dev, host), (what, len(bad), bad[:4].tolist())


def _device_equals_host(region, trees, what):
    plan = xc.Plan(trees)
    host = region.ts_expr_csr(*plan.args(), host=True)
    dev = region.ts_expr_csr(*plan.args())
    assert dev.shape == (plan.orow[-1],)
    _same(dev, host, what)
    return plan


@pytest.mark.parametrize("k,E", list(enumerate(ES)))
def test_batches_are_bit_identical_to_host(region, k, E):
    # E == 1: tree 0 of the batch would be over a terminal without points; start the shapes at the 257-point one
    trees = xc.batch_trees(E, k + (7 if E == 1 else 0), long_points=N_LONG)
    plan = _device_equals_host(region, trees, E)
    assert plan.depth.max() <= 8 and np.diff(plan.prog_row).max() <= 64
    if E > 8:
        assert plan.orow[9] - plan.orow[8] == N_LONG
    if E >= 63:
        assert plan.depth.max() == 8  # the depth-8 chains are in


def test_every_shape_on_every_axis_pair_is_bit_identical_to_host(region):
    trees = []
    for fx_a, fx_b in ((0, 1), (1, 0)):
        c = xc._axis([1.5, 2.5, 6.25, 9], 30, 0, 99)
        for name in xc.DEVICE_SHAPES:
            trees += [xc.SHAPES[name](a, b, c, a.twin(j)) for j, (a, b) in enumerate(xc.axis_pairs(fx_a, fx_b).values())]
    _device_equals_host(region, trees, "axis pairs")


def test_value_hazards_are_bit_identical_to_host(region):
    trees = []
    c = xc._axis([1.5, 2.5, 6.25], 30, 0, 98)
    for name in xc.DEVICE_SHAPES:
        for j, (a, b) in enumerate(xc.hazard_pairs().values()):
            trees += [xc.SHAPES[name](a, b, c, a.twin(j)), xc.SHAPES[name](b, a, c, b.twin(j))]
    _device_equals_host(region, trees, "hazards")


def _vector(api, n=40):
    ta = api.TimeAxis(0, 3600, n)
    rng = np.random.default_rng(3)
    a = api.TimeSeries(ta, rng.normal(0, 3, n).tolist(), api.POINT_AVERAGE_VALUE)
    b = api.TimeSeries(api.TimeAxis(1800, 3600, n), rng.normal(0, 3, n).tolist(), api.POINT_INSTANT_VALUE)
    return a, b, lambda: api.TsVector([a + b * 3.0 - a / 2.0, api.max(a, b).abs(), a, -a, a.pow(2.0) + b.time_shift(1800)])


def test_tsvector_evaluate_equals_host_and_counts_one_call(region):
    from shyft_amd import api
    _, _, make = _vector(api)
    calls = region.ts_expr_calls()
    dev = make().evaluate()
    assert region.ts_expr_calls() == calls + 1  # the whole vector in one call
    assert region.ts_expr_last_ms() > 0.0
    host = make().evaluate(host=True)
    assert region.ts_expr_calls() == calls + 1
    for d, h in zip(dev, host):
        assert d.point_interpretation() == h.point_interpretation() and d.total_period().end == h.total_period().end
        assert [d.time(i) for i in range(d.size())] == [h.time(i) for i in range(h.size())]
        _same(np.asarray(d.values), np.asarray(h.values), "evaluate")
    lazy = make()[0]
    one = lazy.evaluate()
    assert region.ts_expr_calls() == calls + 2
    _same(np.asarray(one.values), np.asarray(lazy.values), "the result is kept")
    _same(np.asarray(one.values), np.asarray(host[0].values), "one series")
    assert region.ts_expr_calls() == calls + 2  # reading the evaluated expression computes nothing


def test_a_depth_9_chain_evaluates_on_the_host_path(region):
    from shyft_amd import api
    a, b, _ = _vector(api)
    chain = a
    for _ in range(4):
        chain = a + (b + chain)  # right-deep, nine terminals
    shallow = a * 2.0
    calls = region.ts_expr_calls()
    got = api.TsVector([chain]).evaluate()
    assert region.ts_expr_calls() == calls  # beyond the device's stack: the host twin, no launch
    want = api.TsVector([a + (b + (a + (b + (a + (b + (a + (b + a)))))))]).evaluate(host=True)
    _same(np.asarray(got[0].values), np.asarray(want[0].values), "depth 9")
    both = api.TsVector([a + (b + (a + (b + (a + (b + (a + (b + a))))))), shallow]).evaluate()
    assert region.ts_expr_calls() == calls + 1  # the shallow one went to the device, the deep one did not
    _same(np.asarray(both[0].values), np.asarray(want[0].values), "depth 9 next to a device expression")
    assert list(both[1].values) == [2.0 * x for x in a.values]


def test_nothing_to_do_launches_nothing(region):
    a, b = xc.axis_pairs()["disjoint"]
    calls = region.ts_expr_calls()
    empty = xc.Plan([(xc.TS_TS, xc.ADD, a, b)])  # one expression without points
    assert region.ts_expr_csr(*empty.args()).shape == (0,)
    none = xc.Plan([])
    assert region.ts_expr_csr(*none.args()).shape == (0,)
    assert region.ts_expr_calls() == calls


def test_calls_and_last_ms_move_with_device_calls_only(region):
    a, b = xc.axis_pairs()["interleaved"]
    plan = xc.Plan([(xc.TS_TS, xc.MUL, a, b)])
    calls = region.ts_expr_calls()
    region.ts_expr_csr(*plan.args(), host=True)
    assert region.ts_expr_calls() == calls
    region.ts_expr_csr(*plan.args())
    assert region.ts_expr_calls() == calls + 1 and 0.0 < region.ts_expr_last_ms() < 1000.0
