"""The Brent opening of the 256-lane pt_gs_k run kernels (gs_brent_job_open, device/gs_brent.h), bit for bit.

A workgroup-step with at most 16 (32) Brent jobs gives each job 4 (2) neighbouring lanes of the solving wavefront:
the lanes evaluate f at the first points of brent_find_minima at once, the group's first lane takes the siblings'
values across lanes and runs the solver, looking its first points up among them. f is a pure function of its
argument, so every result is the one-lane solver's (kernels/ptgsk.hip).

Job level: shyft_hip_device_selftest's BRENT_OPEN4 / BRENT_OPEN2 run the job entry as the run kernel calls it, 16 or
32 jobs per workgroup, against gs_corr_lwc (BRENT's first column), on the recorded January jobs, the edge jobs of
tests/test_device_functions.py and a sweep of small z1 where the tolerance test ends the search before the first or
the second iteration (counted on the CPU with tools/ptgsk_brent_opening_count.py's restatement of the solver).

Kernel level: the 300-cell region and the January and autumn windows of tests/test_ptgsk_lgamma_queue.py, and a
third window of 48 steps whose temperature and precipitation are the same in every cell (four hours of snowfall, four
of rain, repeated), so that every lane of a workgroup has a job in the same step: 256 jobs in the first workgroup and
44 in the second. The module asserts from the oracle replay that the windows hold workgroup-steps with 1-16, 17-32,
33-64 and more than 64 jobs before any GPU result is looked at."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

from shyft_amd import synthetic
from tests import test_ptgsk_lgamma_queue as q
from tests.test_device_functions import BRENT, BRENT_EDGE, GOLDEN, _assert_bits, _device

pytestmark = pytest.mark.gpu

BRENT_OPEN4, BRENT_OPEN2 = 11, 12   # function codes of include/shyft_hip.h
N = q.N
T3 = 48                             # the uniform-forcing window
CLASSES = {"1-16": (1, 16), "17-32": (17, 32), "33-64": (33, 64), ">64": (65, q.BLOCK)}


def _count_tool():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "ptgsk_brent_opening_count.py")
    spec = importlib.util.spec_from_file_location("ptgsk_brent_opening_count", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ------------------------------------------------------------------------------------------------ job level
@functools.lru_cache(maxsize=None)
def _jobs():
    """z1 a1 b1 a2 b2 rows: recorded, edge (series / continued-fraction rescale, points at and below 0, |exp
    argument| > 708: f takes gs_calc_q_general; both gamma policies) and small z1. The count is 21 mod 32: the last
    workgroup of either entry is ragged, and the last one of the 32-job entry still has 17-32 jobs (groups of 2)."""
    rec = np.load(os.path.join(GOLDEN, "brent_jobs_sample.npy"))
    small = np.array([(z1, a, b, a * 1.1, b * 0.95) for a, b in ((6.25, 0.01), (0.5, 0.5))
                      for z1 in np.geomspace(1e-5, 2e-3, 24)])
    jobs = np.concatenate([rec, np.array(BRENT_EDGE), small])
    jobs = jobs[:len(jobs) - (len(jobs) - 21) % 32]
    assert len(jobs) % 32 == 21 and len(jobs) % 16 != 0
    assert len(jobs) > len(rec) + len(BRENT_EDGE) + 40   # the small-z1 rows are not the ones cut
    return jobs


@functools.lru_cache(maxsize=None)
def _evaluations_of_small_jobs():
    """f evaluations of the solver on the small-z1 rows, on the CPU (the oracle's incomplete gamma)."""
    from tests import oracle_lib
    tool = _count_tool()
    lib = oracle_lib.load("detmath")
    d = C.c_double
    lib.oracle_gamma_pq_policy.restype = None
    lib.oracle_gamma_pq_policy.argtypes = [d, d, C.POINTER(d), C.POINTER(d), C.POINTER(d)]
    p, p1, pre = d(), d(), d()

    def calc_q(a, b, z):
        lib.oracle_gamma_pq_policy(a, z / b, C.byref(p), C.byref(p1), C.byref(pre))
        return a * b * p1.value + z * (1.0 - p.value)
    n = []
    for z1, a1, b1, a2, b2 in _jobs()[2048 + len(BRENT_EDGE):].tolist():
        Q1 = calc_q(a1, b1, z1)
        n.append(len(tool.brent(lambda z: (calc_q(a2, b2, z) - Q1) ** 2, z1)[1]))
    return np.array(n)


def test_small_jobs_end_before_the_first_and_the_second_iteration():
    """A condition of the job-level test, from the CPU alone: the sweep holds jobs whose search ends with 1
    evaluation (no iteration: the opening's other points are wasted), with 2 (the second lookup is never made) and
    with more."""
    n = _evaluations_of_small_jobs()
    print("f evaluations of the small-z1 jobs:", np.bincount(n))
    assert (n == 1).any() and (n == 2).any() and (n >= 4).any()


@pytest.mark.parametrize("mode", [0, 1])
def test_job_entry_in_groups_of_4_and_2(mode):
    """gs_brent_job_open on 4 and 2 lanes per job equals gs_corr_lwc bit for bit, with Q1 left to the job (mode 0:
    q1 = NaN) or supplied (mode 1)."""
    _evaluations_of_small_jobs()
    jobs = _jobs()
    cols = [np.ascontiguousarray(jobs[:, k]) for k in range(5)] + [np.full(len(jobs), float(mode))]
    ref = _device(BRENT, cols, 2)[0]
    assert np.isfinite(ref[:2048]).all()
    _assert_bits(_device(BRENT_OPEN4, cols, 1)[0], ref, f"job entry, groups of 4, q1 mode {mode}", *cols[:5])
    _assert_bits(_device(BRENT_OPEN2, cols, 1)[0], ref, f"job entry, groups of 2, q1 mode {mode}", *cols[:5])


# ------------------------------------------------------------------------------------------------ kernel level
@functools.lru_cache(maxsize=None)
def _uniform_forcing():
    f = synthetic.forcing(N, 0, T3).copy()
    snow = (np.arange(T3) % 8) < 4
    f[0][:] = np.where(snow, -6.0, 3.0)[:, None]   # temperature, deg C
    f[1][:] = np.where(snow, 4.0, 2.0)[:, None]    # precipitation, mm/h
    return f


@functools.lru_cache(maxsize=None)
def _oracle_uniform(override=False, step0=0):
    from tests import oracle_lib
    p, ix = q._params(override)
    return oracle_lib.ptgsk_run(q._geo(), p, synthetic.default_ptgsk_state(N), synthetic.T0_2015_US, synthetic.HOUR_US,
                                _uniform_forcing(), start_step=step0, n_steps=T3 - step0, set_ix=ix, full=True,
                                collect_state=True)


@functools.lru_cache(maxsize=None)
def _hip_uniform(collect, state_series=False, cids=None, override=False, delay=0, step0=0):
    """tests/test_ptgsk_lgamma_queue._hip on the uniform-forcing window."""
    from shyft_amd.region import HipRegion, PT_GS_K, KNOB_PTGSK_INSTANCE, KNOB_BRENT_READ_DELAY
    p, ix = q._params(override)
    f = _uniform_forcing()
    r = HipRegion(PT_GS_K, N, device=0)
    try:
        r.set_geo(q._geo())
        r.set_parameters(p, ix)
        r.set_time_axis(synthetic.T0_2015_US, synthetic.HOUR_US, T3)
        r.set_collection(collect, state_series)
        r.set_state(synthetic.default_ptgsk_state(N))
        if cids is not None:
            r.set_catchment_filter(list(cids))
        r.set_test_knob(KNOB_PTGSK_INSTANCE, 4)
        r.set_test_knob(KNOB_BRENT_READ_DELAY, delay)
        for v in range(5):
            r.set_forcing(v, 0, f[v])
        r.run_cells(0, step0, T3 - step0)
        ns = (2, 4, 8)[collect]
        return {"series": np.stack([r.get_series(k, 0, T3) for k in range(ns)]), "state": r.get_state(),
                "state_series": np.stack([r.get_state_series(k, 0, T3 + 1) for k in range(9)]) if state_series
                else None}
    finally:
        r.close()


def _job_counts(window):
    """Brent jobs per workgroup-step [T][2] of a window, from the oracle replay."""
    if window == "uniform":
        f = _uniform_forcing()
        return q.lgamma_events(_oracle_uniform()["state_series"], f[0], f[1], synthetic.default_ptgsk_parameters())["n_job"]
    return q._events(window)["n_job"]


@functools.lru_cache(maxsize=None)
def _assert_classes():
    """From the oracle alone: the January and autumn windows hold workgroup-steps with 1-16, 17-32 and 33-64 jobs
    (the entry's three group sizes), the uniform window steps with more than 64 (every wavefront solves, one lane
    per job, several jobs per lane of none) and with 33-64 in its second workgroup."""
    k = {w: {c: int(((_job_counts(w) >= lo) & (_job_counts(w) <= hi)).sum()) for c, (lo, hi) in CLASSES.items()}
         for w in list(q.WINDOWS) + ["uniform"]}
    print(k)
    for c in ("1-16", "17-32", "33-64"):
        assert sum(k[w][c] for w in q.WINDOWS) > 0, c
    assert k["uniform"][">64"] > 0 and k["uniform"]["33-64"] > 0
    assert (_job_counts("uniform")[:, 0] == q.BLOCK).any()   # every lane of a workgroup in the queue at one step
    # both group sizes at their limits or next to them somewhere in the windows
    nj = np.concatenate([_job_counts(w).ravel() for w in q.WINDOWS])
    assert ((nj >= 14) & (nj <= 16)).any() and ((nj >= 17) & (nj <= 19)).any() and ((nj >= 30) & (nj <= 34)).any()


@pytest.fixture(scope="module", autouse=True)
def classes_checked():
    """Before any GPU result is compared: the windows exercise every job class."""
    _assert_classes()


def test_windows_hold_every_job_class():
    _assert_classes()


def _runs(window):
    """(_hip, _oracle, length) of a window."""
    if window == "uniform":
        return _hip_uniform, _oracle_uniform, T3
    return functools.partial(q._hip, window), functools.partial(q._oracle, window), q.T


WINDOWS = sorted(q.WINDOWS) + ["uniform"]


@pytest.mark.parametrize("window", WINDOWS)
def test_lean_instance_equals_oracle(window):
    hip, oracle, _ = _runs(window)
    q._check_oracle(hip(0), oracle())


@pytest.mark.parametrize("window", WINDOWS)
def test_general_instance_with_state_series_equals_oracle(window):
    hip, oracle, _ = _runs(window)
    g = hip(2, True)
    q._check_oracle(g, oracle())
    assert (g["series"][3] > 0).any()   # a snow pack


@pytest.mark.parametrize("window", WINDOWS)
def test_per_cell_parameter_sets(window):
    """A second parameter set for catchment 2: the per-cell parameter instances, lean and general."""
    hip, oracle, _ = _runs(window)
    o = oracle(override=True)
    q._check_oracle(hip(0, override=True), o)
    q._check_oracle(hip(2, True, override=True), o)
    assert not q._same(o["full"][0], oracle()["full"][0])


@pytest.mark.parametrize("window", WINDOWS)
def test_odd_first_step(window):
    hip, oracle, _ = _runs(window)
    o = oracle(step0=q.ODD_STEP0)
    q._check_oracle(hip(0, step0=q.ODD_STEP0), o, q.ODD_STEP0)
    q._check_oracle(hip(2, True, step0=q.ODD_STEP0), o, q.ODD_STEP0)


@pytest.mark.parametrize("window", WINDOWS)
def test_catchment_filter_through_a_wavefront(window):
    """Catchments 1 and 3 only: lanes 50-99 and 200-249 are off; they queue no job and their state stays."""
    hip, oracle, _ = _runs(window)
    on = np.isin(q._geo()[:, 4], (1, 3))
    assert 0 < on[:64].sum() < 64 and 0 < on[64:128].sum() < 64
    for g in (hip(0, cids=(1, 3)), hip(2, True, cids=(1, 3))):
        q._check_oracle(g, oracle(), on=on)
        assert np.array_equal(g["state"][~on], synthetic.default_ptgsk_state(N)[~on])


@pytest.mark.parametrize("window", WINDOWS)
def test_late_readers(window):
    """read_delay 3 (general instance): three wavefronts read their Brent results late, while the first is already
    queueing the next step's jobs into the arrays the opening read."""
    hip, oracle, _ = _runs(window)
    q._check_oracle(hip(0, delay=3), oracle())
    q._check_oracle(hip(2, True, delay=3), oracle())
