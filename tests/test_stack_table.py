"""What the C ABI knows about each method stack, through HipRegion: the accepted parameter-row widths and the
reference's `.set size` texts, the snow-bin check, the state field count and the state-collector series count.
One row per stack below; every stack is asked the same questions."""
import numpy as np
import pytest

from shyft_amd import synthetic
from shyft_amd._native import ShyftHipError
from shyft_amd.region import (COLLECT_DISCHARGE, HBV_STACK, HipRegion, PT_GS_K, PT_HPS_K, PT_HS_K, PT_SS_K)

pytestmark = pytest.mark.gpu

N = 3
DIST = 1 + 2 * 8  # n_bins, s[8], intervals[8]

# name: (stack id, reference width, device row width or None where the stack has no snow distribution,
#        a width the stack refuses although another stack's row has it, `.set size` text,
#        state fields, state-collector series, default reference row)
STACKS = {
    "pt_gs_k": (PT_GS_K, 31, None, 36, "PTGSK Parameter Accessor: .set size missmatch", 9, 9,
                synthetic.default_ptgsk_parameters),
    "hbv_stack": (HBV_STACK, 22, 22 + DIST, None, "HBV_Stack Parameter Accessor: .set size missmatch", 22, 22,
                  synthetic.default_hbv_parameters),
    "pt_ss_k": (PT_SS_K, 21, None, 21 + DIST, "pt_ss_k parameter accessor: .set size mismatch", 8, 7,
                synthetic.default_ptssk_parameters),
    "pt_hs_k": (PT_HS_K, 18, 18 + DIST, None, "pt_ss_k parameter accessor: .set size missmatch", 20, 19,
                synthetic.default_pthsk_parameters),
    "pt_hps_k": (PT_HPS_K, 24, 24 + 1 + DIST, None, "pt_ss_k parameter accessor: .set size missmatch", 37, 36,
                 synthetic.default_pthpsk_parameters),
}


@pytest.fixture(params=list(STACKS))
def stack(request):
    sid, n_ref, width, refused, text, n_state, n_state_series, defaults = STACKS[request.param]
    r = HipRegion(sid, N)
    try:
        yield r, n_ref, width, refused, text, n_state, n_state_series, defaults()
    finally:
        r.close()


def _full_row(ref, width, n_bins=5):
    """The device row: the reference values, zeros up to the distribution (pt_hps_k's gm.direct_response), then
    n_bins, s[8] = 1 and intervals[8] evenly spaced over the bins in use."""
    row = np.zeros(width)
    row[:ref.size] = ref
    d = width - DIST
    row[d] = n_bins
    k = min(max(n_bins, 0), 8)
    row[d + 1:d + 1 + k] = 1.0
    row[d + 9:d + 9 + k] = np.linspace(0.0, 1.0, k) if k > 1 else 0.0
    return row


def _refused(r, row, text):
    with pytest.raises(ShyftHipError) as e:
        r.set_parameters(row)
    assert str(e.value) == text


def test_parameter_row_widths(stack):
    r, n_ref, width, refused, text, _, _, ref = stack
    assert ref.size == n_ref
    r.set_parameters(ref)
    r.set_parameters(np.stack([ref, ref]), np.array([0, 1, 0], dtype=np.int32))
    _refused(r, ref[:-1], text)
    _refused(r, np.append(ref, 0.0), text)
    if width is not None:
        r.set_parameters(_full_row(ref, width))
        _refused(r, _full_row(ref, width)[:-1], text)
        _refused(r, np.append(_full_row(ref, width), 0.0), text)
    else:
        _refused(r, np.zeros(refused), text)


def test_snow_bin_count_is_checked_in_a_full_row(stack):
    r, _, width, _, _, _, _, ref = stack
    if width is None:
        return  # no snow distribution in this stack's row: nothing to check
    for nb in (2, 8):
        r.set_parameters(_full_row(ref, width, nb))
    for nb in (1, 9):
        _refused(r, _full_row(ref, width, nb), "hbv_snow: number of snow bins must be in [2, 8]")


def test_state_field_count(stack):
    r, _, _, _, _, n_state, _, _ = stack
    st = np.arange(N * n_state, dtype=np.float64).reshape(N, n_state)
    with pytest.raises(ShyftHipError) as e:
        r.set_state(np.zeros((N, n_state + 1)))
    assert str(e.value) == "set_state: wrong number of state fields"
    r.set_state(st)
    got = r.get_state()
    assert got.shape == (N, n_state)
    assert np.array_equal(got, st)
    with pytest.raises(ShyftHipError) as e:
        r.get_state(n_state + 1)
    assert str(e.value) == "get_state: wrong number of state fields"


def test_state_series_count(stack):
    r, _, _, _, _, _, n_state_series, _ = stack
    T = 4
    r.set_time_axis(synthetic.T0_2015_US, synthetic.HOUR_US, T)
    with pytest.raises(ShyftHipError) as e:
        r.get_state_series(0, 0, T + 1)
    assert str(e.value) == "get_state_series: state collection is off"
    r.set_collection(COLLECT_DISCHARGE, True)
    for k in range(n_state_series):
        assert r.get_state_series(k, 0, T + 1).shape == (T + 1, N)
    with pytest.raises(ShyftHipError) as e:
        r.get_state_series(n_state_series, 0, T + 1)
    assert str(e.value) == "get_state_series: invalid field"


@pytest.mark.parametrize("devices", [None, [0]], ids=["plain", "sharded"])
def test_unknown_stack_id_is_refused(devices):
    with pytest.raises(ShyftHipError) as e:
        HipRegion(99, N, devices=devices)
    assert str(e.value) == "shyft_hip_region_create: unsupported method stack"
