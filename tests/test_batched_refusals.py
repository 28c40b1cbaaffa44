"""The refusals of the batched series entries (shyft_hip_resample and the four shyft_hip_ts_* entries): malformed
arguments are refused before the first HIP call, so the device entry and its _host twin are both called here without a
GPU, and both must give the same complete message. The expected texts are written out; they are the ones the entries
had when each kept its own copy of the series checks. S = 2 series of 2 and 3 points."""
import numpy as np
import pytest

from shyft_amd import region
from shyft_amd._native import ShyftHipError

SEC = 1000000
I64_MIN = -2 ** 63

IN_ORDER = "time_axis::point_dt() needs time-points in increasing order"
END_OF_AXIS = "time_axis::point_dt() illegal end-of-axis"


def _series():
    return dict(row=np.array([0, 2, 5], dtype=np.int64),
                t=np.array([0, 1, 0, 1, 2], dtype=np.int64) * SEC,
                v=np.array([1.0, 2.0, 3.0, 4.0, 5.0]),
                t_end=np.array([2, 3], dtype=np.int64) * SEC,
                fx=np.array([0, 1], dtype=np.int32))


def _resample(s, host, **kw):
    a = dict(ta_t0=0, ta_dt=SEC, T=4)
    a.update(kw)
    return region.resample_csr(s["row"], s["t"], s["v"], s["t_end"], s["fx"], a["ta_t0"], a["ta_dt"], a["T"],
                               region.RESAMPLE_AVERAGE, host=host)


def _rating(s, host, **kw):
    return region.ts_rating_curve_csr(s["row"], s["t"], s["v"], s["t_end"], s["fx"], pack_row=[0, 1], curve_t=[0],
                                      curve_row=[0, 1], seg=[[0.0, 1.0, 1.0, 0.0]], host=host)


def _ice(s, host, **kw):
    a = dict(qrow=[0, 2, 3], qt=[1 * SEC, 2 * SEC, 2 * SEC], window=SEC, threshold=-1.0,
             policy=region.ICE_ALLOW_ANY_MISSING)
    a.update(kw)
    return region.ts_ice_packing_csr(s["row"], s["t"], s["v"], s["t_end"], s["fx"], a["qrow"], a["qt"], a["window"],
                                     a["threshold"], a["policy"], host=host)


def _recession(s, host, **kw):
    return region.ts_ice_packing_recession_csr(s["row"], s["t"], s["v"], s["t_end"], s["fx"], ice=np.zeros(5),
                                               ice_start=0, ice_end=3 * SEC, alpha=1e-5, recession_minimum=0.0,
                                               host=host)


def _fill(s, host, **kw):
    return region.ts_min_max_fill_csr(s["row"], s["t"], s["v"], s["t_end"], s["fx"], min_x=0.0, max_x=10.0,
                                      max_timespan=10 * SEC, host=host)


ENTRIES = {"resample": (_resample, "resample"), "ts_rating_curve": (_rating, "tsprep"), "ts_ice_packing": (_ice, "tsprep"),
           "ts_ice_packing_recession": (_recession, "tsprep"), "ts_min_max_fill": (_fill, "tsprep")}


def _refused(call, s, expected, **kw):
    texts = []
    for host in (False, True):
        with pytest.raises(ShyftHipError) as e:
            call(s, host, **kw)
        texts.append(str(e.value))
    assert texts[0] == expected  # the device entry, refused before it touches the device
    assert texts[1] == expected  # its _host twin


def test_the_well_formed_batch_is_accepted_by_the_host_twins():
    """the cases below change one thing each in a batch that is not refused"""
    shapes = {"resample": (4, 2), "ts_ice_packing": (3,)}
    for entry, (call, _) in ENTRIES.items():
        assert call(_series(), True).shape == shapes.get(entry, (5,))


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_decreasing_row_is_refused(entry):
    call, prefix = ENTRIES[entry]
    s = _series()
    s["row"] = np.array([0, 6, 5], dtype=np.int64)
    _refused(call, s, prefix + ": row must not decrease")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_fx_2_is_refused(entry):
    call, prefix = ENTRIES[entry]
    s = _series()
    s["fx"][1] = 2
    _refused(call, s, prefix + ": fx must be POINT_INSTANT_VALUE or POINT_AVERAGE_VALUE")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_equal_consecutive_times_are_refused(entry):
    call, _ = ENTRIES[entry]
    s = _series()
    s["t"][4] = s["t"][3]
    _refused(call, s, IN_ORDER)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_t_end_equal_to_the_last_time_is_refused(entry):
    call, _ = ENTRIES[entry]
    s = _series()
    s["t_end"][0] = s["t"][1]
    _refused(call, s, END_OF_AXIS)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_first_time_below_a_quarter_of_the_range_is_refused(entry):
    call, prefix = ENTRIES[entry]
    s = _series()
    s["t"][0] = I64_MIN // 4 - 1
    _refused(call, s, prefix + ": times beyond a quarter of the 64-bit range are not supported")


def test_resample_refuses_a_zero_delta_t():
    _refused(_resample, _series(), "resample: the time-axis needs a delta-t larger than 0", ta_dt=0)


def test_ice_packing_refuses_a_decreasing_qrow():
    _refused(_ice, _series(), "tsprep: row must not decrease", qrow=[0, 4, 3])


def test_ice_packing_refuses_policy_3():
    _refused(_ice, _series(),
             "ice_packing: policy must be DISALLOW_MISSING, ALLOW_INITIAL_MISSING or ALLOW_ANY_MISSING", policy=3)


def test_ice_packing_refuses_a_negative_window():
    _refused(_ice, _series(), "ice_packing: the window must lie in 0 .. a quarter of the 64-bit range", window=-1)
