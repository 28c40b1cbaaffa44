"""Thin Python owner of a C-ABI region handle (include/shyft_hip.h).

This is plumbing for tests, the bench and the Python API layer: every call
goes straight to libshyft_hip.so. Arrays are numpy (host) or, where a
function takes `on_device`, a raw device pointer (e.g. torch tensor.data_ptr()).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._native import check, lib

PT_GS_K, HBV_STACK, PT_SS_K, PT_HS_K, PT_HPS_K = 1, 2, 3, 4, 5
TEMPERATURE, PRECIPITATION, WIND_SPEED, REL_HUM, RADIATION = range(5)
FORCING_NAMES = ("temperature", "precipitation", "wind_speed", "rel_hum", "radiation")
COLLECT_DISCHARGE, COLLECT_DISCHARGE_SNOW, COLLECT_ALL = 0, 1, 2
PTGSK_SERIES = ("avg_discharge", "charge_m3s", "snow_sca", "snow_swe", "snow_outflow", "glacier_melt", "ae_output",
                "pe_output")
PTGSK_STATE = ("albedo", "lwc", "surface_heat", "alpha", "sdc_melt_mean", "acc_melt", "iso_pot_energy", "temp_swe",
               "kirchner_q")
HBV_SERIES = ("avg_discharge", "charge_m3s", "snow_sca", "snow_swe", "snow_outflow", "glacier_melt", "ae_output",
              "pe_output", "soil_outflow")
HBV_MAX_BINS = 8
HBV_STATE = (("swe", "sca", "soil_moisture", "tank_uz", "tank_lz", "n_bins") +
             tuple(f"sp{i}" for i in range(HBV_MAX_BINS)) + tuple(f"sw{i}" for i in range(HBV_MAX_BINS)))
SCOPE_CELL_IX, SCOPE_CATCHMENT = 0, 1
SERIES_FORCING, SERIES_STATE = 100, 200
KNOB_PTGSK_INSTANCE, KNOB_BRENT_READ_DELAY, KNOB_SERIAL_SHARDS, KNOB_CLONE_FAIL_AT = 1, 2, 3, 4
KNOB_PERCENTILES_PATH = 5  # 0 auto, 1 LDS sort, 2 radix select
# shyft_hip_percentiles (include/shyft_hip.h): list cap, LDS-sort segment limit, statistics_property, path names
PERCENTILES_MAX, PERCENTILES_LDS_MAX = 16, 4096
STAT_AVERAGE, STAT_MIN_EXTREME, STAT_MAX_EXTREME = -1, -1000, 1000
PERCENTILES_PATHS = ("none", "lds_sort", "radix")
# shyft_hip_region_create_sharded_ex options (include/shyft_hip.h)
SHARD_RCCL_ALWAYS, SHARD_NO_RCCL, SHARD_TEST_FAIL_INIT, SHARD_TEST_FAIL_GATHER, SHARD_TEST_CORRUPT_CHECK = 1, 2, 4, 8, 16
SHARD_BALANCE_Z = 32
SHARD_TEST_STALL_CHECK = 64
# pt_ss_k (core/pt_ss_k.h:154-181, pt_ss_k_cell_model.h:38-200); response series ids are the pt_gs_k ones
PTSSK_STATE = ("nu", "alpha", "sca", "swe", "free_water", "residual", "num_units", "kirchner_q")
PTSSK_STATE_SERIES = ("kirchner_discharge", "snow_sca", "snow_swe", "snow_alpha", "snow_nu", "snow_lwc",
                      "snow_residual")
# pt_hs_k (core/pt_hs_k.h:148-172, pt_hs_k_cell_model.h:148-210); response series ids are the pt_gs_k ones
PTHSK_STATE = (("swe", "sca", "n_bins") + tuple(f"sp{i}" for i in range(HBV_MAX_BINS)) +
               tuple(f"sw{i}" for i in range(HBV_MAX_BINS)) + ("kirchner_q",))
PTHSK_STATE_SERIES = (("kirchner_discharge", "snow_sca", "snow_swe") + tuple(f"sp{i}" for i in range(HBV_MAX_BINS)) +
                      tuple(f"sw{i}" for i in range(HBV_MAX_BINS)))
# pt_hps_k (core/pt_hps_k.h:163-185, pt_hps_k_cell_model.h:160-232); response series ids are the pt_gs_k ones
_B = tuple(range(HBV_MAX_BINS))
PTHPSK_STATE = (("swe", "sca", "surface_heat", "n_bins") + tuple(f"sp{i}" for i in _B) + tuple(f"sw{i}" for i in _B) +
                tuple(f"albedo{i}" for i in _B) + tuple(f"iso_pot_energy{i}" for i in _B) + ("kirchner_q",))
PTHPSK_STATE_SERIES = (("kirchner_discharge", "hps_sca", "hps_swe", "hps_surface_heat") +
                       tuple(f"sp{i}" for i in _B) + tuple(f"sw{i}" for i in _B) + tuple(f"albedo{i}" for i in _B) +
                       tuple(f"iso_pot_energy{i}" for i in _B))
STACK_NPARAM = {PT_GS_K: 31, HBV_STACK: 22, PT_SS_K: 21, PT_HS_K: 18, PT_HPS_K: 24}
STACK_NSTATE = {PT_GS_K: 9, HBV_STACK: len(HBV_STATE), PT_SS_K: len(PTSSK_STATE), PT_HS_K: len(PTHSK_STATE),
                PT_HPS_K: len(PTHPSK_STATE)}
STACK_NSERIES = {PT_GS_K: len(PTGSK_SERIES), HBV_STACK: len(HBV_SERIES), PT_SS_K: len(PTGSK_SERIES),
                 PT_HS_K: len(PTGSK_SERIES), PT_HPS_K: len(PTGSK_SERIES)}


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HipRegion:
    """A region on one device, or -- with `devices` (a list, one entry per shard, repeats allowed) -- one region
    whose cells are split into len(devices) contiguous shards driven from this process
    (shyft_hip_region_create_sharded): every method below then works on the whole region."""

    def __init__(self, stack: int, n_cells: int, device: int = -1, devices=None, shard_flags: int = 0):
        self._L = lib()
        h = C.c_void_p()
        if devices is None:
            check(self._L.shyft_hip_region_create(stack, n_cells, device, C.byref(h)), None)
        else:
            d = np.ascontiguousarray(list(devices), dtype=np.int32)
            check(self._L.shyft_hip_region_create_sharded_ex(stack, n_cells, _ptr(d), d.size, int(shard_flags),
                                                             C.byref(h)), None)
        self.h = h
        self.stack = stack
        self.n = n_cells
        self.n_steps = 0
        self.window = 0

    def shards(self) -> list:
        """[(device, first cell, n_cells)] of every shard ([(device, 0, n)] for an unsharded region)."""
        dev, c0, nc = C.c_int(), C.c_size_t(), C.c_size_t()
        S = int(self._L.shyft_hip_region_shards(self.h, 0, None, None, None))
        out = []
        for k in range(S):
            self._L.shyft_hip_region_shards(self.h, k, C.byref(dev), C.byref(c0), C.byref(nc))
            out.append((dev.value, c0.value, nc.value))
        return out

    def combine_path(self) -> str:
        """How shard partial sums are combined: "none" (unsharded), "copy" (shards share a device), "rccl"."""
        return ("none", "copy", "rccl")[int(self._L.shyft_hip_region_combine_path(self.h))]

    def combine_report(self) -> str:
        """The combine path's decision: why RCCL or copies, the RCCL self-check result, run-time fallbacks."""
        r = self._L.shyft_hip_region_combine_report(self.h)
        return r.decode() if r else ""

    def close(self):
        if getattr(self, "h", None):
            self._L.shyft_hip_region_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, status):
        check(status, self.h)

    def set_geo(self, geo11: np.ndarray, routing_id=None, routing_distance=None):
        g = np.ascontiguousarray(geo11, dtype=np.float64).reshape(self.n, 11)
        rid = None if routing_id is None else np.ascontiguousarray(routing_id, dtype=np.int64)
        rd = None if routing_distance is None else np.ascontiguousarray(routing_distance, dtype=np.float64)
        self._chk(self._L.shyft_hip_set_geo(self.h, _ptr(g), _ptr(rid), _ptr(rd)))

    def set_parameters(self, params: np.ndarray, set_ix: np.ndarray | None = None):
        p = np.ascontiguousarray(params, dtype=np.float64)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        ix = None if set_ix is None else np.ascontiguousarray(set_ix, dtype=np.int32)
        self._chk(self._L.shyft_hip_set_parameters(self.h, _ptr(p), p.shape[0], p.shape[1], _ptr(ix)))

    def set_time_axis(self, t0_us: int, dt_us: int, n_steps: int, window_steps: int = 0):
        self._chk(self._L.shyft_hip_set_time_axis(self.h, int(t0_us), int(dt_us), int(n_steps), int(window_steps)))
        self.n_steps = n_steps
        self.window = n_steps if window_steps in (0, None) or window_steps > n_steps else window_steps

    def set_window(self, w0: int):
        self._chk(self._L.shyft_hip_set_window(self.h, int(w0)))

    def move_window(self, w0: int, fill_mask: int = 0):
        """set_window without (or with a subset of) the NaN fill; for callers that rewrite the whole window."""
        self._chk(self._L.shyft_hip_move_window(self.h, int(w0), int(fill_mask)))

    def set_collection(self, collect: int, collect_state: bool = False):
        self._chk(self._L.shyft_hip_set_collection(self.h, int(collect), int(bool(collect_state))))

    def set_catchment_filter(self, cids):
        c = np.ascontiguousarray(cids, dtype=np.int64)
        self._chk(self._L.shyft_hip_set_catchment_filter(self.h, _ptr(c) if c.size else None, c.size))

    def set_state(self, state: np.ndarray):
        s = np.ascontiguousarray(state, dtype=np.float64).reshape(self.n, -1)
        self._chk(self._L.shyft_hip_set_state(self.h, _ptr(s), s.shape[1]))

    def get_state(self, n_fields: int | None = None) -> np.ndarray:
        nf = n_fields or STACK_NSTATE[self.stack]
        s = np.empty((self.n, nf), dtype=np.float64)
        self._chk(self._L.shyft_hip_get_state(self.h, _ptr(s), nf))
        return s

    def copy_state_from(self, src: "HipRegion"):
        """This region's state := src's state, device to device (same stack and cell count)."""
        self._chk(self._L.shyft_hip_copy_state(self.h, src.h))

    def set_forcing(self, var: int, step0: int, values: np.ndarray):
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.n)
        self._chk(self._L.shyft_hip_set_forcing(self.h, var, step0, v.shape[0], _ptr(v), 0))

    def set_forcing_device(self, var: int, step0: int, n: int, dev_ptr: int):
        self._chk(self._L.shyft_hip_set_forcing(self.h, var, step0, n, C.c_void_p(dev_ptr), 1))

    def get_forcing(self, var: int, step0: int, n: int) -> np.ndarray:
        out = np.empty((n, self.n), dtype=np.float64)
        self._chk(self._L.shyft_hip_get_forcing(self.h, var, step0, n, _ptr(out), 0))
        return out

    def get_forcing_device(self, var: int, step0: int, n: int, dev_ptr: int):
        """[n][cells] forcing rows into device memory (e.g. a torch tensor's data_ptr())."""
        self._chk(self._L.shyft_hip_get_forcing(self.h, var, step0, n, C.c_void_p(dev_ptr), 1))

    def interpolate(self, var: int, src_xyz: np.ndarray, src_values: np.ndarray, step0: int, idw_param):
        """IDW of one forcing variable from sources (src_values [n][S] on the model axis)."""
        xyz = np.ascontiguousarray(src_xyz, dtype=np.float64).reshape(-1, 3)
        v = np.ascontiguousarray(src_values, dtype=np.float64).reshape(-1, xyz.shape[0])
        p = np.ascontiguousarray(idw_param, dtype=np.float64)
        assert p.size == 7
        self._chk(self._L.shyft_hip_interpolate(self.h, var, xyz.shape[0], _ptr(xyz), _ptr(v), step0, v.shape[0],
                                                _ptr(p)))

    def interpolation_path(self, var: int) -> str:
        """The gather the last interpolate of `var` ran: "wave", "tile", "copy" or "none"."""
        k = int(self._L.shyft_hip_interpolation_path(self.h, int(var)))
        if k < 0:
            raise ValueError(f"interpolation_path: invalid variable {var}")
        return ("none", "tile", "wave", "copy")[k]

    def interpolate_btk(self, src_xyz: np.ndarray, src_values: np.ndarray, step0: int, btk_param,
                        prior_gradient=None):
        """Bayesian temperature kriging into the temperature forcing (src_values [n][S] on the model axis).
        btk_param: gradient_sd (C/m), sill, nugget, range, zscale; prior_gradient [n] or None (day-of-year prior)."""
        xyz = np.ascontiguousarray(src_xyz, dtype=np.float64).reshape(-1, 3)
        v = np.ascontiguousarray(src_values, dtype=np.float64).reshape(-1, xyz.shape[0])
        p = np.ascontiguousarray(btk_param, dtype=np.float64)
        assert p.size == 5
        g = None if prior_gradient is None else np.ascontiguousarray(prior_gradient, dtype=np.float64)
        assert g is None or g.size == v.shape[0]
        self._chk(self._L.shyft_hip_interpolate_btk(self.h, xyz.shape[0], _ptr(xyz), _ptr(v), step0, v.shape[0],
                                                    _ptr(g), _ptr(p)))

    def synthetic_forcing(self, seed: int, step0: int, n: int, cell_offset: int = 0):
        self._chk(self._L.shyft_hip_synthetic_forcing(self.h, seed, cell_offset, step0, n))

    def prefetch_synthetic_forcing(self, seed: int, w0_next: int, cell_offset: int = 0, n_cus: int = 8):
        """Generate the next forcing window (rows w0_next .. w0_next + window) on a side stream of n_cus CUs."""
        self._chk(self._L.shyft_hip_prefetch_synthetic_forcing(self.h, seed, cell_offset, w0_next, n_cus))

    def swap_forcing_window(self, w0_next: int):
        self._chk(self._L.shyft_hip_swap_forcing_window(self.h, w0_next))

    def run_cells(self, use_ncore: int = 0, start_step: int = 0, n_steps: int = 0):
        self._chk(self._L.shyft_hip_run_cells(self.h, int(use_ncore), int(start_step), int(n_steps)))

    def run_cells_async(self, start_step: int, n_steps: int):
        self._chk(self._L.shyft_hip_run_cells_async(self.h, int(start_step), int(n_steps)))

    def synchronize(self):
        self._chk(self._L.shyft_hip_synchronize(self.h))

    def last_run_ms(self) -> float:
        return float(self._L.shyft_hip_last_run_ms(self.h))

    def last_interpolate_ms(self) -> float:
        """The last interpolate()'s gather kernel, ms (HIP events on the region's stream)."""
        return float(self._L.shyft_hip_last_interpolate_ms(self.h))

    def last_run_kernel_ms(self) -> list:
        """The last run's kernels separately (pt_gs_k: [snow kernel, flux kernel]; other stacks: [kernel])."""
        buf = (C.c_double * 4)()
        n = self._L.shyft_hip_last_run_kernel_ms(self.h, buf, 4)
        return [float(buf[k]) for k in range(n)]

    def shard_run_ms(self) -> list:
        """Kernel ms of every shard's last run_cells (one entry when unsharded)."""
        buf = (C.c_double * 256)()
        n = int(self._L.shyft_hip_shard_run_ms(self.h, buf, 256))
        return [float(buf[k]) for k in range(min(n, 256))]

    def get_series(self, series: int, step0: int, n: int) -> np.ndarray:
        out = np.empty((n, self.n), dtype=np.float64)
        self._chk(self._L.shyft_hip_get_series(self.h, series, step0, n, _ptr(out), 0))
        return out

    def get_series_device(self, series: int, step0: int, n: int, dev_ptr: int):
        """[n][cells] rows of a collected series into device memory (e.g. a torch tensor's data_ptr())."""
        self._chk(self._L.shyft_hip_get_series(self.h, series, step0, n, C.c_void_p(dev_ptr), 1))

    def get_state_series(self, field: int, step0: int, n: int) -> np.ndarray:
        out = np.empty((n, self.n), dtype=np.float64)
        self._chk(self._L.shyft_hip_get_state_series(self.h, field, step0, n, _ptr(out), 0))
        return out

    def sample_cells(self, series: int, cells, step0: int, n: int) -> np.ndarray:
        """[n][len(cells)] columns of a series (response id, SERIES_FORCING + v, SERIES_STATE + f) for the given
        cells over steps [step0, step0 + n) of the resident window (one device gather; per shard if sharded)."""
        c = np.ascontiguousarray(cells, dtype=np.int64)
        out = np.empty((n, c.size), dtype=np.float64)
        self._chk(self._L.shyft_hip_sample_cells(self.h, int(series), _ptr(c), c.size, int(step0), int(n), _ptr(out)))
        return out

    def set_test_knob(self, knob: int, value: int):
        """KNOB_PTGSK_INSTANCE (0 auto, 2, 4) / KNOB_BRENT_READ_DELAY (s_sleep(127) rounds); tests only."""
        self._chk(self._L.shyft_hip_set_test_knob(self.h, int(knob), int(value)))

    def statistics(self, series: int, ids=(), scope: int = SCOPE_CATCHMENT, weighted: bool = False, step0: int = 0,
                   n: int | None = None) -> np.ndarray:
        n = self.n_steps - step0 if n is None else n
        i = np.ascontiguousarray(list(ids), dtype=np.int64)
        out = np.empty(n, dtype=np.float64)
        self._chk(self._L.shyft_hip_statistics(self.h, series, _ptr(i) if i.size else None, i.size, scope,
                                               int(weighted), step0, n, _ptr(out)))
        return out

    def percentiles(self, series: int, pcts, ids=(), scope: int = SCOPE_CATCHMENT, step0: int = 0,
                    n: int | None = None) -> np.ndarray:
        """[len(pcts)][n] percentiles across the selected cells per step (shyft_hip_percentiles): 0..100 R7,
        STAT_AVERAGE, STAT_MIN_EXTREME / STAT_MAX_EXTREME; non-finite values are dropped."""
        n = self.n_steps - step0 if n is None else n
        i = np.ascontiguousarray(list(ids), dtype=np.int64)
        p = np.ascontiguousarray(list(pcts), dtype=np.int64)
        out = np.empty((p.size, n), dtype=np.float64)
        self._chk(self._L.shyft_hip_percentiles(self.h, int(series), _ptr(i) if i.size else None, i.size, int(scope),
                                                _ptr(p), p.size, int(step0), int(n), _ptr(out)))
        return out

    def catchment_percentiles(self, series: int, pcts, step0: int, n: int) -> np.ndarray:
        """[n_catchments][len(pcts)][n], catchments in catchment_ids() order (shyft_hip_catchment_percentiles)."""
        p = np.ascontiguousarray(list(pcts), dtype=np.int64)
        out = np.empty((self.number_of_catchments(), p.size, n), dtype=np.float64)
        self._chk(self._L.shyft_hip_catchment_percentiles(self.h, int(series), _ptr(p), p.size, int(step0), int(n),
                                                          _ptr(out), 0))
        return out

    def catchment_percentiles_device(self, series: int, pcts, step0: int, n: int, dev_ptr: int):
        p = np.ascontiguousarray(list(pcts), dtype=np.int64)
        self._chk(self._L.shyft_hip_catchment_percentiles(self.h, int(series), _ptr(p), p.size, int(step0), int(n),
                                                          C.c_void_p(dev_ptr), 1))

    def percentiles_path(self) -> str:
        """The path of the last percentile call: "none", "lds_sort" or "radix"."""
        return PERCENTILES_PATHS[int(self._L.shyft_hip_percentiles_path(self.h))]

    def last_percentiles_ms(self) -> float:
        """The last percentile call's kernels, ms (HIP events on the region's stream)."""
        return float(self._L.shyft_hip_last_percentiles_ms(self.h))

    def number_of_catchments(self) -> int:
        return int(self._L.shyft_hip_number_of_catchments(self.h))

    def catchment_ids(self) -> np.ndarray:
        c = np.empty(self.number_of_catchments(), dtype=np.int64)
        self._chk(self._L.shyft_hip_catchment_ids(self.h, _ptr(c)))
        return c

    def catchment_sums(self, series: int, step0: int, n: int) -> np.ndarray:
        out = np.empty((self.number_of_catchments(), n), dtype=np.float64)
        self._chk(self._L.shyft_hip_catchment_sums(self.h, series, step0, n, _ptr(out), 0))
        return out

    def catchment_sums_device(self, series: int, step0: int, n: int, dev_ptr: int):
        self._chk(self._L.shyft_hip_catchment_sums(self.h, series, step0, n, C.c_void_p(dev_ptr), 1))

    # routing (routing.h:239-421): cells sharing (river, UHG) are one group
    def set_routing_groups(self, group_of_cell, n_groups: int):
        g = np.ascontiguousarray(group_of_cell, dtype=np.int32)
        assert g.size == self.n
        self._chk(self._L.shyft_hip_set_routing_groups(self.h, _ptr(g), int(n_groups)))
        self.n_route_groups = int(n_groups)

    def routing_group_sums(self, step0: int, n: int) -> np.ndarray:
        out = np.empty((self.n_route_groups, n), dtype=np.float64)
        self._chk(self._L.shyft_hip_routing_group_sums(self.h, step0, n, _ptr(out), 0))
        return out

    def routing_group_sums_device(self, step0: int, n: int, dev_ptr: int):
        self._chk(self._L.shyft_hip_routing_group_sums(self.h, step0, n, C.c_void_p(dev_ptr), 1))

    # parameter ensembles (model_calibration.h:830-899): n_members parameter vectors in one launch
    def ensemble_run(self, params: np.ndarray, start_step: int = 0, n_steps: int = 0,
                     collect: int = COLLECT_DISCHARGE):
        p = np.ascontiguousarray(params, dtype=np.float64)
        assert p.ndim == 2
        self._chk(self._L.shyft_hip_ensemble_run(self.h, _ptr(p), p.shape[0], p.shape[1], start_step, n_steps,
                                                 collect))
        self.ens_members = p.shape[0]

    def ensemble_sums(self, series: int, step0: int, n: int, area_weighted: bool = False) -> np.ndarray:
        """[n_members][n_catchments][n] sums of `series` over each member's calculated cells per catchment."""
        out = np.empty((self.ens_members, self.number_of_catchments(), n), dtype=np.float64)
        self._chk(self._L.shyft_hip_ensemble_sums(self.h, series, int(area_weighted), step0, n, _ptr(out), 0))
        return out

    def ensemble_last_ms(self) -> float:
        return float(self._L.shyft_hip_ensemble_last_ms(self.h))

    def ensemble_group_sums(self, group_of, group_row, step0: int, n: int, dev_ptr=None):
        """Routing-group discharge sums of the last ensemble run (shyft_hip_ensemble_group_sums): group_of
        [n_members][n_cells] (-1 = not part of this evaluation), group_row [n_members + 1]. Returns
        [group_row[-1]][n], or writes it to dev_ptr."""
        g = np.ascontiguousarray(group_of, dtype=np.int32)
        row = np.ascontiguousarray(group_row, dtype=np.int64)
        assert g.ndim == 2 and g.shape[1] == self.n and row.shape == (g.shape[0] + 1,)
        if dev_ptr is not None:
            self._chk(self._L.shyft_hip_ensemble_group_sums(self.h, g.shape[0], _ptr(g), _ptr(row), step0, n,
                                                            C.c_void_p(dev_ptr), 1))
            return None
        out = np.empty((max(int(row[-1]), 0), n), dtype=np.float64)
        self._chk(self._L.shyft_hip_ensemble_group_sums(self.h, g.shape[0], _ptr(g), _ptr(row), step0, n, _ptr(out), 0))
        return out


def route(group_sums, group_uhgs, group_river, river_uhgs, river_downstream, device: int = -1, sums_dev_ptr=None,
          T: int | None = None):
    """River network evaluation on the device (shyft_hip_route). group_sums [G][T] (numpy) or sums_dev_ptr (+T);
    group_uhgs / river_uhgs: lists of UHG weight vectors; group_river[G] and river_downstream[R] are river
    indices (ascending river id), -1 = no downstream. Returns (local, upstream, output), each [R][T]."""
    L = lib()
    G, R = len(group_uhgs), len(river_uhgs)
    max_len = max([1] + [len(w) for w in group_uhgs] + [len(w) for w in river_uhgs])
    gw = np.zeros((G, max_len))
    for k, w in enumerate(group_uhgs):
        gw[k, :len(w)] = w
    rw = np.zeros((R, max_len))
    for k, w in enumerate(river_uhgs):
        rw[k, :len(w)] = w
    glen = np.array([len(w) for w in group_uhgs], dtype=np.int32)
    rlen = np.array([len(w) for w in river_uhgs], dtype=np.int32)
    gr = np.ascontiguousarray(group_river, dtype=np.int32)
    rd = np.ascontiguousarray(river_downstream, dtype=np.int32)
    if sums_dev_ptr is None:
        s = np.ascontiguousarray(group_sums, dtype=np.float64)
        T = s.shape[1]
        src, on_dev = _ptr(s), 0
    else:
        src, on_dev = C.c_void_p(sums_dev_ptr), 1
    out = [np.empty((R, T)) for _ in range(3)]
    check(L.shyft_hip_route(device, G, T, src, on_dev, _ptr(gw), _ptr(glen), _ptr(gr), R, _ptr(rw), _ptr(rlen),
                            _ptr(rd), max_len, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), 0), None)
    return tuple(out)


def route_members(group_row, group_sums, group_uhgs, group_river, river_uhgs, river_downstream, device: int = -1,
                  host: bool = False, sums_dev_ptr=None, T: int | None = None, max_len: int | None = None):
    """River network evaluation for members with their own routing groups (shyft_hip_route_members; host=True: its
    _host twin, the literal loops). Member m owns the global group rows [group_row[m], group_row[m+1]) of group_sums
    [G][T] (numpy, or sums_dev_ptr + T on the device), group_uhgs and group_river; the rivers are shared. Returns
    (local, upstream, output), each [n_members][R][T]."""
    L = lib()
    row = np.ascontiguousarray(group_row, dtype=np.int64)
    P, G, R = row.size - 1, len(group_uhgs), len(river_uhgs)
    width = max([1] + [len(w) for w in group_uhgs] + [len(w) for w in river_uhgs])
    max_len = width if max_len is None else int(max_len)  # a smaller max_len than the tables' width: a refusal test
    gw = np.zeros((G, width))
    for k, w in enumerate(group_uhgs):
        gw[k, :len(w)] = w
    rw = np.zeros((R, width))
    for k, w in enumerate(river_uhgs):
        rw[k, :len(w)] = w
    glen = np.array([len(w) for w in group_uhgs], dtype=np.int32)
    rlen = np.array([len(w) for w in river_uhgs], dtype=np.int32)
    gr = np.ascontiguousarray(group_river, dtype=np.int32)
    rd = np.ascontiguousarray(river_downstream, dtype=np.int32)
    if sums_dev_ptr is None:
        s = np.ascontiguousarray(group_sums, dtype=np.float64)
        assert s.ndim == 2 and s.shape[0] == G
        T = s.shape[1]
        src, on_dev = _ptr(s), 0
    else:
        assert not host
        src, on_dev = C.c_void_p(sums_dev_ptr), 1
    out = [np.zeros((P, R, T)) for _ in range(3)]
    if host:
        check(L.shyft_hip_route_members_host(P, _ptr(row), T, src, _ptr(gw), _ptr(glen), _ptr(gr), R, _ptr(rw),
                                             _ptr(rlen), _ptr(rd), max_len, _ptr(out[0]), _ptr(out[1]), _ptr(out[2])),
              None)
    else:
        check(L.shyft_hip_route_members(device, P, _ptr(row), T, src, on_dev, _ptr(gw), _ptr(glen), _ptr(gr), R,
                                        _ptr(rw), _ptr(rlen), _ptr(rd), max_len, _ptr(out[0]), _ptr(out[1]),
                                        _ptr(out[2]), 0), None)
    return tuple(out)


def route_members_last_ms(device: int = -1) -> float:
    return float(lib().shyft_hip_route_members_last_ms(device))


def btk(src_xyz, src_values, prior_gradient, btk_param, dst_xyz, device: int = -1, block_steps: int = 0) -> np.ndarray:
    """Stateless Bayesian temperature kriging on the device (shyft_hip_btk): src_values [n][S] on the model axis,
    prior_gradient [n], btk_param (gradient_sd C/m, sill, nugget, range, zscale), dst_xyz [D][3] -> [n][D].
    block_steps caps the steps of one valid-source pattern per device product (0 = default; a test aid)."""
    L = lib()
    xyz = np.ascontiguousarray(src_xyz, dtype=np.float64).reshape(-1, 3)
    v = np.ascontiguousarray(src_values, dtype=np.float64).reshape(-1, xyz.shape[0])
    g = np.ascontiguousarray(prior_gradient, dtype=np.float64).reshape(v.shape[0])
    p = np.ascontiguousarray(btk_param, dtype=np.float64).reshape(5)
    d = np.ascontiguousarray(dst_xyz, dtype=np.float64).reshape(-1, 3)
    out = np.empty((v.shape[0], d.shape[0]))
    check(L.shyft_hip_btk_blocked(device, xyz.shape[0], _ptr(xyz), _ptr(v), v.shape[0], _ptr(g), _ptr(p), d.shape[0],
                                  _ptr(d), _ptr(out), int(block_steps)), None)
    return out


def percentiles_host(rows, pcts) -> np.ndarray:
    """The host restatement of the percentile kernels (shyft_hip_percentiles_host, no device call):
    rows [n_steps][n_samples] -> [len(pcts)][n_steps]."""
    r = np.ascontiguousarray(rows, dtype=np.float64)
    assert r.ndim == 2
    p = np.ascontiguousarray(list(pcts), dtype=np.int64)
    out = np.empty((p.size, r.shape[0]), dtype=np.float64)
    check(lib().shyft_hip_percentiles_host(_ptr(r), r.shape[0], r.shape[1], _ptr(p), p.size, _ptr(out)), None)
    return out


def ordinary_kriging(src_xyz, src_values, ok_param, dst_xyz, device: int = -1, host: bool = False,
                     dst_block: int = 0) -> np.ndarray:
    """Stateless ordinary kriging (shyft_hip_ordinary_kriging): src_values [n][S] on the model axis, ok_param
    (c, a, z_scale, cov_type 0 GAUSSIAN / 1 EXPONENTIAL), dst_xyz [D][3] -> [n][D]. host=True evaluates the same
    arithmetic on the host (shyft_hip_ordinary_kriging_host), which the device result is bit-identical to;
    dst_block sets the destinations per device pass (0 = default)."""
    L = lib()
    xyz = np.ascontiguousarray(src_xyz, dtype=np.float64).reshape(-1, 3)
    v = np.ascontiguousarray(src_values, dtype=np.float64).reshape(-1, xyz.shape[0]) if xyz.shape[0] else \
        np.empty((0, 0))
    p = np.append(np.asarray(ok_param, dtype=np.float64).reshape(4), float(dst_block))
    d = np.ascontiguousarray(dst_xyz, dtype=np.float64).reshape(-1, 3)
    out = np.empty((v.shape[0], d.shape[0]))
    if host:
        check(L.shyft_hip_ordinary_kriging_host(xyz.shape[0], _ptr(xyz), _ptr(v), v.shape[0], _ptr(p), d.shape[0],
                                                _ptr(d), _ptr(out)), None)
    else:
        check(L.shyft_hip_ordinary_kriging(device, xyz.shape[0], _ptr(xyz), _ptr(v), v.shape[0], _ptr(p), d.shape[0],
                                           _ptr(d), _ptr(out)), None)
    return out


KALMAN_FILTER, KALMAN_PREDICTOR = 0, 1


def kalman_initial_state(n: int, covariance_init: float, hourly_correlation: float, process_noise_init: float):
    """state::state's matrices (shyft_hip_kalman_initial_state; core/kalman.h:31-50): (P, W), both [n][n]."""
    n = int(n)
    P, W = np.empty((n, n)), np.empty((n, n))
    check(lib().shyft_hip_kalman_initial_state(n, float(covariance_init), float(hourly_correlation),
                                               float(process_noise_init), _ptr(P), _ptr(W)), None)
    return P, W


def kalman_run(bias, fold, w, v2, x, k, P, mode: int = KALMAN_PREDICTOR, running=None, device: int = -1,
               host: bool = False):
    """M independent Kalman bias filters over T steps in one call (shyft_hip_kalman_run; core/kalman.h:127-236).
    bias [T][M]; fold [T] the daily index of each step; w [n/2+1] the values of W by folded distance; v2 the squared
    measurement error; x [n][M], k [n][M], P [n*n][M] (or [n][n][M]) the start state. mode KALMAN_FILTER: a non-finite
    bias still grows P; KALMAN_PREDICTOR: it skips the step. running = (save_every, piece_begin [T+1], piece_ix,
    piece_seconds) also gives the running bias [T][M] (predictor mode). host=True evaluates the same arithmetic on
    the host (shyft_hip_kalman_run_host), which the device result is bit-identical to. Returns (x, k, P, out) as new
    arrays, P shaped [n][n][M], out None without `running`."""
    L = lib()
    x = np.array(x, dtype=np.float64, order="C", ndmin=2)
    n, M = x.shape
    k = np.array(k, dtype=np.float64, order="C").reshape(n, M)
    P = np.array(P, dtype=np.float64, order="C").reshape(n * n, M)
    b = np.ascontiguousarray(bias, dtype=np.float64).reshape(-1, M) if M else np.empty((len(fold), 0))
    T = b.shape[0]
    f = np.ascontiguousarray(fold, dtype=np.int32).reshape(-1)
    ww = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    if f.shape[0] != T:
        raise ValueError("kalman_run: fold and bias differ in the number of steps")
    if ww.shape[0] != n // 2 + 1:
        raise ValueError("kalman_run: w must have n/2+1 values")
    out, save_every, pb, pi, ps = None, 1, None, None, None
    if running is not None:
        save_every = int(running[0])
        pb = np.ascontiguousarray(running[1], dtype=np.int32).reshape(-1)
        pi = np.ascontiguousarray(running[2], dtype=np.int32).reshape(-1)
        ps = np.ascontiguousarray(running[3], dtype=np.float64).reshape(-1)
        if pb.shape[0] != T + 1 or pi.shape[0] != ps.shape[0] or (T and pb[-1] != pi.shape[0]):
            raise ValueError("kalman_run: the piece table does not match the steps")
        out = np.empty((T, M))
    tail = (float(v2), int(mode), _ptr(x), _ptr(k), _ptr(P), _ptr(out) if out is not None else None, save_every,
            _ptr(pb) if pb is not None else None, _ptr(pi) if pi is not None else None,
            _ptr(ps) if ps is not None else None)
    if host:
        check(L.shyft_hip_kalman_run_host(n, M, T, _ptr(b), _ptr(f), _ptr(ww), *tail), None)
    else:
        check(L.shyft_hip_kalman_run(device, n, M, T, _ptr(b), _ptr(f), _ptr(ww), *tail), None)
    return x, k, P.reshape(n, n, M), out


def kalman_last_ms(device: int = -1) -> float:
    """HIP-event milliseconds of the last kalman_run kernel on the device, copies excluded."""
    return float(lib().shyft_hip_kalman_last_ms(device))


QM_PRIOR, QM_QM, QM_BLEND = 0, 1, 2
QM_PATH_NONE, QM_PATH_WAVE, QM_PATH_GROUP = 0, 1, 2
QM_MAX_SERIES = 1024


def quantile_map(fc, w, pri, mode, interp_weight, interpolated: bool = False, device: int = -1,
                 host: bool = False) -> np.ndarray:
    """Quantile mapping of weighted forecasts onto scenarios, every (problem, step) in one call
    (shyft_hip_quantile_map; core/time_series_qm.h:34-351). fc [B][T][F] and pri [B][T][P] (or [T][F] and [T][P] for
    one problem) are the values averaged onto the axis, NaN where a series does not cover a step; w [F] the weight of
    each forecast, finite and > 0; mode [T] QM_PRIOR / QM_QM / QM_BLEND and interp_weight [T] what quantile_mapping
    derives from the times. interpolated selects compute_interp_weighted_quantiles. Equal values rank by ascending
    series index. host=True evaluates the same arithmetic on the host (shyft_hip_quantile_map_host), which the device
    result is bit-identical to, for any F and P; the device takes at most QM_MAX_SERIES of each. Returns out, shaped
    like pri."""
    L = lib()
    p = np.ascontiguousarray(pri, dtype=np.float64)
    f = np.ascontiguousarray(fc, dtype=np.float64)
    if p.ndim not in (2, 3) or f.ndim != p.ndim or f.shape[:-1] != p.shape[:-1]:
        raise ValueError("quantile_map: fc and pri must be [B][T][F] and [B][T][P], or [T][F] and [T][P]")
    B = p.shape[0] if p.ndim == 3 else 1
    T, P, F = p.shape[-2], p.shape[-1], f.shape[-1]
    ww = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    m = np.ascontiguousarray(mode, dtype=np.int32).reshape(-1)
    iw = np.ascontiguousarray(interp_weight, dtype=np.float64).reshape(-1)
    if ww.shape[0] != F:
        raise ValueError("quantile_map: w must have one weight per forecast")
    if m.shape[0] != T or iw.shape[0] != T:
        raise ValueError("quantile_map: mode and interp_weight must have one entry per step")
    out = np.empty(p.shape)
    args = (B, T, F, P, _ptr(f), _ptr(ww), _ptr(p), _ptr(m), _ptr(iw), int(bool(interpolated)), _ptr(out))
    if host:
        check(L.shyft_hip_quantile_map_host(*args), None)
    else:
        check(L.shyft_hip_quantile_map(device, *args), None)
    return out


def quantile_map_last_path(device: int = -1) -> int:
    """QM_PATH_WAVE or QM_PATH_GROUP: the launch shape of the last quantile_map kernel on the device."""
    return int(lib().shyft_hip_quantile_map_last_path(device))


def quantile_map_last_ms(device: int = -1) -> float:
    """HIP-event milliseconds of the last quantile_map kernel on the device, copies excluded."""
    return float(lib().shyft_hip_quantile_map_last_ms(device))


RESAMPLE_AVERAGE, RESAMPLE_INTEGRAL, RESAMPLE_ACCUMULATE = 0, 1, 2
RESAMPLE_PATH_AUTO, RESAMPLE_PATH_DIRECT, RESAMPLE_PATH_TILED = 0, 1, 2


def resample(series, time_axis, mode: int = RESAMPLE_AVERAGE, device: int = -1, host: bool = False) -> np.ndarray:
    """S point series onto a fixed_dt axis in one call (shyft_hip_resample; core/time_series.h:202-310, 2033-2120,
    core/time_series_dd.h:532-538, 672-679). series is a list of the api's `_PointTs`, time_axis a
    TimeAxisFixedDeltaT; mode RESAMPLE_AVERAGE (the true average, NaN from the series' end on), RESAMPLE_INTEGRAL
    (the integral of each interval) or RESAMPLE_ACCUMULATE (0.0, then the running integral from the axis' start, NaN
    from the series' end on). host=True evaluates the same values with the host's average_values / accumulate_value
    (shyft_hip_resample_host), which the device result is bit-identical to. Returns [T][S], series fastest."""
    from .api import _api
    row, t, v, t_end, fx, t0, dt, T = _api._resample_plan(list(series), time_axis)
    return resample_csr(row, t, v, t_end, fx, t0, dt, T, mode, device=device, host=host)


def _csr_series(what, row, t, v, t_end, fx):
    """S point series in the CSR form of the C ABI as contiguous arrays of its types, shapes checked"""
    row = np.ascontiguousarray(row, dtype=np.int64).reshape(-1)
    t = np.ascontiguousarray(t, dtype=np.int64).reshape(-1)
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    t_end = np.ascontiguousarray(t_end, dtype=np.int64).reshape(-1)
    fx = np.ascontiguousarray(fx, dtype=np.int32).reshape(-1)
    S = row.shape[0] - 1
    if S < 0 or t_end.shape[0] != S or fx.shape[0] != S:
        raise ValueError(f"{what}: row must have one entry more than t_end and fx")
    if t.shape[0] != v.shape[0] or (S and (row[0] != 0 or row[-1] != t.shape[0])):
        raise ValueError(f"{what}: row must run from 0 to the number of points")
    return S, row, t, v, t_end, fx


def resample_csr(row, t, v, t_end, fx, ta_t0: int, ta_dt: int, T: int, mode: int = RESAMPLE_AVERAGE, device: int = -1,
                 host: bool = False) -> np.ndarray:
    """resample on the arrays of the C ABI: row [S+1] point offsets, t [row[S]] int64 microseconds, v [row[S]],
    t_end [S] int64 microseconds, fx [S] (0 POINT_INSTANT_VALUE, 1 POINT_AVERAGE_VALUE), and the axis in
    microseconds. Returns [T][S]."""
    S, row, t, v, t_end, fx = _csr_series("resample", row, t, v, t_end, fx)
    out = np.empty((int(T), S), dtype=np.float64)
    fn = lib().shyft_hip_resample_host if host else lib().shyft_hip_resample
    check(fn(device, int(mode), S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), int(ta_t0), int(ta_dt), int(T),
             _ptr(out)), None)
    return out


def resample_last_ms(device: int = -1) -> float:
    """HIP-event milliseconds of the kernel or kernels of the last resample on the device, copies excluded."""
    return float(lib().shyft_hip_resample_last_ms(device))


def resample_calls(device: int = -1) -> int:
    """The number of resample calls that launched on the device so far."""
    return int(lib().shyft_hip_resample_calls(device))


def resample_set_path(path: int) -> None:
    """RESAMPLE_PATH_DIRECT or RESAMPLE_PATH_TILED forces the launch shape of resample for the process,
    RESAMPLE_PATH_AUTO gives the choice back (test and measurement aid)."""
    check(lib().shyft_hip_resample_set_path(int(path)), None)


def resample_last_path(device: int = -1) -> int:
    """RESAMPLE_PATH_DIRECT or RESAMPLE_PATH_TILED: the launch shape of the last resample on the device."""
    return int(lib().shyft_hip_resample_last_path(device))


# ---- percentiles of a vector of series on a fixed_dt axis (kernels/ts_percentiles.hip) ---------------------------------
TS_PERCENTILES_MAX_SERIES = 4096
TS_PERCENTILES_PATH_AUTO, TS_PERCENTILES_PATH_WAVE, TS_PERCENTILES_PATH_LDS = 0, 1, 2


def ts_percentiles_csr(row, t, v, t_end, fx, src, shift, ta_t0: int, ta_dt: int, T: int, pcts, device: int = -1,
                       host: bool = False) -> np.ndarray:
    """Percentiles across S views of R stored series on a fixed_dt axis in one fused device call
    (shyft_hip_ts_percentiles; calculate_percentiles, core/time_series_statistics.h:184-246). The stored series are in
    the CSR form of resample_csr; view s is series src[s] moved shift[s] microseconds later, so many views can share one
    stored series. Each entry of pcts is 0..100 (R7), STAT_AVERAGE, or STAT_MIN_EXTREME / STAT_MAX_EXTREME (the
    extremes of the points inside each interval). On the device S is at most TS_PERCENTILES_MAX_SERIES and len(pcts)
    at most PERCENTILES_MAX. host=True evaluates the same values with the host restatement
    (shyft_hip_ts_percentiles_host, no limits), which the device result is bit-identical to. Returns [len(pcts)][T]; a
    call without views gives NaN."""
    R, row, t, v, t_end, fx = _csr_series("ts_percentiles", row, t, v, t_end, fx)
    src = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
    shift = np.ascontiguousarray(shift, dtype=np.int64).reshape(-1)
    if src.shape[0] != shift.shape[0]:
        raise ValueError("ts_percentiles: src and shift must have one entry per view")
    p = np.ascontiguousarray(list(pcts), dtype=np.int64).reshape(-1)
    out = np.full((p.size, int(T)), np.nan, dtype=np.float64)
    fn = lib().shyft_hip_ts_percentiles_host if host else lib().shyft_hip_ts_percentiles
    check(fn(device, R, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), src.shape[0], _ptr(src), _ptr(shift),
             int(ta_t0), int(ta_dt), int(T), _ptr(p), p.size, _ptr(out)), None)
    return out


def ts_percentiles(series, time_axis, pcts, device: int = -1, host: bool = False) -> np.ndarray:
    """ts_percentiles_csr over a list of the api's `_PointTs`, each its own stored series, on a TimeAxisFixedDeltaT.
    Returns [len(pcts)][T]."""
    from .api import _api
    row, t, v, t_end, fx, t0, dt, T = _api._resample_plan(list(series), time_axis)
    S = len(t_end)
    return ts_percentiles_csr(row, t, v, t_end, fx, np.arange(S), np.zeros(S, np.int64), t0, dt, T, pcts, device=device,
                              host=host)


def ts_percentiles_last_ms(device: int = -1) -> float:
    """HIP-event milliseconds of the kernel of the last ts_percentiles on the device, copies excluded."""
    return float(lib().shyft_hip_ts_percentiles_last_ms(device))


def ts_percentiles_calls(device: int = -1) -> int:
    """The number of ts_percentiles calls that launched on the device so far."""
    return int(lib().shyft_hip_ts_percentiles_calls(device))


def ts_percentiles_set_path(path: int) -> None:
    """TS_PERCENTILES_PATH_WAVE or TS_PERCENTILES_PATH_LDS forces the launch shape of ts_percentiles for the process,
    TS_PERCENTILES_PATH_AUTO gives the choice back (test and measurement aid)."""
    check(lib().shyft_hip_ts_percentiles_set_path(int(path)), None)


def ts_percentiles_last_path(device: int = -1) -> int:
    """TS_PERCENTILES_PATH_WAVE or TS_PERCENTILES_PATH_LDS: the launch shape of the last ts_percentiles on the device."""
    return int(lib().shyft_hip_ts_percentiles_last_path(device))


# ---- observation preparation: rating curve, ice packing, recession, min-max fill (kernels/tsprep.hip) ------------------
ICE_DISALLOW_MISSING, ICE_ALLOW_INITIAL_MISSING, ICE_ALLOW_ANY_MISSING = 0, 1, 2


def _per_series(what, name, x, S, dtype):
    """one value for all series, or one per series"""
    a = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
    if a.shape[0] == 1 and S != 1:
        a = np.repeat(a, S)
    if a.shape[0] != S:
        raise ValueError(f"{what}: {name} must hold one value or one per series")
    return np.ascontiguousarray(a)


def ts_rating_curve_csr(row, t, v, t_end, fx, pack_row, curve_t, curve_row, seg, pack_of=0, device: int = -1,
                        host: bool = False) -> np.ndarray:
    """Water levels to flow through rating-curve parameter packs, one value per point in CSR order
    (shyft_hip_ts_rating_curve; rating_curve_parameters::flow, core/time_series.h:1493-1506). The S level series are in
    the CSR form of resample_csr. The packs are a three-level CSR: pack_row [P+1] -> curve_t [C] curve start times
    (int64 microseconds) -> curve_row [C+1] -> seg [G][4] = lower, a, b, c; pack_of names the pack of each series (one
    value for all, or [S]). host=True runs the host restatement, which the device is bit-identical to."""
    S, row, t, v, t_end, fx = _csr_series("ts_rating_curve", row, t, v, t_end, fx)
    pack_row = np.ascontiguousarray(pack_row, dtype=np.int64).reshape(-1)
    curve_t = np.ascontiguousarray(curve_t, dtype=np.int64).reshape(-1)
    curve_row = np.ascontiguousarray(curve_row, dtype=np.int64).reshape(-1)
    seg = np.ascontiguousarray(seg, dtype=np.float64).reshape(-1, 4)
    pack_of = _per_series("ts_rating_curve", "pack_of", pack_of, S, np.int64)
    P = pack_row.shape[0] - 1
    if P < 0 or (P and (pack_row[0] != 0 or pack_row[-1] != curve_t.shape[0])) or curve_row.shape[0] != curve_t.shape[0] + 1 \
            or curve_row[0] != 0 or curve_row[-1] != seg.shape[0]:
        raise ValueError("ts_rating_curve: pack_row, curve_t, curve_row and seg do not form a CSR")
    out = np.empty(t.shape[0], dtype=np.float64)
    fn = lib().shyft_hip_ts_rating_curve_host if host else lib().shyft_hip_ts_rating_curve
    check(fn(device, S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), P, _ptr(pack_row), _ptr(curve_t),
             _ptr(curve_row), _ptr(seg), _ptr(pack_of), _ptr(out)), None)
    return out


def ts_ice_packing_csr(row, t, v, t_end, fx, qrow, qt, window, threshold, policy=ICE_DISALLOW_MISSING, device: int = -1,
                       host: bool = False) -> np.ndarray:
    """The ice-packing indicator of S temperature series at query times of their own CSR (qrow [S+1], qt int64
    microseconds), one value per query (shyft_hip_ts_ice_packing; ice_packing_ts::detect_ice_packing,
    core/time_series.h:1808-1831): 1.0 when the average over [t - window, t) is below the threshold, 0.0 when not, NaN
    when the policy cannot tell. window (int64 microseconds), threshold and policy (ICE_*) are one value for all
    series or [S]. Pass qrow=row, qt=t for the series' own points."""
    S, row, t, v, t_end, fx = _csr_series("ts_ice_packing", row, t, v, t_end, fx)
    qrow = np.ascontiguousarray(qrow, dtype=np.int64).reshape(-1)
    qt = np.ascontiguousarray(qt, dtype=np.int64).reshape(-1)
    if qrow.shape[0] != S + 1 or (S and (qrow[0] != 0 or qrow[-1] != qt.shape[0])):
        raise ValueError("ts_ice_packing: qrow must run from 0 to the number of queries")
    window = _per_series("ts_ice_packing", "window", window, S, np.int64)
    threshold = _per_series("ts_ice_packing", "threshold", threshold, S, np.float64)
    policy = _per_series("ts_ice_packing", "policy", policy, S, np.int32)
    out = np.empty(qt.shape[0], dtype=np.float64)
    fn = lib().shyft_hip_ts_ice_packing_host if host else lib().shyft_hip_ts_ice_packing
    check(fn(device, S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), _ptr(qrow), _ptr(qt), _ptr(window),
             _ptr(threshold), _ptr(policy), _ptr(out)), None)
    return out


def ts_ice_packing_recession_csr(row, t, v, t_end, fx, ice, ice_start, ice_end, alpha, recession_minimum,
                                 device: int = -1, host: bool = False) -> np.ndarray:
    """S flow series with the recession curve wherever the indicator `ice` (one value per flow point, already sampled
    at the flow's points) says ice-packing, one value per point (shyft_hip_ts_ice_packing_recession;
    ice_packing_recession_ts::evaluate, core/time_series_dd.h:1323-1354). ice_start / ice_end [S] are the indicator's
    total period (the flow's must lie inside); alpha [1/s] and recession_minimum are one value for all or [S]."""
    S, row, t, v, t_end, fx = _csr_series("ts_ice_packing_recession", row, t, v, t_end, fx)
    ice = np.ascontiguousarray(ice, dtype=np.float64).reshape(-1)
    if ice.shape[0] != t.shape[0]:
        raise ValueError("ts_ice_packing_recession: ice must hold one value per flow point")
    ice_start = _per_series("ts_ice_packing_recession", "ice_start", ice_start, S, np.int64)
    ice_end = _per_series("ts_ice_packing_recession", "ice_end", ice_end, S, np.int64)
    alpha = _per_series("ts_ice_packing_recession", "alpha", alpha, S, np.float64)
    qmin = _per_series("ts_ice_packing_recession", "recession_minimum", recession_minimum, S, np.float64)
    out = np.empty(t.shape[0], dtype=np.float64)
    fn = lib().shyft_hip_ts_ice_packing_recession_host if host else lib().shyft_hip_ts_ice_packing_recession
    check(fn(device, S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), _ptr(ice), _ptr(ice_start), _ptr(ice_end),
             _ptr(alpha), _ptr(qmin), _ptr(out)), None)
    return out


def ts_min_max_fill_csr(row, t, v, t_end, fx, min_x, max_x, max_timespan, device: int = -1,
                        host: bool = False) -> np.ndarray:
    """S series with every value that is not finite or lies outside [min_x, max_x] (NaN = no limit) replaced by the
    line through its nearest valid neighbours, or NaN when they are missing or more than max_timespan (int64
    microseconds) apart, one value per point (shyft_hip_ts_min_max_fill; qac_ts::value,
    core/time_series_dd.cpp:1335-1376). The three parameters are one value for all series or [S]."""
    S, row, t, v, t_end, fx = _csr_series("ts_min_max_fill", row, t, v, t_end, fx)
    min_x = _per_series("ts_min_max_fill", "min_x", min_x, S, np.float64)
    max_x = _per_series("ts_min_max_fill", "max_x", max_x, S, np.float64)
    span = _per_series("ts_min_max_fill", "max_timespan", max_timespan, S, np.int64)
    out = np.empty(t.shape[0], dtype=np.float64)
    fn = lib().shyft_hip_ts_min_max_fill_host if host else lib().shyft_hip_ts_min_max_fill
    check(fn(device, S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), _ptr(min_x), _ptr(max_x), _ptr(span),
             _ptr(out)), None)
    return out


def tsprep_last_ms(device: int = -1) -> float:
    """HIP-event milliseconds of the kernels of the last ts_*_csr device call on the device, copies excluded."""
    return float(lib().shyft_hip_tsprep_last_ms(device))


def tsprep_calls(device: int = -1) -> int:
    """The number of ts_*_csr device calls that launched on the device so far."""
    return int(lib().shyft_hip_tsprep_calls(device))


# ---- point-wise filters: convolve_w, derivative, inside, decode (kernels/tsfilter.hip) -------------------------------
CONVOLVE_USE_FIRST, CONVOLVE_USE_ZERO, CONVOLVE_USE_NAN = 0, 1, 2
DERIVATIVE_DEFAULT, DERIVATIVE_FORWARD, DERIVATIVE_BACKWARD, DERIVATIVE_CENTER = 0, 1, 2, 3
TSFILTER_PATH_AUTO, TSFILTER_PATH_DIRECT, TSFILTER_PATH_TILED = 0, 1, 2


def ts_convolve_w_csr(row, t, v, t_end, fx, w_row, w, w_of=0, policy=CONVOLVE_USE_FIRST, device: int = -1,
                      host: bool = False) -> np.ndarray:
    """S series convolved with weight profiles, one value per point in CSR order (shyft_hip_ts_convolve_w;
    convolve_w_ts::value, core/time_series.h:966-975): out[i] = sum_j w[j] * x[i-j], the taps added in ascending j,
    with the policy's stand-in before the first point (CONVOLVE_USE_FIRST x[0], _USE_ZERO 0.0, _USE_NAN NaN). The
    profiles are a CSR, w_row [W+1] offsets into w; w_of names the profile and policy the policy of each series (one
    value for all, or [S]). host=True runs the host restatement, which the device is bit-identical to."""
    S, row, t, v, t_end, fx = _csr_series("ts_convolve_w", row, t, v, t_end, fx)
    w_row = np.ascontiguousarray(w_row, dtype=np.int64).reshape(-1)
    w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    W = w_row.shape[0] - 1
    if W < 0 or w_row[-1] != w.shape[0]:
        raise ValueError("ts_convolve_w: w_row must end at the number of weights")
    w_of = _per_series("ts_convolve_w", "w_of", w_of, S, np.int64)
    policy = _per_series("ts_convolve_w", "policy", policy, S, np.int32)
    out = np.empty(t.shape[0], dtype=np.float64)
    fn = lib().shyft_hip_ts_convolve_w_host if host else lib().shyft_hip_ts_convolve_w
    check(fn(device, S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), W, _ptr(w_row), _ptr(w), _ptr(w_of),
             _ptr(policy), _ptr(out)), None)
    return out


def ts_derivative_csr(row, t, v, t_end, fx, fixed_dt=0, method=DERIVATIVE_DEFAULT, device: int = -1,
                      host: bool = False) -> np.ndarray:
    """The derivative of S series, one value per point (shyft_hip_ts_derivative; derivative_ts::values,
    core/time_series_dd.cpp:311-463): the slope to the next point for a POINT_INSTANT_VALUE series (NaN at the last),
    the DERIVATIVE_* method's difference for a POINT_AVERAGE_VALUE series. fixed_dt (int64 microseconds) > 0 names
    the series' even spacing and takes the reference's fixed-step branch, 0 its variable branch; fixed_dt and method
    are one value for all series or [S]. The result is POINT_AVERAGE_VALUE."""
    S, row, t, v, t_end, fx = _csr_series("ts_derivative", row, t, v, t_end, fx)
    fixed_dt = _per_series("ts_derivative", "fixed_dt", fixed_dt, S, np.int64)
    method = _per_series("ts_derivative", "method", method, S, np.int32)
    out = np.empty(t.shape[0], dtype=np.float64)
    fn = lib().shyft_hip_ts_derivative_host if host else lib().shyft_hip_ts_derivative
    check(fn(device, S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), _ptr(fixed_dt), _ptr(method), _ptr(out)), None)
    return out


def ts_inside_csr(row, t, v, t_end, fx, min_x, max_x, nan_x=float("nan"), x_inside=1.0, x_outside=0.0,
                  device: int = -1, host: bool = False) -> np.ndarray:
    """S series mapped to x_inside where the value lies in [min_x, max_x) (NaN = no limit), x_outside where not and
    nan_x where it is not finite, one value per point (shyft_hip_ts_inside; inside_parameter::inside_value,
    core/time_series_dd.h:1546-1554). The five parameters are one value for all series or [S]."""
    S, row, t, v, t_end, fx = _csr_series("ts_inside", row, t, v, t_end, fx)
    p = [_per_series("ts_inside", name, x, S, np.float64)
         for name, x in (("min_x", min_x), ("max_x", max_x), ("nan_x", nan_x), ("x_inside", x_inside),
                         ("x_outside", x_outside))]
    out = np.empty(t.shape[0], dtype=np.float64)
    fn = lib().shyft_hip_ts_inside_host if host else lib().shyft_hip_ts_inside
    check(fn(device, S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), *(_ptr(x) for x in p), _ptr(out)), None)
    return out


def ts_decode_csr(row, t, v, t_end, fx, start_bit, n_bits, device: int = -1, host: bool = False) -> np.ndarray:
    """n_bits bits from start_bit of the values of S series taken as unsigned integers, one value per point; NaN for a
    value that is not finite, negative or above 2^52 (shyft_hip_ts_decode; bit_decoder::decode,
    core/time_series_dd.h:1650-1655). start_bit and n_bits are one value for all series or [S]."""
    S, row, t, v, t_end, fx = _csr_series("ts_decode", row, t, v, t_end, fx)
    start_bit = _per_series("ts_decode", "start_bit", start_bit, S, np.int32)
    n_bits = _per_series("ts_decode", "n_bits", n_bits, S, np.int32)
    out = np.empty(t.shape[0], dtype=np.float64)
    fn = lib().shyft_hip_ts_decode_host if host else lib().shyft_hip_ts_decode
    check(fn(device, S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), _ptr(start_bit), _ptr(n_bits), _ptr(out)), None)
    return out


def tsfilter_last_ms(device: int = -1) -> float:
    """HIP-event milliseconds of the kernel of the last ts_convolve_w_csr, ts_derivative_csr, ts_inside_csr or
    ts_decode_csr device call on the device, copies excluded."""
    return float(lib().shyft_hip_tsfilter_last_ms(device))


def tsfilter_calls(device: int = -1) -> int:
    """The number of those device calls that launched on the device so far."""
    return int(lib().shyft_hip_tsfilter_calls(device))


def tsfilter_set_path(path: int) -> None:
    """TSFILTER_PATH_DIRECT or TSFILTER_PATH_TILED forces the launch shape of ts_convolve_w_csr for the process,
    TSFILTER_PATH_AUTO gives the choice back (test and measurement aid)."""
    check(lib().shyft_hip_tsfilter_set_path(int(path)), None)


def tsfilter_last_path(device: int = -1) -> int:
    """TSFILTER_PATH_DIRECT or TSFILTER_PATH_TILED: the launch shape of the last ts_convolve_w_csr on the device."""
    return int(lib().shyft_hip_tsfilter_last_path(device))


# ---- forecast skill by lead time (kernels/forecast.hip) ---------------------------------------------------------------
def forecast_skill_csr(row, t, v, t_end, fx, fc_row, fc_ix, obs_ix, t0_offset, dt, n, device: int = -1,
                       host: bool = False, slices: bool = False):
    """The Nash-Sutcliffe score of P problems in one device call (shyft_hip_forecast_skill; nash_sutcliffe of
    core/time_series_merge.h:123-144). The S series, forecasts and observations together, are in the CSR form of
    resample_csr. Problem p takes the forecasts fc_ix[fc_row[p]:fc_row[p+1]] (indexes into the series) against the
    observation obs_ix[p] (-1: none) over n[p] slices of dt[p] that start t0_offset[p] after each forecast's first
    point (int64 microseconds; one value for all problems, or [P]). Returns ns [P]; with slices=True (ns, sim, obs),
    the slice averages of every forecast and of the observation, [sum of F_p * n[p]] in problem, forecast, slice
    order. host=True runs the host restatement, which the device is bit-identical to."""
    S, row, t, v, t_end, fx = _csr_series("forecast_skill", row, t, v, t_end, fx)
    fc_row = np.ascontiguousarray(fc_row, dtype=np.int64).reshape(-1)
    fc_ix = np.ascontiguousarray(fc_ix, dtype=np.int64).reshape(-1)
    obs_ix = np.ascontiguousarray(obs_ix, dtype=np.int64).reshape(-1)
    P = fc_row.shape[0] - 1
    if P < 0 or obs_ix.shape[0] != P:
        raise ValueError("forecast_skill: fc_row must have one entry more than obs_ix")
    if P and (fc_row[0] != 0 or fc_row[-1] != fc_ix.shape[0]):
        raise ValueError("forecast_skill: fc_row must run from 0 to the number of forecast indexes")
    t0_offset = _per_series("forecast_skill", "t0_offset", t0_offset, P, np.int64)
    dt = _per_series("forecast_skill", "dt", dt, P, np.int64)
    n = _per_series("forecast_skill", "n", n, P, np.int64)
    ns = np.empty(P, dtype=np.float64)
    sim = obs = None
    if slices:
        J = int(np.sum(np.diff(fc_row) * np.maximum(n, 0), dtype=np.int64)) if P else 0
        sim, obs = np.full(J, np.nan), np.full(J, np.nan)
    fn = lib().shyft_hip_forecast_skill_host if host else lib().shyft_hip_forecast_skill
    check(fn(device, S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), P, _ptr(fc_row), _ptr(fc_ix), _ptr(obs_ix),
             _ptr(t0_offset), _ptr(dt), _ptr(n), _ptr(ns), _ptr(sim), _ptr(obs)), None)
    return (ns, sim, obs) if slices else ns


def forecast_skill_last_ms(device: int = -1) -> float:
    """HIP-event milliseconds of the kernel of the last forecast_skill_csr device call on the device, copies excluded."""
    return float(lib().shyft_hip_forecast_skill_last_ms(device))


def forecast_skill_calls(device: int = -1) -> int:
    """The number of forecast_skill_csr device calls that launched on the device so far."""
    return int(lib().shyft_hip_forecast_skill_calls(device))


# ---- time-series arithmetic (kernels/ts_expr.hip) ---------------------------------------------------------------------
def ts_expr_csr(row, t, v, t_end, fx, prog_row, prog, consts, periods, orow, ot, device: int = -1,
                host: bool = False) -> np.ndarray:
    """E expressions over S terminal series, every point of every expression in one device call (shyft_hip_ts_expr;
    the reference's lazy apoint_ts arithmetic, core/time_series_dd.cpp:70-129, 197-224, 835-920). The terminals are in
    the CSR form of resample_csr. Expression e runs the postfix program prog[prog_row[e]:prog_row[e+1]] (int32 words,
    csrc/host/ts_expr.hpp; api._api._ts_expr_plan makes them from trees) at its output points orow[e]:orow[e+1], whose
    times (int64 microseconds) are ot; consts and periods [n][2] are the tables the programs index. Returns
    [orow[E]]. The device entry refuses a stack deeper than 8 values or a program longer than 64 words; host=True runs
    the host interpreter, which has no such limit and which the device is bit-identical to."""
    S, row, t, v, t_end, fx = _csr_series("ts_expr", row, t, v, t_end, fx)
    prog_row = np.ascontiguousarray(prog_row, dtype=np.int64).reshape(-1)
    prog = np.ascontiguousarray(prog, dtype=np.int32).reshape(-1)
    consts = np.ascontiguousarray(consts, dtype=np.float64).reshape(-1)
    periods = np.ascontiguousarray(periods, dtype=np.int64).reshape(-1, 2)
    orow = np.ascontiguousarray(orow, dtype=np.int64).reshape(-1)
    ot = np.ascontiguousarray(ot, dtype=np.int64).reshape(-1)
    E = prog_row.shape[0] - 1
    if E < 0 or orow.shape[0] != E + 1:
        raise ValueError("ts_expr: prog_row and orow must have one entry more than there are expressions")
    if E and (prog_row[-1] != prog.shape[0] or orow[-1] != ot.shape[0]):
        raise ValueError("ts_expr: prog_row must end at the number of words and orow at the number of output points")
    out = np.empty(ot.shape[0] if E else 0, dtype=np.float64)
    fn = lib().shyft_hip_ts_expr_host if host else lib().shyft_hip_ts_expr
    check(fn(device, S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), E, _ptr(prog_row), _ptr(prog),
             consts.shape[0], _ptr(consts), periods.shape[0], _ptr(periods), _ptr(orow), _ptr(ot), _ptr(out)), None)
    return out


def ts_expr_last_ms(device: int = -1) -> float:
    """HIP-event milliseconds of the kernel of the last ts_expr_csr device call on the device, copies excluded."""
    return float(lib().shyft_hip_ts_expr_last_ms(device))


def ts_expr_calls(device: int = -1) -> int:
    """The number of ts_expr_csr device calls that launched on the device so far."""
    return int(lib().shyft_hip_ts_expr_calls(device))


# ---- KRLS interpolation (kernels/krls.hip) ------------------------------------------------------------------------------
KRLS_LDS_CAPACITY, KRLS_MAX_DICT = 99, 1024  # SHYFT_HIP_KRLS_LDS_CAPACITY, SHYFT_HIP_KRLS_MAX_DICT
KRLS_LDS_SMALL_CAPACITY = 31                 # SHYFT_HIP_KRLS_LDS_SMALL_CAPACITY: the LDS storage tried first
KRLS_PATH_LDS, KRLS_PATH_WORKSPACE, KRLS_PATH_HOST = 1, 2, 3
KRLS_DEFAULT_SIZE = 1000000


def krls_train_csr(row, t, v, t_end, fx, dt, gamma=1e-3, tolerance=0.01, size=KRLS_DEFAULT_SIZE, offset=0, count=-1,
                   stride=1, iterations=1, mse_tol=0.001, state=None, device: int = -1, host: bool = False):
    """One KRLS predictor trained per series, all in one device call (shyft_hip_krls_train_csr;
    krls_rbf_predictor::train, core/predictions.h:139-181, restated in csrc/host/krls.hpp). The S series are in the CSR
    form of resample_csr. dt (int64 microseconds), gamma, tolerance, size (the most dictionary entries), offset, count
    (< 0: to the end), stride, iterations and mse_tol are one value for all series or [S]. state = (d_row, d, alpha,
    Kinv, P), as this function returns it, trains trained predictors further; None starts empty ones.
    Returns (d_row, d, alpha, Kinv, P, mse, path): d_row [S+1] offsets of the dictionaries d (sample positions) and
    weights alpha, Kinv and P lists of S dense [m][m] arrays, mse [S] as train returns it, and path [S]: KRLS_PATH_LDS
    (both matrices in LDS, at most KRLS_LDS_CAPACITY entries), KRLS_PATH_WORKSPACE (device memory, at most
    KRLS_MAX_DICT) or KRLS_PATH_HOST (a longer dictionary, or one that reached `size` and had an entry removed).
    host=True trains every series with the host restatement, which the device is bit-identical to."""
    S, row, t, v, t_end, fx = _csr_series("krls_train", row, t, v, t_end, fx)
    dt = _per_series("krls_train", "dt", dt, S, np.int64)
    gamma = _per_series("krls_train", "gamma", gamma, S, np.float64)
    tolerance = _per_series("krls_train", "tolerance", tolerance, S, np.float64)
    size = _per_series("krls_train", "size", size, S, np.int64)
    offset = _per_series("krls_train", "offset", offset, S, np.int64)
    count = _per_series("krls_train", "count", count, S, np.int64)
    stride = _per_series("krls_train", "stride", stride, S, np.int64)
    iterations = _per_series("krls_train", "iterations", iterations, S, np.int64)
    mse_tol = _per_series("krls_train", "mse_tol", mse_tol, S, np.float64)
    s_row = s_d = s_alpha = s_K = s_P = None
    if state is not None:
        s_row = np.ascontiguousarray(state[0], dtype=np.int64).reshape(-1)
        s_d = np.ascontiguousarray(state[1], dtype=np.float64).reshape(-1)
        s_alpha = np.ascontiguousarray(state[2], dtype=np.float64).reshape(-1)
        if s_row.shape[0] != S + 1 or s_row[0] != 0 or s_row[-1] != s_d.shape[0] or s_alpha.shape[0] != s_d.shape[0] \
                or len(state[3]) != S or len(state[4]) != S:
            raise ValueError("krls_train: the starting state must hold one predictor per series")
        mats = []
        for M in (state[3], state[4]):
            dense = [np.ascontiguousarray(x, dtype=np.float64) for x in M]
            if any(x.shape != (s_row[k + 1] - s_row[k],) * 2 for k, x in enumerate(dense)):
                raise ValueError("krls_train: a starting matrix is not [m][m]")
            mats.append(np.concatenate([x.reshape(-1) for x in dense]) if dense else np.empty(0))
        s_K, s_P = mats
    res = C.c_void_p()
    fn = lib().shyft_hip_krls_train_csr_host if host else lib().shyft_hip_krls_train_csr
    check(fn(device, S, _ptr(row), _ptr(t), _ptr(v), _ptr(t_end), _ptr(fx), _ptr(dt), _ptr(gamma), _ptr(tolerance),
             _ptr(size), _ptr(offset), _ptr(count), _ptr(stride), _ptr(iterations), _ptr(mse_tol), _ptr(s_row), _ptr(s_d),
             _ptr(s_alpha), _ptr(s_K), _ptr(s_P), C.byref(res)), None)
    try:
        d_row = np.zeros(S + 1, dtype=np.int64)
        check(lib().shyft_hip_krls_result_sizes(res, S, _ptr(d_row)), None)
        m = np.diff(d_row)
        d = np.empty(int(d_row[-1]), dtype=np.float64)
        alpha = np.empty_like(d)
        K = np.empty(int((m * m).sum()), dtype=np.float64)
        P = np.empty_like(K)
        mse = np.empty(S, dtype=np.float64)
        path = np.empty(S, dtype=np.int32)
        check(lib().shyft_hip_krls_result_fetch(res, S, _ptr(d), _ptr(alpha), _ptr(K), _ptr(P), _ptr(mse), _ptr(path)), None)
    finally:
        lib().shyft_hip_krls_result_free(res)
    m_off = np.concatenate([[0], np.cumsum(m * m)]).astype(np.int64)
    Ks = [K[m_off[k]:m_off[k + 1]].reshape(m[k], m[k]) for k in range(S)]
    Ps = [P[m_off[k]:m_off[k + 1]].reshape(m[k], m[k]) for k in range(S)]
    return d_row, d, alpha, Ks, Ps, mse, path


def krls_predict(d_row, d, alpha, dt, gamma, q_row, q_t, q_v=None, device: int = -1, host: bool = False) -> np.ndarray:
    """S trained predictors evaluated at output times of their own CSR (q_row [S+1], q_t int64 microseconds), one value
    per output time (shyft_hip_krls_predict; krls_rbf_predictor::predict_vec, core/predictions.h:193-207):
    sum_i alpha_i * k(x, d_i) in index order, 0.0 for an empty dictionary. With q_v, one value per output time, the
    result is the residual q_v - f(x), NaN where q_v is NaN (the terms of predictor_mse and mse_ts). dt and gamma are
    one value for all predictors or [S]. host=True runs the host restatement, which the device is bit-identical to."""
    d_row = np.ascontiguousarray(d_row, dtype=np.int64).reshape(-1)
    d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1)
    alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
    q_row = np.ascontiguousarray(q_row, dtype=np.int64).reshape(-1)
    q_t = np.ascontiguousarray(q_t, dtype=np.int64).reshape(-1)
    S = d_row.shape[0] - 1
    if S < 0 or q_row.shape[0] != S + 1 or d.shape[0] != alpha.shape[0]:
        raise ValueError("krls_predict: d_row and q_row must have one entry more than there are predictors")
    if S and (d_row[0] != 0 or d_row[-1] != d.shape[0] or q_row[0] != 0 or q_row[-1] != q_t.shape[0]):
        raise ValueError("krls_predict: d_row must run over the dictionaries and q_row over the output times")
    if q_v is not None:
        q_v = np.ascontiguousarray(q_v, dtype=np.float64).reshape(-1)
        if q_v.shape[0] != q_t.shape[0]:
            raise ValueError("krls_predict: q_v must hold one value per output time")
    dt = _per_series("krls_predict", "dt", dt, S, np.int64)
    gamma = _per_series("krls_predict", "gamma", gamma, S, np.float64)
    out = np.empty(q_t.shape[0] if S else 0, dtype=np.float64)
    fn = lib().shyft_hip_krls_predict_host if host else lib().shyft_hip_krls_predict
    check(fn(device, S, _ptr(d_row), _ptr(d), _ptr(alpha), _ptr(dt), _ptr(gamma), _ptr(q_row), _ptr(q_t), _ptr(q_v),
             _ptr(out)), None)
    return out


def krls_last_ms(device: int = -1) -> float:
    """HIP-event milliseconds of the kernels of the last krls_train_csr (all its launches) or krls_predict device call
    on the device, copies excluded."""
    return float(lib().shyft_hip_krls_last_ms(device))


def krls_set_path(path: int) -> None:
    """KRLS_PATH_WORKSPACE makes krls_train_csr skip the LDS storage for the process, 0 gives the choice back
    (measurement aid)."""
    check(lib().shyft_hip_krls_set_path(int(path)), None)
