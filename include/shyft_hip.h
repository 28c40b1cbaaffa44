/* shyft_hip.h — C ABI of the MI355X (gfx950) region engine.
 *
 * This is the drop-in boundary for Shyft's distributed-cell hot path:
 * region_model::run_interpolation / run_cells (core/region_model.h:546-597)
 * and the catchment statistics that consume run_cells' output
 * (core/cell_model.h:228-368, api/api.h:289-318). The C++ host class that
 * keeps the reference's region_model<cell_t> API (shyft_amd/csrc/host/) and
 * the Python surface (shyft_amd.api) call nothing but these functions.
 *
 * Conventions
 *  - Every function returns 0 on success, non-zero on error; the message is
 *    available from shyft_hip_last_error(h) (or shyft_hip_last_error(NULL) for
 *    errors raised before a handle exists). This replaces the std::runtime_error
 *    the reference throws (region_model.h:583-592, cell_model.h:198-211).
 *  - Cells are indexed 0..n_cells-1 in the caller's order. Host arrays are
 *    borrowed for the duration of the call; device memory is owned by the handle.
 *  - Time is int64 microseconds since 1970-01-01Z, as the reference's utctime
 *    (core/utctime_utilities.h:29-34). The time axis is fixed_dt
 *    (core/time_axis.h:74-115).
 *  - Arrays marked [A][B] are row-major: element (a, b) at a*B + b.
 */
#ifndef SHYFT_HIP_H
#define SHYFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shyft_hip_region shyft_hip_region;

/* method stacks (core/pt_gs_k.h, core/hbv_stack.h, core/pt_ss_k.h, core/pt_hs_k.h, core/pt_hps_k.h) */
enum shyft_hip_stack {
    SHYFT_HIP_PT_GS_K = 1, SHYFT_HIP_HBV_STACK = 2, SHYFT_HIP_PT_SS_K = 3, SHYFT_HIP_PT_HS_K = 4, SHYFT_HIP_PT_HPS_K = 5
};

/* forcing variables, the cell env_ts of core/cell_model.h:47-81 */
enum shyft_hip_forcing {
    SHYFT_HIP_TEMPERATURE = 0, SHYFT_HIP_PRECIPITATION = 1, SHYFT_HIP_WIND_SPEED = 2,
    SHYFT_HIP_REL_HUM = 3, SHYFT_HIP_RADIATION = 4
};

/* response collection (core/pt_gs_k_cell_model.h:41-150):
 *  DISCHARGE      = discharge_collector (avg_discharge, charge_m3s)
 *  DISCHARGE_SNOW = discharge_collector with collect_snow (+ snow_sca, snow_swe)
 *  ALL            = all_response_collector (8 series) */
enum shyft_hip_collect { SHYFT_HIP_COLLECT_DISCHARGE = 0, SHYFT_HIP_COLLECT_DISCHARGE_SNOW = 1, SHYFT_HIP_COLLECT_ALL = 2 };

/* pt_gs_k response series ids (all_response_collector member order) */
enum shyft_hip_ptgsk_series {
    SHYFT_HIP_AVG_DISCHARGE = 0, SHYFT_HIP_CHARGE_M3S = 1, SHYFT_HIP_SNOW_SCA = 2, SHYFT_HIP_SNOW_SWE = 3,
    SHYFT_HIP_SNOW_OUTFLOW = 4, SHYFT_HIP_GLACIER_MELT = 5, SHYFT_HIP_AE_OUTPUT = 6, SHYFT_HIP_PE_OUTPUT = 7
};

/* series ids accepted by the statistics / cell-series entry points besides the response ids above:
 * the cell environment (forcing) variable v as SHYFT_HIP_SERIES_FORCING + v, and state-collector
 * field f (T+1 instant axis) as SHYFT_HIP_SERIES_STATE + f. */
enum shyft_hip_series_base { SHYFT_HIP_SERIES_FORCING = 100, SHYFT_HIP_SERIES_STATE = 200 };

/* statistics scope (core/cell_model.h:183-186 stat_scope) */
enum shyft_hip_stat_scope { SHYFT_HIP_SCOPE_CELL_IX = 0, SHYFT_HIP_SCOPE_CATCHMENT = 1 };

const char* shyft_hip_last_error(const shyft_hip_region* h);

/* Replaces region_model(const vector<geo_cell_data>&, const parameter_t&) — core/region_model.h:285-293.
 * device < 0 selects the current HIP device. */
int shyft_hip_region_create(int stack, size_t n_cells, int device, shyft_hip_region** out);
void shyft_hip_region_destroy(shyft_hip_region* h);
/* One region whose cells are split into n_shards contiguous shards, shard k (cells [n*k/S, n*(k+1)/S)) on device
 * devices[k] -- devices may repeat (several shards on one device). Every entry point below works on the whole
 * region as on an unsharded one (cell indexes, catchment ids and series are the region's); the shards run
 * concurrently, one host thread per shard. This is region_model over all of a node's GPUs from one process
 * (core/region_model.h:972-1021 runs the whole region in one process). Catchment / routing-group / ensemble sums
 * add per-shard partial sums in shard order after an all-gather: RCCL (ncclAllGather over xGMI) when every shard
 * has its own device, device-to-device copies when shards share one; a catchment whose cells lie in one shard sums
 * exactly as on the unsharded region. Forcing and series move between host memory and the shards (no device
 * pointers: each shard's memory is on its own device). */
int shyft_hip_region_create_sharded(int stack, size_t n_cells, const int* devices, size_t n_shards,
                                    shyft_hip_region** out);
/* create_sharded with options. The combine path is chosen once, at creation: RCCL when every shard has its own
 * device (or with SHYFT_HIP_SHARD_RCCL_ALWAYS: also one shard, a one-rank communicator), then a self-check before any
 * data uses it -- an all-gather of known partials must arrive bit for bit on every device and their shard-order sum
 * must equal the device-copy path's bitwise. A failed communicator initialisation, a failed self-check, or an RCCL error
 * at run time switches the region to device copies (same results; shyft_hip_region_combine_report says why). Every
 * RCCL step has a deadline (SHYFT_HIP_RCCL_DEADLINE_MS, default 120 s; non-blocking communicators, polled): one that
 * stalls is aborted (ncclCommAbort) and handled like one that fails. No reference
 * counterpart: the reference's one-process region has no exchange (core/region_model.h:972-1021).
 * SHYFT_HIP_SHARD_NO_RCCL: device copies only. The TEST_ flags inject the failures for the fallback tests:
 * ncclCommInitAll failing, the first all-gather after the self-check failing, the self-check comparing unequal, the
 * self-check's all-gather not seen to complete before the deadline (TEST_STALL_CHECK).
 * SHYFT_HIP_SHARD_BALANCE_Z: instead of contiguous cell ranges, the first shyft_hip_set_geo ranks the cells by
 * elevation and deals rank r to shard r % n_shards (each shard keeps its cells in region order), so every shard holds
 * the same mix of elevations and so of snow-season work. Every entry point still takes the region's cell indexes;
 * results per cell are unchanged, catchment sums are partial sums added in shard order (each catchment now spans the
 * shards, so they are reassociated), and shyft_hip_region_shards reports shard k's cell count (cell0 is then only its
 * position in the deal). */
enum shyft_hip_shard_flags {
    SHYFT_HIP_SHARD_RCCL_ALWAYS = 1, SHYFT_HIP_SHARD_NO_RCCL = 2, SHYFT_HIP_SHARD_TEST_FAIL_INIT = 4,
    SHYFT_HIP_SHARD_TEST_FAIL_GATHER = 8, SHYFT_HIP_SHARD_TEST_CORRUPT_CHECK = 16, SHYFT_HIP_SHARD_BALANCE_Z = 32,
    SHYFT_HIP_SHARD_TEST_STALL_CHECK = 64
};
int shyft_hip_region_create_sharded_ex(int stack, size_t n_cells, const int* devices, size_t n_shards, unsigned flags,
                                       shyft_hip_region** out);
/* One line: the combine path, why it was chosen, the self-check result and any run-time fallback ("" unsharded). */
const char* shyft_hip_region_combine_report(const shyft_hip_region* h);
/* Number of shards (1 for an unsharded region); for k below it, shard k's device, first cell and cell count. */
size_t shyft_hip_region_shards(const shyft_hip_region* h, size_t k, int* device, size_t* cell0, size_t* n_cells);
/* How the shards' partial sums are combined: SHYFT_HIP_COMBINE_NONE (unsharded), _COPY (device copies), _RCCL. */
enum shyft_hip_combine { SHYFT_HIP_COMBINE_NONE = 0, SHYFT_HIP_COMBINE_COPY = 1, SHYFT_HIP_COMBINE_RCCL = 2 };
int shyft_hip_region_combine_path(const shyft_hip_region* h);
size_t shyft_hip_region_size(const shyft_hip_region* h);

/* Cell geometry, n_cells x 11 doubles in the geo_cell_data_io layout
 * (api/api.h:1598-1621): x y z area cid slope glacier lake reservoir forest unspecified.
 * routing_id / routing_distance (geo_cell_data.routing, core/geo_cell_data.h:83-92) may be NULL. */
int shyft_hip_set_geo(shyft_hip_region* h, const double* geo11, const int64_t* routing_id, const double* routing_distance);

/* Parameters: n_sets rows of the stack's calibration vector in the reference's
 * get/set order (pt_gs_k: 31 values, core/pt_gs_k.h:77-112; hbv_stack 22, hbv_stack.h:82-109;
 * pt_ss_k 21, pt_ss_k.h:78-101; pt_hs_k 18, pt_hs_k.h:66-88; pt_hps_k 24, pt_hps_k.h:64-90). hbv_stack and
 * pt_hs_k rows may carry 17 more values, the hbv_snow distribution: n_bins (2..8), s[8], intervals[8]; pt_hps_k
 * rows may carry 18 more: gm.direct_response, then that distribution; set_ix[n_cells]
 * selects the row of each cell (region parameter + catchment overrides,
 * region_model.h:287-319). set_ix == NULL means row 0 for every cell. */
int shyft_hip_set_parameters(shyft_hip_region* h, const double* params, size_t n_sets, size_t n_per_set,
                             const int32_t* set_ix);

/* Time axis (fixed_dt). Allocates forcing/response storage for a resident
 * window of window_steps steps starting at step 0 (window_steps == 0: whole axis).
 * Replaces initialize_cell_environment (region_model.h:359-364): forcing is NaN-filled.
 * Any dt_us > 0 is taken (sub-hourly, hours, days, not a whole number of seconds), with 1 <= n_steps <= INT32_MAX,
 * else "region_model::run with invalid time_axis invoked". Every step time t0_us + i * dt_us, i <= n_steps, must lie
 * within +-2^62 us of 1970-01-01 (about +-146 000 years), negative times included: there the day-of-year and
 * time-in-year tables of pt_gs_k are exact (proleptic Gregorian, UTC); an axis that leaves that range is refused
 * ("set_time_axis: step times beyond ..."). On a region that has already run, the call also has the dt-derived
 * pt_gs_k parameter columns rebuilt before the next run. */
int shyft_hip_set_time_axis(shyft_hip_region* h, int64_t t0_us, int64_t dt_us, size_t n_steps, size_t window_steps);
/* Move the resident window to start at step w0 (window length unchanged). Forcing
 * in the window becomes NaN, responses NaN. Used to stream long horizons in chunks. */
int shyft_hip_set_window(shyft_hip_region* h, size_t w0);
/* set_window with control over the NaN fill: fill_mask bit 0 forcing, bit 1 responses, bit 2 state series
 * (set_window == fill_mask 7). A caller that rewrites the whole window (a device forcing generator, a full
 * run_cells over the window) passes 0 and saves a pass over the window's HBM. */
int shyft_hip_move_window(shyft_hip_region* h, size_t w0, int fill_mask);

/* Collection mode (shyft_hip_collect) and state collection on/off
 * (set_state_collection / set_snow_sca_swe_collection, region_model.h:784-818). */
int shyft_hip_set_collection(shyft_hip_region* h, int collect, int collect_state);

/* Catchment calculation filter (region_model.h:715-779): cids[n] or n == 0 to clear. */
int shyft_hip_set_catchment_filter(shyft_hip_region* h, const int64_t* cids, size_t n);

/* State, n_cells x n_fields (pt_gs_k: 9 = gs albedo lwc surface_heat alpha sdc_melt_mean acc_melt
 * iso_pot_energy temp_swe, kirchner q; hbv_stack: 22 = swe sca sm uz lz n_bins sp[8] sw[8];
 * pt_ss_k: 8 = nu alpha sca swe free_water residual num_units q; pt_hs_k: 20 = swe sca n_bins sp[8]
 * sw[8] q; pt_hps_k: 37 = swe sca surface_heat n_bins sp[8] sw[8] albedo[8] iso_pot_energy[8] q).
 * get/set_states (region_model.h:784-805). */
int shyft_hip_set_state(shyft_hip_region* h, const double* state, size_t n_fields);
int shyft_hip_get_state(const shyft_hip_region* h, double* state, size_t n_fields);
/* dst's state := src's state, device to device (the same method stack and cell count, one device).
 * Replaces dst.set_states(src.get_states()) (region_model.h:784-805) without the host round trip: waits for
 * src's queued work, then copies on dst's stream. Used to pipeline two regions over consecutive windows. */
int shyft_hip_copy_state(shyft_hip_region* dst, const shyft_hip_region* src);

/* Forcing for steps [step0, step0+n) of one variable, [n][n_cells].
 * src_on_device != 0: src is a device pointer on the region's device. */
int shyft_hip_set_forcing(shyft_hip_region* h, int var, size_t step0, size_t n, const double* src, int src_on_device);
int shyft_hip_get_forcing(const shyft_hip_region* h, int var, size_t step0, size_t n, double* dst, int dst_on_device);

/* Inverse-distance interpolation of one forcing variable from n_sources geo-located sources
 * into the cells (region_model::interpolate's per-variable idw::run_interpolation,
 * core/region_model.h:456-515, core/inverse_distance.h:142-250), for steps [step0, step0+n)
 * of the resident window. Only cells passing the catchment calculation filter are written.
 *  src_xyz    : n_sources x 3 (geo_point x y z)
 *  src_values : [n][n_sources], the sources already averaged onto the model time axis
 *               (the average_accessor step, region_model.h:135-145, is the caller's)
 *  idw_param  : max_members (<= 32), max_distance, distance_measure_factor, zscale,
 *               default_temp_gradient, gradient_by_equation (0/1), precipitation scale_factor
 *               (inverse_distance.h:38-74)
 * Model by variable: temperature (gradient transform), precipitation (scale^(dz/100)),
 * radiation (x slope factor), wind_speed and rel_hum (plain). A single temperature source is
 * copied to every cell as the reference does (region_model.h:470-481). The neighbour table is
 * built on the first call and reused while sources and parameters are unchanged. */
int shyft_hip_interpolate(shyft_hip_region* h, int var, size_t n_sources, const double* src_xyz,
                          const double* src_values, size_t step0, size_t n, const double* idw_param);
/* Which gather the last shyft_hip_interpolate of variable var ran (no reference counterpart: a test and
 * measurement aid): SHYFT_HIP_IDW_WAVE (every wavefront's neighbour union fits 64 stations: the compacted
 * wavefront-union gather), SHYFT_HIP_IDW_TILE (the row-tile gather), SHYFT_HIP_IDW_COPY (one temperature source
 * copied), SHYFT_HIP_IDW_NONE (no interpolation of var yet). Returns -1 on a bad handle or variable. */
enum shyft_hip_idw_path { SHYFT_HIP_IDW_NONE = 0, SHYFT_HIP_IDW_TILE = 1, SHYFT_HIP_IDW_WAVE = 2, SHYFT_HIP_IDW_COPY = 3 };
int shyft_hip_interpolation_path(const shyft_hip_region* h, int var);

/* Bayesian temperature kriging of the temperature forcing into the calculated cells, steps [step0, step0+n)
 * of the resident window: region_model::interpolate's default temperature method
 * (core/region_model.h:460-468 -> bayesian_kriging::btk_interpolation, core/bayesian_kriging.h:280-402).
 *  src_xyz        : n_sources x 3
 *  src_values     : [n][n_sources] on the model axis (average_accessor is the caller's); NaN = missing, and
 *                   a step whose valid-source set differs from the full set uses the reference's reduced
 *                   operators for that set
 *  prior_gradient : [n] the prior temperature gradient per step (parameter.temperature_gradient(period)), or
 *                   NULL for bayesian_kriging::parameter's day-of-year formula on the region's time axis
 *                   (bayesian_kriging.h:220-223)
 *  btk_param      : temperature_gradient_sd (C/m, i.e. already /100), sill, nugget, range, zscale
 * One source is copied to the cells (region_model.h:470-481). Errors carry the reference's texts ("needs at
 * least two sources at different heights", "No valid sources for time period"). */
int shyft_hip_interpolate_btk(shyft_hip_region* h, size_t n_sources, const double* src_xyz, const double* src_values,
                              size_t step0, size_t n, const double* prior_gradient, const double* btk_param);
/* Stateless bayesian_kriging_temperature (api/boostpython/api_interpolation.cpp:54-71) on a device (device < 0 =
 * current): dst_xyz [n_dst][3], prior_gradient [n] (required), out [n][n_dst] host. */
int shyft_hip_btk(int device, size_t n_sources, const double* src_xyz, const double* src_values, size_t n,
                  const double* prior_gradient, const double* btk_param, size_t n_dst, const double* dst_xyz,
                  double* out);
/* shyft_hip_btk with at most block_steps steps of one valid-source pattern per product and placement (0 = the
 * default, bounded by memory only): a test aid that makes a short series take the multi-block path. */
int shyft_hip_btk_blocked(int device, size_t n_sources, const double* src_xyz, const double* src_values, size_t n,
                          const double* prior_gradient, const double* btk_param, size_t n_dst, const double* dst_xyz,
                          double* out, size_t block_steps);

/* Stateless ordinary kriging (api/boostpython/api_interpolation.cpp:86-148; covariances and the system of
 * core/kriging.h:23-135) on a device (device < 0 = current): weights = first n_sources rows of A^-1 B, A^-1 by LU
 * on the host, both products by the fixed-order fp64 kernel of kernels/ok.hip (no rocBLAS), so the result is
 * bit-identical to shyft_hip_ordinary_kriging_host. NaN observations are not filtered: a NaN makes its step NaN.
 * ok_param: c, a, z_scale, cov_type (0 GAUSSIAN, 1 EXPONENTIAL), dst_block (0 = default; else destinations
 * per pass, a test and measurement aid). src_values [n][n_sources] on the model axis; out [n][n_dst], host.
 * One source is copied to every destination without a device call (api_interpolation.cpp:141-146); n == 0 or
 * n_dst == 0 returns 0. Errors carry the reference's texts (api_interpolation.cpp:88-93) or
 * "inv(): matrix is singular". */
int shyft_hip_ordinary_kriging(int device, size_t n_sources, const double* src_xyz, const double* src_values, size_t n,
                               const double* ok_param, size_t n_dst, const double* dst_xyz, double* out);
/* The same arithmetic on the host, no device call: the restatement the device path is bit-identical to
 * (api_interpolation.cpp:86-148, core/kriging.h:23-135). */
int shyft_hip_ordinary_kriging_host(size_t n_sources, const double* src_xyz, const double* src_values, size_t n,
                                    const double* ok_param, size_t n_dst, const double* dst_xyz, double* out);
/* Measurement aid of tools/ok_bench.py (no reference counterpart): the three kernels of the ordinary-kriging
 * path (api_interpolation.cpp:86-148) on generated inputs of n_sources sources, n steps and n_dst destinations,
 * timed with HIP events, and rocBLAS dgemm on the same two product shapes (the calls kernels/btk.hip makes).
 * out_ms[6], best of `reps` passes: covariance, weights product, values product (each summed over the blocks of
 * dst_block destinations, 0 = default), dgemm weights shape, dgemm values shape, and the largest absolute
 * difference between the two paths' values. */
int shyft_hip_ok_bench(int device, size_t n_sources, size_t n, size_t n_dst, size_t dst_block, int reps,
                       double* out_ms);

/* Deterministic synthetic forcing for steps [step0, step0+n) of the resident window,
 * generated on device (bench/test workload; SURVEY.md §8d generator). */
int shyft_hip_synthetic_forcing(shyft_hip_region* h, uint64_t seed, uint64_t cell_offset, size_t step0, size_t n);
/* The synthetic region's cell elevations z[i] = 2000*u(seed, 7, cell_offset+i, 0) (same generator), n_cells values. */
int shyft_hip_synthetic_elevation(uint64_t seed, uint64_t cell_offset, size_t n_cells, double* z_host);

/* region_model::run_cells(use_ncore, start_step, n_steps) — region_model.h:578-597.
 * use_ncore is validated like the reference and otherwise ignored. Blocks until done. */
int shyft_hip_run_cells(shyft_hip_region* h, size_t use_ncore, int start_step, int n_steps);
/* Asynchronous variant on the region's stream (no argument re-validation of state). */
int shyft_hip_run_cells_async(shyft_hip_region* h, int start_step, int n_steps);
int shyft_hip_synchronize(shyft_hip_region* h);
/* Double-buffered forcing window (measurement / pipelining aid, no reference counterpart): generate the synthetic
   forcing of the window starting at w0_next into a second buffer on a side stream restricted to n_cus CUs (0: no
   restriction; < 0: the whole device at the lowest stream priority) while the current window runs (it waits only
   for the run that last read that buffer); shyft_hip_swap_forcing_window(h, w0_next) then makes it the
   region's window (the next run waits for the generator on the device). The swap does not NaN-fill the response
   and state-series rows: a run over the new window must follow before they are read. A pending prefetch is
   dropped when the time axis or window length changes (shyft_hip_set_time_axis). */
int shyft_hip_prefetch_synthetic_forcing(shyft_hip_region* h, uint64_t seed, uint64_t cell_offset, size_t w0_next,
                                         int n_cus);
int shyft_hip_swap_forcing_window(shyft_hip_region* h, size_t w0_next);
/* Milliseconds of the last run_cells kernel launch(es), timed with HIP events on the region's stream. */
double shyft_hip_last_run_ms(const shyft_hip_region* h);
/* The last run's kernels separately: every stack runs one kernel per run_cells, so parts is 1 (ms[0] = the kernel;
   a sharded region: the slowest running shard's). Fills ms[0..min(n, parts)) and returns the number of parts.
   (No reference counterpart: measurement only.) */
int shyft_hip_last_run_kernel_ms(const shyft_hip_region* h, double* ms, int n);
/* Milliseconds of the last shyft_hip_interpolate's gather kernel (HIP events on the region's stream; the neighbour
   table build of a new source geometry is not included). A sharded region: the slowest interpolating shard's.
   (No reference counterpart: measurement only.) */
double shyft_hip_last_interpolate_ms(const shyft_hip_region* h);
/* Kernel milliseconds of the last run_cells of every shard (0 for a shard idle under the catchment filter) into
   ms[0..min(n, shards)); returns the number of shards (1 and the region's own time when unsharded). */
size_t shyft_hip_shard_run_ms(const shyft_hip_region* h, double* ms, size_t n);

/* Response series for steps [step0, step0+n), [n][n_cells]. */
int shyft_hip_get_series(const shyft_hip_region* h, int series, size_t step0, size_t n, double* dst, int dst_on_device);
/* State-collector series (instant, T+1 axis), field f in state order, steps [step0, step0+n). */
int shyft_hip_get_state_series(const shyft_hip_region* h, int field, size_t step0, size_t n, double* dst,
                               int dst_on_device);

/* Catchment statistics (cell_statistics::sum_catchment_feature / average_catchment_feature,
 * core/cell_model.h:228-333): sum (weighted == 0) or area-weighted average (weighted != 0)
 * of series `series` (response id, SHYFT_HIP_SERIES_FORCING + v or SHYFT_HIP_SERIES_STATE + f) over the cells selected by ids[n_ids] (scope: cell index or catchment id;
 * n_ids == 0 selects all cells), for steps [step0, step0+n). dst[n]. Throws (returns error)
 * on unknown ids like verify_cids_exist (cell_model.h:198-211). */
int shyft_hip_statistics(const shyft_hip_region* h, int series, const int64_t* ids, size_t n_ids, int scope,
                         int weighted, size_t step0, size_t n, double* dst);
/* Per-catchment sums of a series for all catchments at once (region_model::catchment_discharges,
 * region_model.h:873-885): dst[n_catchments][n] in catchment_ids() order, device or host. */
int shyft_hip_catchment_sums(const shyft_hip_region* h, int series, size_t step0, size_t n, double* dst,
                             int dst_on_device);
/* Per-catchment sums of value x cell area (calculated catchments, cell order, same reduction as
 * shyft_hip_catchment_sums): the area-weighted snow sca/swe sums of the calibration goal function
 * (optimizer::extract_area_ts_property, core/model_calibration.h:759-776). dst[n_catchments][n]. */
int shyft_hip_catchment_area_sums(const shyft_hip_region* h, int series, size_t step0, size_t n, double* dst,
                                  int dst_on_device);

/* Percentiles across cells (calculate_percentiles with skip_nans, core/time_series_statistics.h:112-246, the
 * api.percentiles / TsVector.percentiles of api/boostpython/api_time_series.cpp, taken over the cells of a region on
 * its own time axis). For every step the samples are the finite values of the selected cells; pct[k] is
 *   0..100   the R7 percentile as the reference evaluates it (:133-153, with its eps = 1e-30 rules),
 *   -1       AVERAGE: the mean of the samples (:127-132),
 *   -1000 / +1000  MIN_EXTREME / MAX_EXTREME: the smallest / largest sample (one value per series and interval,
 *            so extract_statistic_from_vector with nan_min / nan_max, :25-39, :77-90, :221-226, is that),
 *   anything else, or no finite sample: NaN.
 * Order statistics are exact: every entry but AVERAGE is bit-identical to shyft_hip_percentiles_host (the sign of
 * a zero result is unspecified, as +0.0 and -0.0 compare equal in a sort); AVERAGE is a fixed-order sum, reproducible
 * run to run, that differs from the host's sorted sequential sum by rounding only. n_pct is at most
 * SHYFT_HIP_PERCENTILES_MAX; n_pct == 0 returns 0 and writes nothing. A segment (the selection, or a catchment) of at
 * most SHYFT_HIP_PERCENTILES_LDS_MAX cells is sorted in LDS by one workgroup per step; a call with a larger segment
 * runs a radix select over the 64-bit keys of the values (kernels/percentiles.hip). A sharded region returns an
 * error ("percentiles: not available for a sharded region"). */
#define SHYFT_HIP_PERCENTILES_MAX 16
#define SHYFT_HIP_PERCENTILES_LDS_MAX 4096
enum shyft_hip_statistics_property {
    SHYFT_HIP_STAT_AVERAGE = -1, SHYFT_HIP_STAT_MIN_EXTREME = -1000, SHYFT_HIP_STAT_MAX_EXTREME = 1000
};
/* Series ids, selection (ids[n_ids], scope; n_ids == 0 selects all cells), window and unknown-id errors as
 * shyft_hip_statistics. dst is host [n_pct][n]. A selection that matches no cell gives NaN. */
int shyft_hip_percentiles(const shyft_hip_region* h, int series, const int64_t* ids, size_t n_ids, int scope,
                          const int64_t* pct, size_t n_pct, size_t step0, size_t n, double* dst);
/* The same for every catchment in one call: dst[n_catchments][n_pct][n] in catchment_ids() order, device or host. */
int shyft_hip_catchment_percentiles(const shyft_hip_region* h, int series, const int64_t* pct, size_t n_pct,
                                    size_t step0, size_t n, double* dst, int dst_on_device);
/* The host restatement, no device call (time_series_statistics.h:115-160): rows [n_steps][n_samples_per_step], the
 * non-finite samples of a step dropped, a full sort per step, AVERAGE summed sequentially over the sorted samples.
 * dst [n_pct][n_steps]; n_pct is not limited here. */
int shyft_hip_percentiles_host(const double* rows, size_t n_steps, size_t n_samples_per_step, const int64_t* pct,
                               size_t n_pct, double* dst);
/* Which path the last percentile call of this region took (no reference counterpart: a test and measurement aid):
 * SHYFT_HIP_PERCENTILES_NONE (none yet, or nothing was launched), _LDS_SORT, _RADIX. Returns -1 on a bad handle. */
enum shyft_hip_percentiles_path_id {
    SHYFT_HIP_PERCENTILES_NONE = 0, SHYFT_HIP_PERCENTILES_LDS_SORT = 1, SHYFT_HIP_PERCENTILES_RADIX = 2
};
int shyft_hip_percentiles_path(const shyft_hip_region* h);
/* Milliseconds of the last percentile call's kernels, first launch to last, timed with HIP events on the region's
 * stream; uploads and the copy of the result are not included. (No reference counterpart: measurement only.) */
double shyft_hip_last_percentiles_ms(const shyft_hip_region* h);

/* Batched Kalman bias filter (core/kalman.h:24-236): M independent filters of size n = n_daily_observations run T
 * steps of filter::update (kalman.h:127-145) in one launch of kernels/kalman.hip on a device (device < 0 = current).
 * Host pointers, stateless. Structure-of-arrays, point fastest: bias [T][M]; x [n][M], k [n][M] and P [n*n][M]
 * (row-major i*n+j) are read and written in place. Step-uniform tables: fold [T], the daily index of each step
 * (filter::fold_to_daily_observation, kalman.h:114-116); w [n/2+1], the distinct values of W by folded distance
 * min(|i-j|, n-|i-j|) (state::make_covariance, kalman.h:37-50); v2 = std_error_bias_measurements^2.
 * mode 0, filter (filter::update): a non-finite bias still does P += W and leaves x and k untouched.
 * mode 1, predictor (bias_predictor::update_with_forecast / compute_running_bias, kalman.h:173-185, 203-236): a
 * non-finite bias skips the step, the state stays bitwise unchanged.
 * out [T][M], or NULL: the running bias of compute_running_bias (mode 1 only). Every save_every steps from step 0
 * the profile is a snapshot of x; out[t] is written before step t's update as the average of that snapshot over
 * the pieces piece_begin[t] .. piece_begin[t+1] of step t (CSR; piece_ix the profile index, piece_seconds the
 * length of each piece): pieces in order, sum of v * seconds over the finite v, one division by the sum of their
 * seconds (accumulate_value as profile_accessor::value(i) calls it, core/time_series.h:203-305, 682-688).
 * M == 0 or T == 0 returns 0 and writes nothing; n outside 1..32 is an error. Every element of the update is
 * evaluated as written (no FMA, every division a division), so the result is bit-identical to
 * shyft_hip_kalman_run_host. */
int shyft_hip_kalman_run(int device, int n, size_t M, size_t T, const double* bias, const int32_t* fold, const double* w,
                         double v2, int mode, double* x, double* k, double* P, double* out, int save_every,
                         const int32_t* piece_begin, const int32_t* piece_ix, const double* piece_seconds);
/* The same arithmetic in plain C++, no device call (core/kalman.h:127-145, 173-185, 203-236); any n >= 1. */
int shyft_hip_kalman_run_host(int n, size_t M, size_t T, const double* bias, const int32_t* fold, const double* w, double v2,
                              int mode, double* x, double* k, double* P, double* out, int save_every,
                              const int32_t* piece_begin, const int32_t* piece_ix, const double* piece_seconds);
/* state::state's matrices (core/kalman.h:31-50): P = make_covariance(n, covariance_init, hourly_correlation) and
 * W = make_covariance(n, process_noise_init^2, hourly_correlation), both [n][n], with detmath::pow for the power so
 * the matrices are the same on every machine. */
int shyft_hip_kalman_initial_state(int n, double covariance_init, double hourly_correlation, double process_noise_init,
                                   double* P, double* W);
/* HIP-event milliseconds of the kernel of the last shyft_hip_kalman_run on this device (device < 0 = current), copies
 * excluded. (No reference counterpart in core/kalman.h: measurement only.) */
double shyft_hip_kalman_last_ms(int device);

/* Quantile mapping of weighted forecasts onto historical scenarios (core/time_series_qm.h): per step, quantile_index
 * (:34-52) of the F forecast and the P scenario values, wvo_accessor's normalised weights (:187-210),
 * compute_weighted_quantiles (:80-100) or compute_interp_weighted_quantiles (:139-170) with one quantile per finite
 * scenario, and quantile_mapping's write-back by scenario rank with the interpolation blend (:325-347), in one launch
 * of kernels/qm.hip on a device (device < 0 = current). Host pointers, stateless. B independent problems share the
 * axis, the weights and the shapes: fc [B][T][F] and pri [B][T][P] are the values averaged onto the axis (NaN = not
 * covered), w [F] the weight of each forecast, out [B][T][P]. mode [T] and interp_weight [T] are what
 * quantile_mapping derives from the times (:310-311, :328, :335-339): PRIOR, the step keeps its scenarios; QM, scenario
 * of rank i gets quantile i; QM_BLEND, (1 - interp_weight) * quantile + interp_weight * scenario. A step without a
 * finite forecast is PRIOR; scenarios that are not finite at a QM step get NaN. Equal values are ranked by ascending
 * series index (the reference's std::sort leaves their order open; +0.0 and -0.0 are equal). With one finite scenario
 * the quantile is the lowest forecast for both kinds (the reference reads out of range for the interpolated kind).
 * Every weight must be finite and > 0: the reference's loops do not terminate otherwise. B*T == 0 or P == 0 returns 0
 * and launches nothing; F or P above SHYFT_HIP_QM_MAX_SERIES is an error on the device. The prefix sums are formed
 * sequentially in rank order and every operation is evaluated as written (no FMA), so the result is bit-identical to
 * shyft_hip_quantile_map_host. */
#define SHYFT_HIP_QM_MAX_SERIES 1024
#define SHYFT_HIP_QM_PRIOR 0
#define SHYFT_HIP_QM_QM 1
#define SHYFT_HIP_QM_BLEND 2
int shyft_hip_quantile_map(int device, size_t B, size_t T, size_t F, size_t P, const double* fc, const double* w,
                           const double* pri, const int32_t* mode, const double* interp_weight,
                           int interpolated_quantiles, double* out);
/* The same arithmetic in plain C++ (host/qm.hpp map_step; core/time_series_qm.h:34-210, 325-347), no device call; any
 * F and P. */
int shyft_hip_quantile_map_host(size_t B, size_t T, size_t F, size_t P, const double* fc, const double* w,
                                const double* pri, const int32_t* mode, const double* interp_weight,
                                int interpolated_quantiles, double* out);
/* The launch shape of the last shyft_hip_quantile_map kernel on this device (device < 0 = current): WAVE, one
 * wavefront per (problem, step) when the padded max(F, P) is at most 64; GROUP, one workgroup each. (No reference
 * counterpart in core/time_series_qm.h: test and measurement aid.) */
#define SHYFT_HIP_QM_PATH_NONE 0
#define SHYFT_HIP_QM_PATH_WAVE 1
#define SHYFT_HIP_QM_PATH_GROUP 2
int shyft_hip_quantile_map_last_path(int device);
/* HIP-event milliseconds of the last shyft_hip_quantile_map kernel on this device, copies excluded. (No reference
 * counterpart in core/time_series_qm.h: measurement only.) */
double shyft_hip_quantile_map_last_ms(int device);

/* S point series resampled onto the fixed_dt axis (ta_t0, ta_dt, T) in one launch of kernels/resample.hip on a device
 * (device < 0 = current); it replaces one average_accessor / integral_ts / accumulate_ts pass per series. Host
 * pointers, stateless. The series are in CSR form: row [S+1] point offsets (row[0] == 0), t [row[S]] point times in
 * int64 microseconds, v [row[S]] values, t_end [S] the end of each series' last interval, fx [S] POINT_INSTANT_VALUE
 * (0, linear between points) or POINT_AVERAGE_VALUE (1, stair-case). out is [T][S], series fastest. mode:
 *  AVERAGE     average_accessor::value(i) with USE_NAN (core/time_series.h:2033-2072 over average_value :302-306 and
 *              accumulate_value :202-288): NaN for a period that starts at or after the series' end, else the area of
 *              the non-NaN parts divided by to_seconds of their time;
 *  INTEGRAL    integral_ts::value(i) (core/time_series_dd.h:532-538): that area, NaN when no time is covered; no
 *              end-of-series rule;
 *  ACCUMULATE  accumulate_ts::values() (core/time_series_dd.h:672-679), accumulate_accessor::value(i) in ascending i
 *              (core/time_series.h:2100-2120): 0.0 at step 0, NaN once time(i) >= the series' end, else the running
 *              sum of the areas of [time(i-1), time(i)), added in that order; a NaN stays.
 * A series with no points gives NaN (ACCUMULATE: 0.0 at step 0, NaN after). Checked on the host before the launch,
 * with the texts of host/time_series.hpp point_ts (core/time_axis.h:271-293): times increase strictly within a row
 * ("time_axis::point_dt() needs time-points in increasing order"), t_end lies after the last point
 * ("time_axis::point_dt() illegal end-of-axis"), ta_dt > 0. A one-point series whose point lies strictly inside a period is an error, as in the
 * reference (accumulate_value asks point_dt::time for point 1, which throws). S == 0 or T == 0 returns 0 and launches
 * nothing. Every operation is evaluated as written (int64 ticks, to_seconds as a division, no FMA), so the result is
 * bit-identical to shyft_hip_resample_host. */
#define SHYFT_HIP_RESAMPLE_AVERAGE 0
#define SHYFT_HIP_RESAMPLE_INTEGRAL 1
#define SHYFT_HIP_RESAMPLE_ACCUMULATE 2
int shyft_hip_resample(int device, int mode, size_t S, const int64_t* row, const int64_t* t, const double* v,
                       const int64_t* t_end, const int32_t* fx, int64_t ta_t0, int64_t ta_dt, size_t T, double* out);
/* The same values from average_values / accumulate_value of host/time_series.hpp (the restatement of
 * core/time_series.h:202-310, 2033-2072) and a literal accumulate_accessor loop (:2100-2120); no device call, `device`
 * is not used. */
int shyft_hip_resample_host(int device, int mode, size_t S, const int64_t* row, const int64_t* t, const double* v,
                            const int64_t* t_end, const int32_t* fx, int64_t ta_t0, int64_t ta_dt, size_t T,
                            double* out);
/* HIP-event milliseconds of the kernel or kernels of the last shyft_hip_resample on this device (device < 0 =
 * current), copies excluded. (No reference counterpart: measurement only.) */
double shyft_hip_resample_last_ms(int device);
/* The number of shyft_hip_resample calls that launched on this device so far. (No reference counterpart: test aid.) */
uint64_t shyft_hip_resample_calls(int device);
/* The launch shape of the (series, interval) kernel: DIRECT, one lane per job and its own store; TILED, a workgroup
 * per 16 series x 64 intervals, lanes interval-fastest, stored series-fastest through LDS. AUTO takes TILED from 64
 * intervals on. set_path is process-wide; last_path reports what the last call on the device ran. (No reference
 * counterpart: test and measurement aid.) */
#define SHYFT_HIP_RESAMPLE_PATH_AUTO 0
#define SHYFT_HIP_RESAMPLE_PATH_DIRECT 1
#define SHYFT_HIP_RESAMPLE_PATH_TILED 2
int shyft_hip_resample_set_path(int path);
int shyft_hip_resample_last_path(int device);

/* Percentiles of a vector of point series on the fixed_dt axis (ta_t0, ta_dt, T) in one fused launch of
 * kernels/ts_percentiles.hip on a device (device < 0 = current): calculate_percentiles with skip_nans = true
 * (core/time_series_statistics.h:184-246), which api.percentiles binds (api_time_series.cpp:1299). It replaces one
 * average_accessor per series (core/time_series.h:2033-2072), the sample sort of every interval
 * (time_series_statistics.h:115-160) and the extract_statistic_from_vector passes (:41-90, :221-226). Host pointers,
 * stateless. The R stored series are in the CSR form of shyft_hip_resample (row [R+1], t and v [row[R]], t_end [R],
 * fx [R]). The vector has S views: view s is stored series src[s] in [0, R) with every point time and its t_end moved
 * by shift[s] microseconds (time_shift_ts, core/time_series_dd.h:707-751), so the partitions of one record
 * (ts.partition_by, core/time_series.h:2451-2494, time_series_dd.cpp:653-663) share one stored copy. The sample of
 * (view, interval) is mode AVERAGE of shyft_hip_resample on the moved series; non-finite samples are dropped. pct[k]:
 *   0..100   the R7 percentile with the reference's eps = 1e-30 rules (:133-153),
 *   -1       AVERAGE: the sorted samples added in sorted order, over their count (:127-132),
 *   -1000 / +1000  MIN_EXTREME / MAX_EXTREME: nan_min / nan_max (:24-39) folded over the values of the points whose
 *            moved times lie inside the interval, across all views; not an order statistic of the averages,
 *   anything else, or an interval without a finite sample: NaN.
 * out is [n_pct][T]. Checked before any work with the texts of shyft_hip_resample: increasing times, t_end after the
 * last point, ta_dt > 0, the one-point-series refusal (on the moved series); src[s] out of range is an error that
 * names the view. S == 0, T == 0 or n_pct == 0 returns 0 and launches nothing. n_pct above SHYFT_HIP_PERCENTILES_MAX
 * or S above SHYFT_HIP_TS_PERCENTILES_MAX_SERIES is refused on the device, the text naming the limit. Every entry,
 * AVERAGE included, is bit-identical to shyft_hip_ts_percentiles_host; the sign of a zero result is unspecified (+0.0
 * and -0.0 compare equal in a sort and in min / max). */
#define SHYFT_HIP_TS_PERCENTILES_MAX_SERIES 4096
int shyft_hip_ts_percentiles(int device, size_t R, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, size_t S, const int32_t* src,
                             const int64_t* shift, int64_t ta_t0, int64_t ta_dt, size_t T, const int64_t* pct,
                             size_t n_pct, double* out);
/* The same values from host/ts_percentiles.hpp, the restatement of time_series_statistics.h:24-90, 115-160 and
 * 184-246 over average_values of host/time_series.hpp; no device call, `device` is not used, S and n_pct are not
 * limited. */
int shyft_hip_ts_percentiles_host(int device, size_t R, const int64_t* row, const int64_t* t, const double* v,
                                  const int64_t* t_end, const int32_t* fx, size_t S, const int32_t* src,
                                  const int64_t* shift, int64_t ta_t0, int64_t ta_dt, size_t T, const int64_t* pct,
                                  size_t n_pct, double* out);
/* HIP-event milliseconds of the kernel of the last shyft_hip_ts_percentiles on this device (device < 0 = current),
 * copies excluded. (No reference counterpart: measurement only.) */
double shyft_hip_ts_percentiles_last_ms(int device);
/* The number of shyft_hip_ts_percentiles calls that launched on this device so far. (No reference counterpart: test
 * aid.) */
uint64_t shyft_hip_ts_percentiles_calls(int device);
/* The launch shape: WAVE, one wavefront per interval, one view per lane, the keys sorted across the lanes (S <= 64);
 * LDS, one workgroup per interval, the keys sorted in LDS. AUTO takes WAVE up to 64 views and LDS above. A forced
 * WAVE with more than 64 views is an error. set_path is process-wide; last_path reports what the last call on the
 * device ran. (No reference counterpart: test and measurement aid.) */
#define SHYFT_HIP_TS_PERCENTILES_PATH_AUTO 0
#define SHYFT_HIP_TS_PERCENTILES_PATH_WAVE 1
#define SHYFT_HIP_TS_PERCENTILES_PATH_LDS 2
int shyft_hip_ts_percentiles_set_path(int path);
int shyft_hip_ts_percentiles_last_path(int device);

/* Observation preparation of S point series in one device call each (kernels/tsprep.hip; device < 0 = current). Host
 * pointers, stateless. The series are in the CSR form of shyft_hip_resample (row [S+1], t and v [row[S]], t_end [S],
 * fx [S]) and are checked in the same way and with the same texts before anything is launched: row[0] == 0 and
 * non-decreasing, times strictly increasing in a series, t_end after the last point, times within a quarter of the
 * 64-bit range. out holds one double per input point (per query for ice-packing) in the same CSR order. A refused
 * batch launches nothing; S == 0 or zero points (queries) returns 0 and launches nothing. Every operation is
 * evaluated as written (int64 ticks, to_seconds as a division, no FMA, detmath exp and pow), so each entry is
 * bit-identical to its _host twin, which runs host/ts_prep.hpp on one thread and does not use `device`.
 *
 * shyft_hip_ts_rating_curve replaces rating_curve_ts::value(i) = rating_curve_parameters::flow(time(i), value(i))
 * per series (core/time_series.h:1493-1506, 1395-1408, 1641-1644). The parameter packs are a three-level CSR:
 * pack_row [P+1] offsets into curve_t [C] (the start times of a pack's curves, strictly increasing in a pack),
 * curve_row [C+1] offsets into seg [G][4] = lower, a, b, c (sorted on lower in a curve); pack_of [S] is the pack of
 * each series. NaN before the first curve, below the first segment and for a pack without curves; a curve without
 * segments that a point would use is refused with the reference's "no rating-curve segments". */
int shyft_hip_ts_rating_curve(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                              const int64_t* t_end, const int32_t* fx, size_t P, const int64_t* pack_row,
                              const int64_t* curve_t, const int64_t* curve_row, const double* seg, const int64_t* pack_of,
                              double* out);
int shyft_hip_ts_rating_curve_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                   const int64_t* t_end, const int32_t* fx, size_t P, const int64_t* pack_row,
                                   const int64_t* curve_t, const int64_t* curve_row, const double* seg,
                                   const int64_t* pack_of, double* out);
/* shyft_hip_ts_ice_packing replaces ice_packing_ts::detect_ice_packing(t) per query (core/time_series.h:1808-1831;
 * value(i) and operator()(t)): 1.0 when the average temperature over [t - window, t) lies below the threshold, 0.0
 * when not or when the period is empty, NaN when it cannot be told under the policy (0 DISALLOW_MISSING,
 * 1 ALLOW_INITIAL_MISSING, 2 ALLOW_ANY_MISSING). The series are the temperatures; the query times are a CSR of their
 * own, qrow [S+1] and qt [qrow[S]], so the series' own points and any other axis are served alike. window [S] (ticks,
 * >= 0), threshold [S], policy [S]. out is [qrow[S]]. A one-point series queried under DISALLOW_MISSING with a window
 * that starts before the point and holds it is an error, as in the reference (point_dt::time throws). */
int shyft_hip_ts_ice_packing(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, const int64_t* qrow, const int64_t* qt,
                             const int64_t* window, const double* threshold, const int32_t* policy, double* out);
int shyft_hip_ts_ice_packing_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                  const int64_t* t_end, const int32_t* fx, const int64_t* qrow, const int64_t* qt,
                                  const int64_t* window, const double* threshold, const int32_t* policy, double* out);
/* shyft_hip_ts_ice_packing_recession replaces ice_packing_recession_ts::values() (core/time_series_dd.h:1313-1354).
 * The series are the flows; ice [row[S]] is the indicator already sampled at the flow's points, ice_start / ice_end
 * [S] the indicator's total period for ensure_overlap (:1358-1362, same text), alpha [S] and recession_minimum [S]
 * the parameters. Without ice the flow's own f(t); with ice the recession from the last earlier point without ice
 * (point 0 of the series when there is none); NaN on a non-finite indicator at the point or where the walk ends. */
int shyft_hip_ts_ice_packing_recession(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                       const int64_t* t_end, const int32_t* fx, const double* ice,
                                       const int64_t* ice_start, const int64_t* ice_end, const double* alpha,
                                       const double* recession_minimum, double* out);
int shyft_hip_ts_ice_packing_recession_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                            const int64_t* t_end, const int32_t* fx, const double* ice,
                                            const int64_t* ice_start, const int64_t* ice_end, const double* alpha,
                                            const double* recession_minimum, double* out);
/* shyft_hip_ts_min_max_fill replaces qac_ts::value(i) without a replacement series (core/time_series_dd.cpp:1335-1376,
 * qac_parameter core/time_series_dd.h:1456-1478): a finite value inside [min_x, max_x] (NaN = no limit) stays, any
 * other becomes the line through the nearest valid neighbours, or NaN at the first and last point, with
 * max_timespan == 0, without such neighbours, or when they lie more than max_timespan [S] (ticks) apart. */
int shyft_hip_ts_min_max_fill(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                              const int64_t* t_end, const int32_t* fx, const double* min_x, const double* max_x,
                              const int64_t* max_timespan, double* out);
int shyft_hip_ts_min_max_fill_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                   const int64_t* t_end, const int32_t* fx, const double* min_x, const double* max_x,
                                   const int64_t* max_timespan, double* out);
/* HIP-event milliseconds of the kernels of the last shyft_hip_ts_* device call on this device, copies excluded, and
 * the number of such calls that launched so far. (No reference counterpart: measurement and test aid.) */
double shyft_hip_tsprep_last_ms(int device);
uint64_t shyft_hip_tsprep_calls(int device);

/* The point-wise filter series of S point series in one device call each (kernels/tsfilter.hip; device < 0 = current).
 * Host pointers, stateless. The series are in the CSR form of shyft_hip_resample and are checked in the same way and
 * with the same texts (prefix "ts_filter") before anything is launched. out holds one double per input point in the
 * same CSR order. A refused batch launches nothing; S == 0 or zero points returns 0 and launches nothing. Every
 * operation is evaluated as written (int64 ticks, to_seconds as a division, no FMA), so each entry is bit-identical to
 * its _host twin, which runs host/ts_filter.hpp on one thread and does not use `device`.
 *
 * shyft_hip_ts_convolve_w replaces convolve_w_ts::value(i) (core/time_series.h:966-975; apoint_ts::convolve_w,
 * core/time_series_dd.h:919-950): v = 0.0, then for j = 0 .. K-1 in that order v += w[j] * x[i-j], and where j > i the
 * policy's stand-in: 0 USE_FIRST w[j] * x[0], 1 USE_ZERO 0.0, 2 USE_NAN NaN. The weight profiles are a CSR, w_row [W+1]
 * offsets into w; w_of [S] names the profile of a series, policy [S] its policy. A profile without weights gives 0.0.
 * Refused: a w_row that does not start at 0 or decreases, w_of outside [0, W), a policy outside 0..2 and, by the
 * device entry only, a used profile of more than 65,536 weights. */
int shyft_hip_ts_convolve_w(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                            const int64_t* t_end, const int32_t* fx, size_t W, const int64_t* w_row, const double* w,
                            const int64_t* w_of, const int32_t* policy, double* out);
int shyft_hip_ts_convolve_w_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                 const int64_t* t_end, const int32_t* fx, size_t W, const int64_t* w_row,
                                 const double* w, const int64_t* w_of, const int32_t* policy, double* out);
/* shyft_hip_ts_derivative replaces derivative_ts::values() (core/time_series_dd.cpp:450-463) with derivative_fx
 * (:311-448). A POINT_INSTANT_VALUE series gives the slope to the next point and NaN at its last point; a
 * POINT_AVERAGE_VALUE series the method's difference, method [S]: 0 default (= center), 1 forward, 2 backward,
 * 3 center, with the reference's rules for non-finite neighbours. fixed_dt [S] (ticks) > 0 takes the reference's
 * fixed-step branch and must be the spacing of every point of the series and of t_end; 0 takes the variable branch.
 * Refused: a method outside 0..3, fixed_dt < 0, a fixed_dt > 0 that is not the series' spacing. */
int shyft_hip_ts_derivative(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                            const int64_t* t_end, const int32_t* fx, const int64_t* fixed_dt, const int32_t* method,
                            double* out);
int shyft_hip_ts_derivative_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                 const int64_t* t_end, const int32_t* fx, const int64_t* fixed_dt,
                                 const int32_t* method, double* out);
/* shyft_hip_ts_inside replaces inside_ts::values() = inside_parameter::inside_value per point
 * (core/time_series_dd.h:1546-1554; core/time_series_dd.cpp:1409-1426): nan_x for a non-finite value, x_outside below
 * a finite min_x or at or above a finite max_x, x_inside otherwise. Each parameter is [S]. */
int shyft_hip_ts_inside(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                        const int64_t* t_end, const int32_t* fx, const double* min_x, const double* max_x,
                        const double* nan_x, const double* x_inside, const double* x_outside, double* out);
int shyft_hip_ts_inside_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, const double* min_x, const double* max_x,
                             const double* nan_x, const double* x_inside, const double* x_outside, double* out);
/* shyft_hip_ts_decode replaces decode_ts::values() = bit_decoder::decode per point (core/time_series_dd.h:1650-1655;
 * core/time_series_dd.cpp:1428-1445): NaN for a non-finite or negative value or one above 2^52, else the n_bits [S]
 * bits from start_bit [S] of the value as an unsigned integer. Refused with the texts of apoint_ts::decode
 * (core/time_series_dd.cpp:943-946): "start_bit must be in range [0..51], was N" and "n_bits must be > 0 and
 * start_bit+n_bits <= 51: n_bits =N, start_bit=M". */
int shyft_hip_ts_decode(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                        const int64_t* t_end, const int32_t* fx, const int32_t* start_bit, const int32_t* n_bits,
                        double* out);
int shyft_hip_ts_decode_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, const int32_t* start_bit, const int32_t* n_bits,
                             double* out);
/* HIP-event milliseconds of the kernel of the last of these four device calls on this device, copies excluded, and the
 * number of such calls that launched so far. (No reference counterpart: measurement and test aid.) */
double shyft_hip_tsfilter_last_ms(int device);
uint64_t shyft_hip_tsfilter_calls(int device);
/* The launch shape of shyft_hip_ts_convolve_w: DIRECT, one lane per point with taps and values from global memory;
 * TILED, a workgroup per 256 consecutive points of one series, the values staged through LDS in chunks of 256 taps.
 * AUTO takes TILED from 2 weights on when the tiles are at least a quarter full on average. set_path is process-wide;
 * last_path reports what the last convolve_w on the device ran. (No reference counterpart: test and measurement aid.) */
#define SHYFT_HIP_TSFILTER_PATH_AUTO 0
#define SHYFT_HIP_TSFILTER_PATH_DIRECT 1
#define SHYFT_HIP_TSFILTER_PATH_TILED 2
int shyft_hip_tsfilter_set_path(int path);
int shyft_hip_tsfilter_last_path(int device);

/* Time-series arithmetic: E expressions over S terminal point series, every point of every expression in one launch
 * of kernels/ts_expr.hip on a device (device < 0 = current). An expression is the reference's lazy apoint_ts tree of
 * ts op ts, ts op scalar, scalar op ts (ADD SUB MUL DIV MAX MIN POW) and abs (core/time_series_dd.h:825-872, 1705-1890;
 * core/time_series_dd.cpp:70-129, 197-224, 835-920), planned by host/ts_expr.hpp make_plan into a postfix program of
 * int32 words; that header states the words, the two evaluation modes and the axis rules. The terminals are in the CSR
 * form of shyft_hip_resample. Expression e runs prog[prog_row[e] .. prog_row[e+1]) at each of its output points
 * orow[e] .. orow[e+1), whose times (the root axis, int64 microseconds) are ot; consts [n_const] and periods
 * [n_period][2] = start, end are the tables the programs index. out [orow[E]] receives what the reference's values()
 * gives for the expression, with detmath::pow for std::pow.
 * Refused before anything is launched: malformed series (the texts of shyft_hip_resample, prefix "ts_expr"), rows that
 * do not start at 0 or decrease, unknown words, operation, terminal, constant or period indexes out of range, a stack
 * that underflows or does not end at depth 1, a LOAD_RAW of a terminal whose size is not the expression's, and, by the
 * device entry only, a stack deeper than 8 values or a program longer than 64 words; _host evaluates those.
 * E == 0 or orow[E] == 0 returns 0 and launches nothing. _host runs the interpreter of host/ts_expr.hpp on one thread
 * and ignores device; the device result is bit-identical to it, NaN matching NaN. */
int shyft_hip_ts_expr(int device, size_t S, const int64_t* row, const int64_t* t, const double* v, const int64_t* t_end,
                      const int32_t* fx, size_t E, const int64_t* prog_row, const int32_t* prog, size_t n_const,
                      const double* consts, size_t n_period, const int64_t* periods, const int64_t* orow,
                      const int64_t* ot, double* out);
int shyft_hip_ts_expr_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                           const int64_t* t_end, const int32_t* fx, size_t E, const int64_t* prog_row,
                           const int32_t* prog, size_t n_const, const double* consts, size_t n_period,
                           const int64_t* periods, const int64_t* orow, const int64_t* ot, double* out);
/* HIP-event milliseconds of the kernel of the last shyft_hip_ts_expr call on this device, copies excluded, and the
 * number of such calls that launched so far. (No reference counterpart: measurement and test aid.) */
double shyft_hip_ts_expr_last_ms(int device);
uint64_t shyft_hip_ts_expr_calls(int device);

/* Forecast skill by lead time: the Nash-Sutcliffe score of P problems in one launch of kernels/forecast.hip on a device
 * (device < 0 = current). A problem is ats_vector::nash_sutcliffe(obs, t0_offset, dt, n)
 * (core/time_series_dd.cpp:1137-1145 -> core/time_series_merge.h:123-144): for each forecast in order the n slice
 * averages of the forecast and of the observation on the axis (forecast.time(0) + t0_offset, dt, n)
 * (average_accessor with USE_NAN, core/time_series.h:2033-2072), appended forecast-major, then
 * 1 - nash_sutcliffe_goal_function(observed, forecast) (core/time_series.h:2316-2344), whose two sums run sequentially
 * in that order over the pairs where both values are finite. The slice averages alone are
 * ats_vector::average_slice (time_series_dd.cpp:1147-1165). It replaces one average_accessor pass per forecast per
 * lead time on one thread. Host pointers, stateless.
 *
 * The S series are one pool in the CSR form of shyft_hip_resample (row [S+1], t and v [row[S]], t_end [S], fx [S]);
 * forecasts and observations sit together, so a lead-time table lists the same forecasts under many problems and
 * uploads their points once. Problem p names its forecasts fc_ix[fc_row[p] .. fc_row[p+1]) by index into the pool, in
 * the reference's order, and its observation obs_ix[p] (-1: none), and carries t0_offset[p], dt[p] (ticks) and n[p].
 * J is the sum over p of F_p * n[p]; job (p, k, i) lies at job_row[p] + k * n[p] + i with job_row the running sum.
 * sim and obs ([J], or NULL) receive the slice averages of forecast k and of the observation over
 * [t[row[f]] + t0_offset[p] + i * dt[p], + dt[p]): NaN when the period starts at or after the series' end, else
 * area / to_seconds(tsum), NaN without covered time; obs is NaN throughout for obs_ix == -1 or an observation without
 * points. ns ([P], or NULL) receives the score: NaN when F_p * n[p] == 0 and, by the division, without finite pairs;
 * a constant observation gives -inf or NaN. No special cases are added.
 *
 * Checked on the host before anything is launched, by both twins with the same texts: the series as for
 * shyft_hip_resample; fc_row a CSR row; every index in [0, S), or -1 for obs_ix; a forecast has at least one point
 * ("forecast_skill: a forecast has no points": the reference asks an empty axis for time(0)); n >= 0, dt > 0,
 * t0_offset >= 0 with the texts of time_series_dd.cpp:1138-1143; every slice axis inside a quarter of the int64 range;
 * a one-point observation whose point lies strictly inside a period of any forecast's axis of its problems is an
 * error, as in the reference (point_dt::time throws). A refused batch launches nothing; P == 0 or J == 0 returns 0
 * and launches nothing, after writing NaN to ns. Every operation is evaluated as written (int64 ticks, to_seconds as
 * a division, no FMA) and the sums keep the reference's order (no tree reduction), so ns, sim and obs are
 * bit-identical to shyft_hip_forecast_skill_host, which runs host/forecast.hpp on one thread and does not use
 * `device`. */
int shyft_hip_forecast_skill(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, size_t P, const int64_t* fc_row,
                             const int64_t* fc_ix, const int64_t* obs_ix, const int64_t* t0_offset, const int64_t* dt,
                             const int64_t* n, double* ns, double* sim, double* obs);
int shyft_hip_forecast_skill_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                  const int64_t* t_end, const int32_t* fx, size_t P, const int64_t* fc_row,
                                  const int64_t* fc_ix, const int64_t* obs_ix, const int64_t* t0_offset,
                                  const int64_t* dt, const int64_t* n, double* ns, double* sim, double* obs);
/* HIP-event milliseconds of the kernel of the last shyft_hip_forecast_skill on this device, copies excluded, and the
 * number of such calls that launched so far. (No reference counterpart: measurement and test aid.) */
double shyft_hip_forecast_skill_last_ms(int device);
uint64_t shyft_hip_forecast_skill_calls(int device);

/* ---- KRLS interpolation (prediction::krls_rbf_predictor, core/predictions.h:30-343, over dlib::krls;
 * krls_interpolation_ts, core/time_series_dd.h:1368-1442) ----
 * The algorithm is restated from its published form (Engel, Mannor, Meir 2004, eqs. 3.12-3.16) in host/krls.hpp;
 * last-bit parity with dlib is not pinned. A predictor's state is its dictionary d [m] of sample positions, the weights
 * alpha [m] and the dense row-major matrices Kinv and P [m][m].
 *
 * shyft_hip_krls_train_csr replaces one krls_rbf_predictor::train call (predictions.h:139-181) per series: the S series
 * in the CSR form of shyft_hip_resample, each with its own predictor parameters dt (int64 microseconds), gamma, tolerance,
 * max_dict (the predictor's size), and its own offset, count (< 0: to the end), stride, iterations and mse_tol, all [S].
 * s_row [S+1] (null: every predictor starts empty) gives the starting dictionaries s_d, s_alpha [s_row[S]] and the dense
 * starting matrices s_Kinv, s_P, one after the other (sum of m^2 doubles), so that a trained predictor is trained
 * further. One workgroup trains one series: with both matrices in LDS while the dictionary stays within
 * SHYFT_HIP_KRLS_LDS_CAPACITY entries, in a device-memory workspace up to SHYFT_HIP_KRLS_MAX_DICT, and with
 * host/krls.hpp beyond that or when the dictionary reaches max_dict (the removal of an entry is host only). *result
 * holds the trained states; read it with shyft_hip_krls_result_sizes (d_row [S+1]) and shyft_hip_krls_result_fetch
 * (d, alpha [d_row[S]]; Kinv, P [sum of m^2]; mse [S] as train returns it; path [S] SHYFT_HIP_KRLS_PATH_*) and release
 * it with shyft_hip_krls_result_free. A batch whose workspace exceeds the free device memory is refused.
 * shyft_hip_krls_train_csr_host trains every series with host/krls.hpp (path HOST); the device is bit-identical to it. */
#define SHYFT_HIP_KRLS_LDS_CAPACITY 99
#define SHYFT_HIP_KRLS_LDS_SMALL_CAPACITY 31 /* tried first: a storage small enough for eight workgroups per CU */
#define SHYFT_HIP_KRLS_MAX_DICT 1024
#define SHYFT_HIP_KRLS_PATH_LDS 1
#define SHYFT_HIP_KRLS_PATH_WORKSPACE 2
#define SHYFT_HIP_KRLS_PATH_HOST 3
typedef struct shyft_hip_krls_result shyft_hip_krls_result;
int shyft_hip_krls_train_csr(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, const int64_t* dt, const double* gamma,
                             const double* tolerance, const int64_t* max_dict, const int64_t* offset, const int64_t* count,
                             const int64_t* stride, const int64_t* iterations, const double* mse_tol, const int64_t* s_row,
                             const double* s_d, const double* s_alpha, const double* s_Kinv, const double* s_P,
                             shyft_hip_krls_result** result);
int shyft_hip_krls_train_csr_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                  const int64_t* t_end, const int32_t* fx, const int64_t* dt, const double* gamma,
                                  const double* tolerance, const int64_t* max_dict, const int64_t* offset,
                                  const int64_t* count, const int64_t* stride, const int64_t* iterations,
                                  const double* mse_tol, const int64_t* s_row, const double* s_d, const double* s_alpha,
                                  const double* s_Kinv, const double* s_P, shyft_hip_krls_result** result);
int shyft_hip_krls_result_sizes(const shyft_hip_krls_result* result, size_t S, int64_t* d_row);
int shyft_hip_krls_result_fetch(const shyft_hip_krls_result* result, size_t S, double* d, double* alpha, double* Kinv,
                                double* P, double* mse, int32_t* path);
void shyft_hip_krls_result_free(shyft_hip_krls_result* result);
/* krls_rbf_predictor::predict_vec (predictions.h:193-207) of S predictors in one launch: predictor s, given by its
 * dictionary and weights (d_row [S+1], d, alpha), dt and gamma [S], evaluated at its output times q_t[q_row[s] ..
 * q_row[s+1]) (int64 microseconds): out = sum_i alpha_i * k(x, d_i) in index order, 0.0 for an empty dictionary. With
 * q_v (one value per output time) out is the residual q_v - f(x), NaN where q_v is NaN: the terms that predictor_mse
 * (:253-282) and mse_ts (:300-334) square and sum. The _host twin evaluates the same with host/krls.hpp. */
int shyft_hip_krls_predict(int device, size_t S, const int64_t* d_row, const double* d, const double* alpha,
                           const int64_t* dt, const double* gamma, const int64_t* q_row, const int64_t* q_t,
                           const double* q_v, double* out);
int shyft_hip_krls_predict_host(int device, size_t S, const int64_t* d_row, const double* d, const double* alpha,
                                const int64_t* dt, const double* gamma, const int64_t* q_row, const int64_t* q_t,
                                const double* q_v, double* out);
/* HIP-event milliseconds of the kernels of the last shyft_hip_krls_train_csr (all its launches) or shyft_hip_krls_predict
 * on this device, copies excluded. (No reference counterpart: measurement and test aid.) */
double shyft_hip_krls_last_ms(int device);
/* SHYFT_HIP_KRLS_PATH_WORKSPACE makes shyft_hip_krls_train_csr skip the LDS storage for the process, 0 gives the
 * choice back. (Measurement aid: the two storages at equal dictionary size.) */
int shyft_hip_krls_set_path(int path);

size_t shyft_hip_number_of_catchments(const shyft_hip_region* h);
int shyft_hip_catchment_ids(const shyft_hip_region* h, int64_t* cids);

/* Deep copy of a region (cells, parameters, time axis, forcing, state, collected series) on the
 * same device: the region_model copy constructor / clone (core/region_model.h:297-301, expose.h:147),
 * used for create_opt_model_clone / create_full_model_clone. */
int shyft_hip_region_clone(const shyft_hip_region* src, shyft_hip_region** out);

/* One cell's view of a series (cell.env_ts.<var>, cell.rc.<series>, cell.sc.<field>,
 * core/cell_model.h:47-81,112-160): steps [step0, step0+n) copied to/from buf[n].
 * write != 0 is allowed for forcing only (env_ts.<var>.set(i, v)). series uses the ids above. */
int shyft_hip_cell_series(shyft_hip_region* h, int series, size_t cell, size_t step0, size_t n, double* buf, int write);
/* Many cells' views at once (the per-cell collector series of region_model::get_cells(), read in bulk): columns
 * cells[n_cells] of series `series` (ids as above), steps [step0, step0+n) of the resident window, into host
 * dst[n][n_cells]. One gather on the device (per shard for a sharded region). */
int shyft_hip_sample_cells(const shyft_hip_region* h, int series, const int64_t* cells, size_t n_cells, size_t step0,
                           size_t n, double* dst);

/* Test knobs (no reference counterpart; every knob is 0 in production). SHYFT_HIP_KNOB_PTGSK_INSTANCE: 0 = the
 * launcher picks the pt_gs_k kernel instance by region size, 2 = the 64-lane 2-wave instance, 4 = the 256-lane 4-wave
 * instance. SHYFT_HIP_KNOB_BRENT_READ_DELAY: n > 0 makes every wavefront of a 256-lane pt_gs_k workgroup except the
 * first sleep n x s_sleep(127) between the Brent phase and reading its results, so the first wavefront runs ahead
 * into the next step's job queue (the interleaving the queue's double buffering must survive). */
enum shyft_hip_knob {
    SHYFT_HIP_KNOB_PTGSK_INSTANCE = 1, SHYFT_HIP_KNOB_BRENT_READ_DELAY = 2,
    /* sharded regions: 1 = run_cells runs the shards one after another (per-shard kernel times without contention,
     * shyft_hip_shard_run_ms); 0 = concurrently (the default) */
    SHYFT_HIP_KNOB_SERIAL_SHARDS = 3,
    /* sharded regions: k >= 0 makes the next shyft_hip_region_clone of this region fail when it reaches shard k (the
     * shards before it already cloned, with their streams), so the clean-up of a partly built clone is exercised;
     * the failure is reported like any other and disarms the knob; < 0 = off (the default) */
    SHYFT_HIP_KNOB_CLONE_FAIL_AT = 4,
    /* percentiles: 0 = the launcher picks the path by segment size, 1 = LDS sort (a call with a segment of more than
     * SHYFT_HIP_PERCENTILES_LDS_MAX cells then fails), 2 = radix select */
    SHYFT_HIP_KNOB_PERCENTILES_PATH = 5
};
int shyft_hip_set_test_knob(shyft_hip_region* h, int knob, int64_t value);

/* region_model::is_cell_env_ts_ok (core/region_model.h:954-962): *ok = 1 when no forcing value of a
 * calculated cell (catchment filter) in the resident window is NaN. */
int shyft_hip_forcing_ok(const shyft_hip_region* h, int* ok);

/* ---- routing::uhg river aggregation (core/routing.h:239-421; region_model.h:909-949) ----
 * Convolution is linear, so the engine reduces the avg_discharge of all cells that share a river
 * and a unit hydrograph ("routing group") to one sum per group on the device, and convolves only
 * those sums. */

/* group_of_cell[n_cells]: the routing group of each cell, -1 = not routed (routing.id <= 0). */
int shyft_hip_set_routing_groups(shyft_hip_region* h, const int32_t* group_of_cell, size_t n_groups);
/* dst[n_groups][n]: sum over each group's cells (cell order) of avg_discharge, steps [step0, step0+n). */
int shyft_hip_routing_group_sums(const shyft_hip_region* h, size_t step0, size_t n, double* dst, int dst_on_device);
/* River network evaluation on a device (stateless; device < 0 = current): rivers are indexed 0..R-1 in
 * ascending river id. group_sums[G][T] (host or device), group_uhg[G][max_len] / group_len[G] the cell UHG
 * of each group (make_uhg_from_gamma, routing.h:399-421), group_river[G] its river, river_uhg[R][max_len] /
 * river_len[R], river_downstream[R] (index, -1 = none). Outputs [R][T]: local_inflow, upstream_inflow,
 * output_m3s (routing::model::local_inflow / upstream_inflow / output_m3s, routing.h:347-387). */
int shyft_hip_route(int device, size_t n_groups, size_t T, const double* group_sums, int src_on_device,
                    const double* group_uhg, const int32_t* group_len, const int32_t* group_river, size_t n_rivers,
                    const double* river_uhg, const int32_t* river_len, const int32_t* river_downstream, size_t max_len,
                    double* local, double* upstream, double* output, int dst_on_device);

/* ---- parameter ensembles for calibration (core/model_calibration.h:830-899) ----
 * The reference optimizer evaluates one parameter vector per region run: set parameters, revert to the
 * initial state, run_cells over the calculated catchments, sum catchment discharge, score against the
 * targets. shyft_hip_ensemble_run evaluates n_members parameter vectors in ONE launch: its lanes are
 * (calculated cell, member) pairs, member-fastest, each starting from the region's current state and
 * reading the region's forcing in place (shared, not copied). The region's own state and responses are
 * not modified. params[n_members][n_per_set] in the reference get/set order (as shyft_hip_set_parameters).
 * collect: SHYFT_HIP_COLLECT_DISCHARGE or SHYFT_HIP_COLLECT_DISCHARGE_SNOW (adds snow sca / swe).
 * Routed targets are batched too: routing.velocity / alpha / beta belong to the parameter vector, so every
 * member has its own routing groups. shyft_hip_ensemble_group_sums reduces each member's groups of the last
 * ensemble run and shyft_hip_route_members evaluates the shared river network for all members in
 * 1 + 2 x levels launches; both give, bit for bit, what shyft_hip_routing_group_sums and shyft_hip_route give
 * after a sequential run with the member's parameters. */
int shyft_hip_ensemble_run(shyft_hip_region* h, const double* params, size_t n_members, size_t n_per_set,
                           int start_step, int n_steps, int collect);
/* Sums of response `series` of the last ensemble run per member and catchment, steps [step0, step0+n)
 * inside its run range: dst[n_members][n_catchments][n], catchments in shyft_hip_catchment_ids order
 * (uncalculated catchments sum to 0). area_weighted != 0: sum of value x cell area (the area-weighted
 * snow sums of model_calibration.h:765-776). */
int shyft_hip_ensemble_sums(const shyft_hip_region* h, int series, int area_weighted, size_t step0, size_t n,
                            double* dst, int dst_on_device);
/* Milliseconds of the last ensemble launch (HIP events on its stream). */
double shyft_hip_ensemble_last_ms(const shyft_hip_region* h);
/* Routing-group discharge sums of the last ensemble run, per member. group_of[n_members][n_cells] is the member's
 * routing group of each cell, numbered from 0 within the member, -1 = the cell is not part of this evaluation;
 * group_row[n_members + 1] gives each member's first row of dst[group_row[n_members]][n] (starts at 0, does not
 * decrease). dst[group_row[m] + g][t] = sum of member m's avg_discharge over the cells of its group g, in cell
 * order, steps [step0, step0 + n) inside the run's range: bit for bit shyft_hip_routing_group_sums of the same
 * cells after a sequential run with the member's parameters (the segment sum adds by position within the segment).
 * Refused before any launch: no ensemble run; n_members different from the run's; a group index outside the
 * member's range; a cell with a group >= 0 that was not a calculated cell of the run; a sharded region (out of
 * scope: evaluate the vectors one by one there). */
int shyft_hip_ensemble_group_sums(const shyft_hip_region* h, size_t n_members, const int32_t* group_of,
                                  const int64_t* group_row, size_t step0, size_t n, double* dst, int dst_on_device);
/* p[n] doubles of device memory on the region's device, owned by the region and valid until the next call of this
 * entry or the region's destruction: where a host caller keeps shyft_hip_ensemble_group_sums' rows (dst_on_device)
 * for shyft_hip_route_members (src_on_device). Not for sharded regions. */
int shyft_hip_ensemble_scratch(shyft_hip_region* h, size_t n, double** p);
/* dst[n] (host) = the scratch rows [offset, offset + n): a host caller downloads only what it was asked for. */
int shyft_hip_ensemble_scratch_read(const shyft_hip_region* h, size_t offset, size_t n, double* dst);
/* shyft_hip_route for n_members independent sets of groups over one shared river network (stateless; device < 0 =
 * current). Member m owns the global group rows [group_row[m], group_row[m+1]) of group_sums[G][T] (host or
 * device), group_uhg[G][max_len], group_len[G] and group_river[G], G = group_row[n_members]; the river tables are
 * those of shyft_hip_route. Outputs [n_members][R][T] (host or device); local and upstream may be null when not
 * wanted. A member without groups gives zeros. The additions happen in shyft_hip_route's order, so member m's rows
 * equal shyft_hip_route of its groups bit for bit. The argument checks of shyft_hip_route, and group_row must
 * start at 0 and not decrease; all of them before the device is touched. */
int shyft_hip_route_members(int device, size_t n_members, const int64_t* group_row, size_t T, const double* group_sums,
                            int src_on_device, const double* group_uhg, const int32_t* group_len,
                            const int32_t* group_river, size_t n_rivers, const double* river_uhg,
                            const int32_t* river_len, const int32_t* river_downstream, size_t max_len, double* local,
                            double* upstream, double* output, int dst_on_device);
/* The definition of correct for shyft_hip_route_members: the literal loops on the host, in the reference's order
 * (groups ascending within a river, taps ascending, upstream rivers ascending); host pointers only. */
int shyft_hip_route_members_host(size_t n_members, const int64_t* group_row, size_t T, const double* group_sums,
                                 const double* group_uhg, const int32_t* group_len, const int32_t* group_river,
                                 size_t n_rivers, const double* river_uhg, const int32_t* river_len,
                                 const int32_t* river_downstream, size_t max_len, double* local, double* upstream,
                                 double* output);
/* Milliseconds of the kernels of the last shyft_hip_route_members on the device (HIP events). */
double shyft_hip_route_members_last_ms(int device);

/* Diagnostic: evaluate one device elementary function (0 exp, 1 log, 2 pow(x, y), 3 lgamma,
 * 4 gamma_p(x, y)) on n host inputs on the current device; out[n] host. Used by the parity
 * tests to show device math == host math bit for bit. */
int shyft_hip_math_selftest(int fn, const double* x, const double* y, size_t n, double* out);

/* Diagnostic: the device-only restatements of the hot paths (device/fastmath.h, special.h, gamma_lean.h,
 * gs_brent.h, ptssk_dev.h) on n host rows, one row per job, evaluated by test kernels that live in the kernel file
 * whose run kernel uses them (pt_gs_k: elementary functions as out-of-line detmath calls; pt_ss_k: the SGPR-table
 * calls). in[n_in_cols][n] and out[n_out_cols][n] are host arrays, column-major. Returns non-zero on an unknown
 * fn, a column count that is not the function's, a null array or a HIP error.
 *   fn                                in columns                  out columns
 *   EXPLOG_INLINE  (pt_gs_k)          x                           exp_fast(x), log_fast(x)
 *   EXPLOG_PAIRS   (pt_gs_k)          x, y                        the step loop's inline pairs: exp2(x, y).a, .b,
 *                                                                 log2p(x, y).a, .b (device/pt_dev.h kmath<true>)
 *   EXPLOG_CALLS   (pt_gs_k)          x, y                        dexp(x), dlog(x), dexp2(x, y).a, .b
 *   EXPLOG_TABLE   (pt_ss_k)          x, y                        the same functions as built there
 *   POWERS         (pt_gs_k)          x, y                        dpowr(x, y), dpow4(x), dpow8(x), dpow(x, y)
 *   GAMMA_LEAN     (pt_gs_k)          a, x                        p, p1, prefix of gs_gamma_pq_cs; ok (0 / 1) of
 *                                                                 gsb_gamma_pq at gamma_snow's policy eps
 *   BRENT          (pt_gs_k)          z1, a1, b1, a2, b2, mode    gs_corr_lwc, gs_corr_lwc_lean
 *   BRENT_SPEC4 / BRENT_SPEC2         the same                    gs_corr_lwc_spec on 4 / 2 lanes per job, then
 *                                                                 gs_corr_lwc_memo, as the small-region run kernel
 *   BRENT_OPEN4 / BRENT_OPEN2         the same                    gs_brent_job_open in groups of 4 / 2 lanes per
 *                                                                 job, as the 256-lane run kernels call it
 *   SKAUGEN        (pt_ss_k)          u, n, nu_a, alpha           ss_sca_rel_red, its error code
 *   SKAUGEN_GROUP2 / SKAUGEN_GROUP4   the same                    ss_sca_rel_red_group on 2 / 4 lanes per job
 * Brent mode 0: Q1 is not supplied (q1 = NaN, the job evaluates it); mode 1: q1 = calc_q(a1, b1, z1). */
#define SHYFT_HIP_DST_EXPLOG_INLINE 0
#define SHYFT_HIP_DST_EXPLOG_CALLS 1
#define SHYFT_HIP_DST_EXPLOG_TABLE 2
#define SHYFT_HIP_DST_POWERS 3
#define SHYFT_HIP_DST_GAMMA_LEAN 4
#define SHYFT_HIP_DST_BRENT 5
#define SHYFT_HIP_DST_BRENT_SPEC4 6
#define SHYFT_HIP_DST_BRENT_SPEC2 7
#define SHYFT_HIP_DST_SKAUGEN 8
#define SHYFT_HIP_DST_SKAUGEN_GROUP2 9
#define SHYFT_HIP_DST_SKAUGEN_GROUP4 10
#define SHYFT_HIP_DST_BRENT_OPEN4 11
#define SHYFT_HIP_DST_BRENT_OPEN2 12
#define SHYFT_HIP_DST_EXPLOG_PAIRS 13
int shyft_hip_device_selftest(int fn, const double* in, size_t n_in_cols, size_t n, double* out, size_t n_out_cols);

#ifdef __cplusplus
}
#endif
#endif /* SHYFT_HIP_H */
