// C-ABI implementation (include/shyft_hip.h): one region handle owns the
// SoA device buffers of its cells on one device and one HIP stream.
//
// Mirrors the state machine of region_model (core/region_model.h:211-1049):
// cells + parameters + time axis + cell environment (forcing) + state +
// collectors; run_cells launches one kernel over every cell of the region.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/shyft_hip.h"
#include "include_internal/host_tables.h"
#include "include_internal/kernels.h"
#include "include_internal/layout.h"
#include "include_internal/region_impl.h"
#include "include_internal/shards.h"
#include "include_internal/synth_hash.h"
#include "../../detmath/detmath.h"

using namespace shyft_hip_impl;

namespace {

// region_model::update_ix_to_id_mapping (region_model.h:236-252)
void update_ix_to_id_mapping(shyft_hip_region* h) {
    h->cid_to_cix.clear();
    h->cix_to_cid.clear();
    h->cid.resize(h->n);
    h->cix.resize(h->n);
    for (size_t i = 0; i < h->n; ++i) {
        const int64_t c = int64_t(int(h->geo[i * 11 + 4]));
        h->cid[i] = c;
        auto f = h->cid_to_cix.find(c);
        if (f == h->cid_to_cix.end()) {
            h->cid_to_cix[c] = h->cix_to_cid.size();
            h->cix[i] = h->cix_to_cid.size();
            h->cix_to_cid.push_back(c);
        } else {
            h->cix[i] = f->second;
        }
    }
    // catchment segments: cells of each catchment in cell order
    const size_t C = h->cix_to_cid.size();
    std::vector<int32_t> off, cells;
    h->seg_identity = build_csr(C, off, cells, [&](auto&& emit) {
        for (size_t i = 0; i < h->n; ++i) emit(h->cix[i], int32_t(i));
    });
    h->d_seg_cells.alloc(h->n);
    h->d_seg_off.alloc(C + 1);
    hip_check(region_copy(h, h->d_seg_cells.p, cells.data(), h->n * sizeof(int32_t), hipMemcpyHostToDevice), "upload seg");
    hip_check(region_copy(h, h->d_seg_off.p, off.data(), (C + 1) * sizeof(int32_t), hipMemcpyHostToDevice), "upload seg");
}

// a pending shyft_hip_prefetch_synthetic_forcing is dropped: its buffer has the old window's shape
void cancel_prefetch(shyft_hip_region* h) {
    if (h->gen_stream) hip_check(hipStreamSynchronize(h->gen_stream), "sync generator");
    h->gen_w0 = SIZE_MAX;
    h->free_pending = false;
    h->d_forcing_next.release();
}

// the collected rows of the window in the current collection mode, NaN until a run writes them
void alloc_collected(shyft_hip_region* h) {
    const size_t N = h->n;
    h->d_resp.alloc(h->n_series() * h->TW * N);
    hip_check(launch_fill(h->d_resp.p, h->d_resp.n, NAN, h->stream), "fill resp");
    if (h->collect_state) {
        h->d_state_series.alloc(h->n_state_series() * (h->TW + 1) * N);
        hip_check(launch_fill(h->d_state_series.p, h->d_state_series.n, NAN, h->stream), "fill state series");
    } else {
        h->d_state_series.release();
    }
    hip_check(hipStreamSynchronize(h->stream), "sync");
}

void alloc_window(shyft_hip_region* h) {
    cancel_prefetch(h);
    h->d_forcing.alloc(N_FORCING * h->TW * h->n);
    hip_check(launch_fill(h->d_forcing.p, h->d_forcing.n, NAN, h->stream), "fill forcing");
    alloc_collected(h);
}

// a handle with no device resources yet: create fills it, a sharded region keeps it as it is
std::unique_ptr<shyft_hip_region> new_handle(int stack, const stack_desc* sd, size_t n, int device) {
    std::unique_ptr<shyft_hip_region> h(new shyft_hip_region());
    h->stack = stack;
    h->sd = sd;
    h->n = n;
    h->device = device;
    return h;
}

// the run-kernel arguments every stack has, steps [b, e)
template <class A>
void fill_common(A& a, const shyft_hip_region* h, size_t b, size_t e) {
    a.n_cells = int(h->n);
    a.step0 = int(b);
    a.n_steps = int(e - b);
    a.win0 = int(h->w0);
    a.win_len = int(h->TW);
    a.collect = h->collect;
    a.params = h->d_params.p;
    a.set_ix = h->d_set_ix.p;
    a.cellc = h->d_cellc.p;
    a.state = h->d_state.p;
    // an ensemble lane region reads its parent's forcing, each lane the column of its cell
    a.forcing = h->forcing_src ? h->forcing_src->d_forcing.p : h->d_forcing.p;
    a.fcol = h->forcing_src ? h->d_fcol.p : nullptr;
    a.f_cols = int(h->forcing_src ? h->forcing_src->n : h->n);
    a.resp = h->d_resp.p;
    a.state_series = h->collect_state ? h->d_state_series.p : nullptr;
    a.active = h->active.empty() ? nullptr : h->d_active.p;
    a.err = h->d_err.p;
    a.uniform_params = h->n_sets == 1 ? 1 : 0;
}

// argument checks of region_model::run_cells (region_model.h:579-592), shared by the synchronous and the
// asynchronous entry
void check_run_args(const shyft_hip_region* h, size_t use_ncore, int start_step, int n_steps) {
    // the reference's ncore is the host's hardware_concurrency (region_model.h:280); its "reasonable minimum" of 4
    // is substituted only on the use_ncore == 0 branch (region_model.h:579-584), so with ncore == 0 any
    // use_ncore > 0 is rejected, as there
    const size_t ncore = std::thread::hardware_concurrency();
    if (use_ncore != 0 && use_ncore > 100 * ncore)
        throw std::runtime_error("illegal parameter value: use_ncore(" + std::to_string(use_ncore) +
                                 " is more than 100 time available physical cores: " + std::to_string(ncore));
    if (!(h->T > 0)) throw std::runtime_error("region_model::run with invalid time_axis invoked");
    if (start_step < 0 || size_t(start_step + 1) > h->T)
        throw std::runtime_error("region_model::run start_step must in range[0..n_steps-1>");
    if (n_steps < 0) throw std::runtime_error("region_model::run n_steps must be range[0..time-axis-steps]");
    if (size_t(start_step + n_steps) > h->T)
        throw std::runtime_error("region_model::run start_step+n_steps must be within time-axis range");
    if (!h->has_state) throw std::runtime_error("region_model::run: no state set");
}

}  // namespace

namespace shyft_hip_impl {

thread_local std::string g_last_error;
int fail(shyft_hip_region* h, const std::string& msg) {
    if (h) h->err = msg;
    g_last_error = msg;
    return 1;
}

// host <-> region copies are ordered on the region's stream (created non-blocking, so a null-stream copy would
// not wait for a run or copy_state still queued there) and complete before returning, like hipMemcpy
hipError_t region_copy(shyft_hip_region* h, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, h->stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(h->stream);
}

// derived per-set parameter rows and per-cell constants (pt_gs_k.h:347-357, gamma_snow.h:85-87, :188, :340-343;
// pt_ss_k.h:237-245, pt_hs_k.h:233-242 and hbv_stack.h:311-318 are the same expressions). Evaluated with the same
// expressions the reference evaluates, on the host. The PT stacks share the pt_gs_k PC_* rows (the rows only
// pt_gs_k fills stay 0); hbv_stack has its own, shorter HC_* rows.
void update_derived(shyft_hip_region* h) {
    if (!h->derived_dirty) return;
    if (!h->has_geo) throw std::runtime_error("region: geo_cell_data not set");
    if (!h->has_params) throw std::runtime_error("region: parameters not set");
    if (h->dt <= 0) throw std::runtime_error("region_model::run with invalid time_axis invoked");
    const stack_desc& sd = *h->sd;
    const bool ptgsk = sd.id == SHYFT_HIP_PT_GS_K;
    const size_t N = h->n;
    const size_t width = sd.param_width;
    std::vector<double> cc(size_t(sd.n_cellc) * N, 0.0);
    for (size_t i = 0; i < N; ++i) {
        const double* g = &h->geo[i * 11];
        const double* p = &h->params[size_t(h->set_ix[i]) * width];
        const double glacier = g[6], lake = g[7], reservoir = g[8];
        const double gm_direct = p[sd.k_gm_direct];
        const double rdrf = p[sd.k_rsv_drf];
        const double direct = glacier * gm_direct + reservoir * rdrf;
        if (h->hbv()) {
            cc[HC_GLACIER * N + i] = glacier;
            cc[HC_DIRECT_RESPONSE * N + i] = direct;
            cc[HC_LAND_FRACTION * N + i] = 1 - direct;
            cc[HC_GLACIER_AREA * N + i] = g[3] * glacier;
        } else {
            cc[PC_GLACIER * N + i] = glacier;
            cc[PC_SNOW_STORAGE * N + i] = 1.0 - lake - reservoir;
            cc[PC_KIRCHNER_ROUTED_PREC * N + i] = reservoir * (1.0 - rdrf) + lake;
            cc[PC_DIRECT_RESPONSE * N + i] = direct;
            cc[PC_KIRCHNER_FRACTION * N + i] = 1 - direct;
            cc[PC_GLACIER_AREA * N + i] = g[3] * glacier;
        }
        cc[sd.c_area * N + i] = g[3];
        if (ptgsk) {
            const double forest = g[9];
            const double cv = p[PK_SNOW_CV] + forest * p[PK_CV_FOREST] + g[2] * p[PK_CV_ALT];
            cc[PC_FOREST * N + i] = forest;
            cc[PC_ALTITUDE * N + i] = g[2];
            cc[PC_CV2 * N + i] = cv * cv;
            cc[PC_INV_CV2 * N + i] = 1.0 / (cv * cv);
        }
    }
    // the device rows: as given, but pt_gs_k's with the columns derived for this run's dt behind them
    std::vector<double> derived;
    if (ptgsk) {
        const double dt_s = double(h->dt) / 1e6;
        const double dt_in_days = dt_s / 86400.0;
        derived.assign(h->n_sets * PTGSK_NP, 0.0);
        for (size_t k = 0; k < h->n_sets; ++k) {
            const double* p = &h->params[k * PTGSK_NP_REF];
            double* q = &derived[k * PTGSK_NP];
            for (int j = 0; j < PTGSK_NP_REF; ++j) q[j] = p[j];
            q[PK_WED] = double(size_t(p[PK_WED]));   // size_t(p[i]) (pt_gs_k.h:103)
            q[PK_NWD] = double(size_t(p[PK_NWD]));   // implicit size_t conversion (pt_gs_k.h:109)
            q[PK_ISO] = p[PK_ISO] != 0.0 ? 1.0 : 0.0;
            const double albedo_range = p[PK_MAX_ALBEDO] - p[PK_MIN_ALBEDO];
            q[PK_ALBEDO_RANGE] = albedo_range;
            q[PK_SLOW_DECAY] = 0.5 * albedo_range * dt_in_days / p[PK_SLOW_DECAY_RATE];
            q[PK_FAST_DECAY] = detmath::pow(2.0, -dt_in_days / p[PK_FAST_DECAY_RATE]);
            q[PK_BB0] = 0.98 * 5.670373e-8 * detmath::pow(273.15, 4.0);
            q[PK_INV_CV2_PARAM] = 1.0 / (p[PK_SNOW_CV] * p[PK_SNOW_CV]);
        }
    }
    const std::vector<double>& P = ptgsk ? derived : h->params;
    h->d_params.alloc(P.size());
    h->d_cellc.alloc(cc.size());
    h->d_set_ix.alloc(N);
    hip_check(region_copy(h, h->d_params.p, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice), "upload params");
    hip_check(region_copy(h, h->d_cellc.p, cc.data(), cc.size() * sizeof(double), hipMemcpyHostToDevice), "upload cellc");
    hip_check(region_copy(h, h->d_set_ix.p, h->set_ix.data(), N * sizeof(int32_t), hipMemcpyHostToDevice), "upload set_ix");
    h->derived_dirty = false;
}

void check_window(const shyft_hip_region* h, size_t step0, size_t n, const char* what) {
    if (step0 < h->w0 || step0 + n > h->w0 + h->TW)
        throw std::runtime_error(std::string(what) + ": steps [" + std::to_string(step0) + "," + std::to_string(step0 + n) +
                                 ") outside the resident window [" + std::to_string(h->w0) + "," +
                                 std::to_string(h->w0 + h->TW) + ")");
}

void copy_rows(hipStream_t s, double* dst, const double* src, size_t bytes, int dst_dev, int src_dev) {
    hipMemcpyKind k = src_dev ? (dst_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost)
                              : (dst_dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost);
    hip_check(hipMemcpyAsync(dst, src, bytes, k, s), "hipMemcpyAsync");
    hip_check(hipStreamSynchronize(s), "sync");
}

// cell_statistics::verify_cids_exist (cell_model.h:198-211) + is_match selection
std::vector<int32_t> select_cells(const shyft_hip_region* h, const int64_t* ids, size_t n_ids, int scope) {
    std::vector<int32_t> sel;
    if (n_ids == 0) {
        sel.resize(h->n);
        for (size_t i = 0; i < h->n; ++i) sel[i] = int32_t(i);
        return sel;
    }
    if (scope == SHYFT_HIP_SCOPE_CELL_IX) {
        for (size_t k = 0; k < n_ids; ++k)
            if (ids[k] < 0 || ids[k] > int64_t(h->n))
                throw std::runtime_error("Supplied cell index reference " + std::to_string(ids[k]) +
                                         " is ouside valid range 0 .." + std::to_string(h->n));
        for (size_t i = 0; i < h->n; ++i)
            for (size_t k = 0; k < n_ids; ++k)
                if (ids[k] == int64_t(i)) { sel.push_back(int32_t(i)); break; }
    } else {
        for (size_t k = 0; k < n_ids; ++k)
            if (h->cid_to_cix.count(ids[k]) == 0)
                throw std::runtime_error("one or more supplied catchment_indexes does not exist:" + std::to_string(ids[k]));
        for (size_t i = 0; i < h->n; ++i)
            for (size_t k = 0; k < n_ids; ++k)
                if (h->cid[i] == ids[k]) { sel.push_back(int32_t(i)); break; }
    }
    return sel;
}

// device rows [step0, step0+n) of a series id (shyft_hip.h: response ids, SHYFT_HIP_SERIES_FORCING + var,
// SHYFT_HIP_SERIES_STATE + field on the T+1 state axis): the one place a window row is addressed
double* series_rows(const shyft_hip_region* h, int series, size_t step0, size_t n, const char* what) {
    // rows of `id` in a buffer that holds `len` window rows of n cells per id
    auto rows = [&](double* base, int id, size_t len) { return base + (size_t(id) * len + (step0 - h->w0)) * h->n; };
    if (series >= SHYFT_HIP_SERIES_STATE) {
        const int f = series - SHYFT_HIP_SERIES_STATE;
        if (!h->collect_state || !h->d_state_series.p)
            throw std::runtime_error(std::string(what) + ": state collection is off");
        if (size_t(f) >= h->n_state_series()) throw std::runtime_error(std::string(what) + ": invalid field");
        if (step0 < h->w0 || step0 + n > h->w0 + h->TW + 1)
            throw std::runtime_error(std::string(what) + ": steps outside the resident window");
        return rows(h->d_state_series.p, f, h->TW + 1);
    }
    check_window(h, step0, n, what);
    if (series >= SHYFT_HIP_SERIES_FORCING) {
        const int v = series - SHYFT_HIP_SERIES_FORCING;
        if (v >= N_FORCING) throw std::runtime_error(std::string(what) + ": invalid forcing variable");
        return rows(h->d_forcing.p, v, h->TW);
    }
    if (series < 0 || size_t(series) >= h->n_series())
        throw std::runtime_error(std::string(what) + ": series not collected in this collection mode");
    return rows(h->d_resp.p, series, h->TW);
}

// bayesian_kriging::parameter::temperature_gradient(period) (core/bayesian_kriging.h:220-223): the prior
// gradient from the day of year of the period's midpoint
double btk_prior_gradient(int64_t start_us, int64_t dt_us) {
    const double doy = double(day_of_year(start_us + dt_us / 2));
    return 1.18e-3 * std::sin(6.2831 / 365 * (doy + 79.0)) - 5.48e-3;
}

void launch_run(shyft_hip_region* h, int start_step, int n_steps) {
    update_derived(h);
    size_t b = n_steps > 0 ? size_t(start_step) : 0;
    size_t e = n_steps > 0 ? size_t(start_step + n_steps) : h->T;
    check_window(h, b, e - b, "run_cells");
    const double dt_s = double(h->dt) / 1e6;  // to_seconds(period.timespan())
    // the largest snow bin count of the parameter sets (the kernels with bins in registers pick their instance by it)
    int nb_max = HBV_MAX_BINS;
    if (const int kd = h->snow_dist_index(); kd >= 0) {
        nb_max = 0;
        for (size_t k = 0; k < h->n_sets; ++k) nb_max = std::max(nb_max, int(h->params[k * h->param_width() + kd]));
    }
    hip_check(hipEventRecord(h->ev0, h->stream), "hipEventRecord");
    if (h->ptssk() || h->pthsk() || h->pthpsk()) {
        ptssk_kargs a;
        fill_common(a, h, b, e);
        a.step_in_days = dt_s / 86400.0;
        a.dt_hours = dt_s / 3600.0;
        a.t1_hours = dt_s / 3600.0;
        a.dt_us = double(h->dt);
        a.nb_max = nb_max;
        if (h->pthpsk())
            hip_check(launch_pthpsk_run(a, h->stream), "pthpsk_run_kernel launch");
        else if (h->pthsk())
            hip_check(launch_pthsk_run(a, h->stream), "pthsk_run_kernel launch");
        else
            hip_check(launch_ptssk_run(a, h->stream), "ptssk_run_kernel launch");
    } else if (h->hbv()) {
        hbv_kargs a;
        fill_common(a, h, b, e);
        a.step_in_days = dt_s / 86400.0;
        a.dt_hours = dt_s / 3600.0;
        a.nb_max = nb_max;
        hip_check(launch_hbv_run(a, h->stream), "hbv_run_kernel launch");
    } else {
        ptgsk_kargs a;
        fill_common(a, h, b, e);
        a.dt_s = dt_s;
        a.dt_us = double(h->dt);
        a.t1_hours = a.dt_s / 3600.0;  // to_seconds(T1-T0)/to_seconds(deltahours(1))
        a.doy = h->d_doy.p;
        a.t_rel_year_us = h->d_trel.p;
        a.instance = h->knob_instance;
        a.read_delay = h->knob_read_delay;
        hip_check(launch_ptgsk_run(a, h->stream), "ptgsk_run_kernel launch");
    }
    hip_check(hipEventRecord(h->ev1, h->stream), "hipEventRecord");
}

void finish_run(shyft_hip_region* h) {
    hip_check(hipStreamSynchronize(h->stream), h->sd->run_kernel);
    float ms = 0.f;
    hip_check(hipEventElapsedTime(&ms, h->ev0, h->ev1), "hipEventElapsedTime");
    h->last_ms = ms;
    // the per-cell error codes stay on the device: one reduction to the lowest failing cell, 8 bytes back
    const int32_t none = INT32_MAX;
    hip_check(hipMemcpyAsync(h->d_flag.p, &none, sizeof(int32_t), hipMemcpyHostToDevice, h->stream), "upload flag");
    hip_check(launch_first_error(h->d_err.p, h->n, h->d_flag.p, h->stream), "first_error");
    int32_t first = none;
    hip_check(hipMemcpyAsync(&first, h->d_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream), "download flag");
    hip_check(hipStreamSynchronize(h->stream), "first_error");
    if (first == none) return;
    const size_t i = size_t(first);
    int32_t code = 0;
    hip_check(region_copy(h, &code, h->d_err.p + i, sizeof(int32_t), hipMemcpyDeviceToHost), "download err");
    hip_check(hipMemsetAsync(h->d_err.p, 0, h->n * sizeof(int32_t), h->stream), "memset");
    hip_check(hipStreamSynchronize(h->stream), "memset");
    if (code == ERR_NEGATIVE_OUTFLOW)
        throw std::runtime_error("Negative outflow: total_water - swe < -1e-6 in hbv_snow (cell " + std::to_string(i) + ")");
    if (code == ERR_SKAUGEN_BISECT)
        throw std::runtime_error("No change of sign in boost::math::tools::bisect, either there is no root to "
                                 "find, or there are multiple roots in the interval (skaugen sca_rel_red, cell " +
                                 std::to_string(i) + ")");
    if (code == ERR_SKAUGEN_PDF)
        throw std::runtime_error("boost::math::pdf(gamma_distribution): overflow at x = 0 (skaugen sca_rel_red, "
                                 "cell " + std::to_string(i) + ")");
    throw std::runtime_error("kirchner: Max number of iterations exceeded (500). A new step size was not found. (cell " +
                             std::to_string(i) + ")");
}

void region_set_cell_ids(shyft_hip_region* h, const int64_t* ids) {
    if (!ids) {
        h->d_cell_ids.release();
        return;
    }
    hip_check(hipSetDevice(h->device), "hipSetDevice");
    h->d_cell_ids.alloc(h->n);
    hip_check(region_copy(h, h->d_cell_ids.p, ids, h->n * sizeof(int64_t), hipMemcpyHostToDevice), "upload cell ids");
}

}  // namespace shyft_hip_impl

extern "C" {

const char* shyft_hip_last_error(const shyft_hip_region* h) { return h ? h->err.c_str() : g_last_error.c_str(); }

int shyft_hip_region_create(int stack, size_t n_cells, int device, shyft_hip_region** out) {
    if (!out) return fail(nullptr, "shyft_hip_region_create: out is null");
    *out = nullptr;
    const stack_desc* sd = stack_desc_of(stack);
    if (!sd) return fail(nullptr, "shyft_hip_region_create: unsupported method stack");
    if (n_cells == 0 || n_cells > (size_t)INT32_MAX) return fail(nullptr, "shyft_hip_region_create: invalid n_cells");
    std::unique_ptr<shyft_hip_region> h = new_handle(stack, sd, n_cells, device);
    try {
        if (device < 0) hip_check(hipGetDevice(&device), "hipGetDevice");
        h->device = device;
        hip_check(hipSetDevice(device), "hipSetDevice");
        hip_check(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking), "hipStreamCreate");
        hip_check(hipEventCreate(&h->ev0), "hipEventCreate");
        hip_check(hipEventCreate(&h->ev1), "hipEventCreate");
        hip_check(hipEventCreateWithFlags(&h->ev_copy, hipEventDisableTiming), "hipEventCreate");
        h->d_state.alloc(h->n_state_fields() * n_cells);
        h->d_err.alloc(n_cells);
        h->d_flag.alloc(1);
        hip_check(hipMemset(h->d_err.p, 0, n_cells * sizeof(int32_t)), "memset");
        h->set_ix.assign(n_cells, 0);
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
    *out = h.release();
    return 0;
}

int shyft_hip_region_create_sharded(int stack, size_t n_cells, const int* devices, size_t n_shards,
                                    shyft_hip_region** out) {
    return shyft_hip_region_create_sharded_ex(stack, n_cells, devices, n_shards, 0u, out);
}

const char* shyft_hip_region_combine_report(const shyft_hip_region* h) {
    return h && h->sh ? shards::combine_report(h->sh) : "";
}

int shyft_hip_region_create_sharded_ex(int stack, size_t n_cells, const int* devices, size_t n_shards, unsigned flags,
                                       shyft_hip_region** out) {
    if (!out) return fail(nullptr, "shyft_hip_region_create_sharded: out is null");
    *out = nullptr;
    const stack_desc* sd = stack_desc_of(stack);
    if (!sd) return fail(nullptr, "shyft_hip_region_create: unsupported method stack");
    if (n_cells == 0 || n_cells > (size_t)INT32_MAX) return fail(nullptr, "shyft_hip_region_create: invalid n_cells");
    try {
        std::unique_ptr<shyft_hip_region> h = new_handle(stack, sd, n_cells, devices && n_shards ? devices[0] : 0);
        h->sh = shard_set_create(stack, n_cells, devices, n_shards, flags);
        *out = h.release();
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

size_t shyft_hip_region_shards(const shyft_hip_region* h, size_t k, int* device, size_t* cell0, size_t* n_cells) {
    if (!h) return 0;
    if (h->sh) return shards::info(h->sh, k, device, cell0, n_cells);
    if (k == 0) {
        if (device) *device = h->device;
        if (cell0) *cell0 = 0;
        if (n_cells) *n_cells = h->n;
    }
    return 1;
}

int shyft_hip_region_combine_path(const shyft_hip_region* h) {
    return h && h->sh ? shards::combine_path(h->sh) : SHYFT_HIP_COMBINE_NONE;
}

void shyft_hip_region_destroy(shyft_hip_region* h) {
    if (!h) return;
    if (h->sh) shard_set_destroy(h->sh);
    if (h->ens) shyft_hip_region_destroy(h->ens);
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->gen_stream) (void)hipStreamSynchronize(h->gen_stream);  // a prefetch may still write d_forcing_next
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->ev_pct0) (void)hipEventDestroy(h->ev_pct0);
    if (h->ev_pct1) (void)hipEventDestroy(h->ev_pct1);
    if (h->ev_gen) (void)hipEventDestroy(h->ev_gen);
    if (h->ev_free) (void)hipEventDestroy(h->ev_free);
    if (h->gen_stream) (void)hipStreamDestroy(h->gen_stream);
    if (h->ev_copy) (void)hipEventDestroy(h->ev_copy);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

size_t shyft_hip_region_size(const shyft_hip_region* h) { return h ? h->n : 0; }

int shyft_hip_set_geo(shyft_hip_region* h, const double* geo11, const int64_t* routing_id, const double* routing_distance) {
    if (!h || !geo11) return fail(h, "shyft_hip_set_geo: null argument");
    if (h->sh) return guarded(h, [&] { shards::set_geo(h->sh, geo11, routing_id, routing_distance); });
    return guarded(h, [&] {  // routing_id / routing_distance are not kept: routing works on groups (region_routing.hip)
        for (size_t i = 0; i < h->n; ++i) {
            const double* g = geo11 + i * 11;
            // land_type_fractions::set_fractions validation (geo_cell_data.h:67-79)
            const double sum = g[6] + g[7] + g[8] + g[9];
            if (!(sum > 1.0 && sum < 1.0 + 1.0e-3) && (sum > 1.0 || g[6] < 0 || g[7] < 0 || g[8] < 0 || g[9] < 0))
                throw std::invalid_argument("LandTypeFractions:: must be >=0.0 and sum <= 1.0");
        }
        h->geo.assign(geo11, geo11 + 11 * h->n);
        for (size_t i = 0; i < h->n; ++i) {  // normalise like set_fractions
            double* g = &h->geo[i * 11];
            const double sum = g[6] + g[7] + g[8] + g[9];
            if (sum > 1.0 && sum < 1.0 + 1.0e-3)
                for (int k = 6; k < 10; ++k) g[k] /= sum;
        }
        update_ix_to_id_mapping(h);
        std::vector<double> z(h->n);
        for (size_t i = 0; i < h->n; ++i) z[i] = h->geo[i * 11 + 2];
        h->d_alt.alloc(h->n);
        hip_check(region_copy(h, h->d_alt.p, z.data(), h->n * sizeof(double), hipMemcpyHostToDevice), "upload z");
        h->has_geo = true;
        h->derived_dirty = true;
        h->dst_dirty = true;
        for (auto& t : h->idw) t.key.clear();
    });
}

int shyft_hip_set_parameters(shyft_hip_region* h, const double* params, size_t n_sets, size_t n_per_set,
                             const int32_t* set_ix) {
    if (!h || !params) return fail(h, "shyft_hip_set_parameters: null argument");
    if (h->sh) return guarded(h, [&] { shards::set_parameters(h->sh, params, n_sets, n_per_set, set_ix); });
    return guarded(h, [&] {
        const size_t width = h->param_width();
        // the reference's row, or this library's row with the snow distribution behind it
        if (n_per_set != h->n_ref_params() && !(h->snow_dist_index() >= 0 && n_per_set == width))
            throw std::runtime_error(h->sd->param_error);
        if (n_sets == 0) throw std::runtime_error("shyft_hip_set_parameters: n_sets == 0");
        std::vector<int32_t> ix(h->n, 0);
        if (set_ix) {
            for (size_t i = 0; i < h->n; ++i) {
                if (set_ix[i] < 0 || size_t(set_ix[i]) >= n_sets)
                    throw std::runtime_error("shyft_hip_set_parameters: set index out of range");
                ix[i] = set_ix[i];
            }
        }
        h->params.assign(n_sets * width, 0.0);
        for (size_t k = 0; k < n_sets; ++k) {
            double* q = &h->params[k * width];
            for (size_t j = 0; j < n_per_set; ++j) q[j] = params[k * n_per_set + j];
            const int kd = h->snow_dist_index();  // n_bins, s[HBV_MAX_BINS], intervals[HBV_MAX_BINS]
            if (kd >= 0 && n_per_set == h->n_ref_params()) {
                // hbv_snow::parameter() default distribution: s = 1 (normalised mean of ones is exactly 1),
                // quantiles 0, .25, .5, .75, 1 (hbv_snow.h:29-41)
                static const double I5[5] = {0.0, 0.25, 0.5, 0.75, 1.0};
                q[kd] = 5.0;
                for (int b = 0; b < 5; ++b) {
                    q[kd + 1 + b] = 1.0;
                    q[kd + 1 + HBV_MAX_BINS + b] = I5[b];
                }
            }
            if (kd >= 0) {
                const double nb = q[kd];
                if (!(nb >= 2.0 && nb <= double(HBV_MAX_BINS)) || nb != double(int(nb)))
                    throw std::runtime_error("hbv_snow: number of snow bins must be in [2, " +
                                             std::to_string(HBV_MAX_BINS) + "]");
            }
        }
        h->n_sets = n_sets;
        h->set_ix.swap(ix);
        h->has_params = true;
        h->derived_dirty = true;
    });
}

int shyft_hip_set_time_axis(shyft_hip_region* h, int64_t t0_us, int64_t dt_us, size_t n_steps, size_t window_steps) {
    if (!h) return fail(h, "shyft_hip_set_time_axis: null handle");
    if (h->sh) return guarded(h, [&] { shards::set_time_axis(h->sh, t0_us, dt_us, n_steps, window_steps); });
    return guarded(h, [&] {
        if (dt_us <= 0 || n_steps == 0) throw std::runtime_error("region_model::run with invalid time_axis invoked");
        if (n_steps > (size_t)INT32_MAX) throw std::runtime_error("time axis too long");
        if (!year_tables_cover(t0_us, dt_us, n_steps))
            throw std::runtime_error("set_time_axis: step times beyond +-2^62 microseconds from 1970-01-01");
        h->t0 = t0_us;
        h->dt = dt_us;
        h->T = n_steps;
        h->w0 = 0;
        h->TW = (window_steps == 0 || window_steps > n_steps) ? n_steps : window_steps;
        std::vector<int32_t> doy(n_steps);
        std::vector<int64_t> trel(n_steps);
        build_year_tables(t0_us, dt_us, n_steps, doy.data(), trel.data());
        h->d_doy.alloc(n_steps);
        h->d_trel.alloc(n_steps);
        hip_check(region_copy(h, h->d_doy.p, doy.data(), n_steps * sizeof(int32_t), hipMemcpyHostToDevice), "upload doy");
        hip_check(region_copy(h, h->d_trel.p, trel.data(), n_steps * sizeof(int64_t), hipMemcpyHostToDevice), "upload trel");
        alloc_window(h);
        h->derived_dirty = true;
    });
}

int shyft_hip_set_window(shyft_hip_region* h, size_t w0) { return shyft_hip_move_window(h, w0, 7); }

int shyft_hip_move_window(shyft_hip_region* h, size_t w0, int fill_mask) {
    if (!h) return fail(h, "shyft_hip_set_window: null handle");
    if (h->sh) return guarded(h, [&] { shards::move_window(h->sh, w0, fill_mask); });
    return guarded(h, [&] {
        if (h->T == 0) throw std::runtime_error("set_window: no time axis");
        if (w0 + h->TW > h->T) throw std::runtime_error("set_window: window beyond the time axis");
        h->w0 = w0;
        if (fill_mask & 1) hip_check(launch_fill(h->d_forcing.p, h->d_forcing.n, NAN, h->stream), "fill");
        if (fill_mask & 2) hip_check(launch_fill(h->d_resp.p, h->d_resp.n, NAN, h->stream), "fill");
        if ((fill_mask & 4) && h->d_state_series.p)
            hip_check(launch_fill(h->d_state_series.p, h->d_state_series.n, NAN, h->stream), "fill");
        hip_check(hipStreamSynchronize(h->stream), "sync");
    });
}

int shyft_hip_set_collection(shyft_hip_region* h, int collect, int collect_state) {
    if (!h) return fail(h, "shyft_hip_set_collection: null handle");
    if (h->sh) return guarded(h, [&] { shards::set_collection(h->sh, collect, collect_state); });
    return guarded(h, [&] {
        if (collect < 0 || collect > 2) throw std::runtime_error("set_collection: invalid mode");
        const bool changed = collect != h->collect || (collect_state != 0) != (h->collect_state != 0);
        h->collect = collect;
        h->collect_state = collect_state != 0;
        if (changed && h->TW) alloc_collected(h);
    });
}

int shyft_hip_set_catchment_filter(shyft_hip_region* h, const int64_t* cids, size_t n) {
    if (!h) return fail(h, "shyft_hip_set_catchment_filter: null handle");
    if (h->sh) return guarded(h, [&] { shards::set_catchment_filter(h->sh, cids, n); });
    return guarded(h, [&] {
        if (n == 0) {
            h->active.clear();
            h->d_active.release();
            return;
        }
        // region_model::set_catchment_calculation_filter (region_model.h:356-370)
        if (n > h->cix_to_cid.size())
            throw std::runtime_error("set_catchment_calculation_filter: supplied list > available catchments");
        for (size_t k = 0; k < n; ++k)
            if (h->cid_to_cix.find(cids[k]) == h->cid_to_cix.end())
                throw std::runtime_error("set_catchment_calculation_filter: no cells have supplied cid");
        std::vector<bool> cf(h->cix_to_cid.size(), false);
        for (size_t k = 0; k < n; ++k) cf[h->cid_to_cix[cids[k]]] = true;
        h->active.assign(h->n, 0);
        for (size_t i = 0; i < h->n; ++i) h->active[i] = cf[h->cix[i]] ? 1 : 0;
        h->d_active.alloc(h->n);
        hip_check(region_copy(h, h->d_active.p, h->active.data(), h->n, hipMemcpyHostToDevice), "upload filter");
    });
}

int shyft_hip_set_state(shyft_hip_region* h, const double* state, size_t n_fields) {
    if (!h || !state) return fail(h, "shyft_hip_set_state: null argument");
    if (h->sh) return guarded(h, [&] { shards::set_state(h->sh, state, n_fields); });
    return guarded(h, [&] {
        if (n_fields != h->n_state_fields()) throw std::runtime_error("set_state: wrong number of state fields");
        const size_t N = h->n;
        std::vector<double> soa(n_fields * N);
        for (size_t i = 0; i < N; ++i)
            for (size_t f = 0; f < n_fields; ++f) soa[f * N + i] = state[i * n_fields + f];
        hip_check(region_copy(h, h->d_state.p, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice), "upload state");
        h->has_state = true;
    });
}

int shyft_hip_copy_state(shyft_hip_region* dst, const shyft_hip_region* src) {
    if (!dst || !src) return fail(dst, "shyft_hip_copy_state: null argument");
    if (dst->sh || src->sh)
        return guarded(dst, [&] {
            if (!dst->sh || !src->sh) throw std::runtime_error("copy_state: one region is sharded, the other is not");
            shards::copy_state(dst->sh, src->sh);
        });
    return guarded(dst, [&] {
        if (src->stack != dst->stack || src->n != dst->n)
            throw std::runtime_error("copy_state: regions differ in method stack or number of cells");
        if (!src->has_state) throw std::runtime_error("copy_state: source region has no state");
        // ordered after everything already queued on the source stream; the copy itself runs on the
        // destination stream, so the destination's next run starts after it without a host wait
        hip_check(hipStreamSynchronize(src->stream), "copy_state: source stream");
        hip_check(hipMemcpyAsync(dst->d_state.p, src->d_state.p, dst->n_state_fields() * dst->n * sizeof(double),
                                 hipMemcpyDeviceToDevice, dst->stream), "copy_state");
        // anything later queued on the source stream (a run, set_state's upload) must not overwrite the source
        // state while the destination stream still reads it
        // (set_state / get_state copy on the region stream too, region_copy). The event lives on the source
        // region's device; a copy between two devices completes before returning instead.
        shyft_hip_region* s = const_cast<shyft_hip_region*>(src);
        if (src->device == dst->device) {
            hip_check(hipEventRecord(s->ev_copy, dst->stream), "copy_state: record");
            hip_check(hipStreamWaitEvent(s->stream, s->ev_copy, 0), "copy_state: order source stream");
        } else {
            hip_check(hipStreamSynchronize(dst->stream), "copy_state: cross-device copy");
        }
        dst->has_state = true;
    });
}

int shyft_hip_get_state(const shyft_hip_region* hc, double* state, size_t n_fields) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !state) return fail(h, "shyft_hip_get_state: null argument");
    if (h->sh) return guarded(h, [&] { shards::get_state(h->sh, state, n_fields); });
    return guarded(h, [&] {
        if (n_fields != h->n_state_fields()) throw std::runtime_error("get_state: wrong number of state fields");
        const size_t N = h->n;
        std::vector<double> soa(n_fields * N);
        hip_check(region_copy(h, soa.data(), h->d_state.p, soa.size() * sizeof(double), hipMemcpyDeviceToHost), "download state");
        for (size_t i = 0; i < N; ++i)
            for (size_t f = 0; f < n_fields; ++f) state[i * n_fields + f] = soa[f * N + i];
    });
}

int shyft_hip_set_forcing(shyft_hip_region* h, int var, size_t step0, size_t n, const double* src, int src_on_device) {
    if (!h || !src) return fail(h, "shyft_hip_set_forcing: null argument");
    if (h->sh) return guarded(h, [&] { shards::set_forcing(h->sh, var, step0, n, src, src_on_device); });
    return guarded(h, [&] {
        if (var < 0 || var >= N_FORCING) throw std::runtime_error("set_forcing: invalid variable");
        double* dst = series_rows(h, SHYFT_HIP_SERIES_FORCING + var, step0, n, "set_forcing");
        copy_rows(h->stream, dst, src, n * h->n * sizeof(double), 1, src_on_device);
    });
}

int shyft_hip_get_forcing(const shyft_hip_region* hc, int var, size_t step0, size_t n, double* dst, int dst_on_device) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !dst) return fail(h, "shyft_hip_get_forcing: null argument");
    if (h->sh) return guarded(h, [&] { shards::get_rows(h->sh, 0, var, step0, n, dst, dst_on_device); });
    return guarded(h, [&] {
        if (var < 0 || var >= N_FORCING) throw std::runtime_error("get_forcing: invalid variable");
        const double* src = series_rows(h, SHYFT_HIP_SERIES_FORCING + var, step0, n, "get_forcing");
        copy_rows(h->stream, dst, src, n * h->n * sizeof(double), dst_on_device, 1);
    });
}

int shyft_hip_synthetic_forcing(shyft_hip_region* h, uint64_t seed, uint64_t cell_offset, size_t step0, size_t n) {
    if (!h) return fail(h, "shyft_hip_synthetic_forcing: null handle");
    if (h->sh) return guarded(h, [&] { shards::synthetic_forcing(h->sh, seed, cell_offset, step0, n); });
    return guarded(h, [&] {
        check_window(h, step0, n, "synthetic_forcing");
        if (!h->has_geo) throw std::runtime_error("synthetic_forcing: geo_cell_data not set");
        const double* z = h->d_alt.p;
        hip_check(launch_synthetic_forcing(h->d_forcing.p, h->TW, step0 - h->w0, n, h->n, seed, cell_offset, step0, z,
                                           h->stream, h->d_cell_ids.p),
                  "synthetic_forcing");
        hip_check(hipStreamSynchronize(h->stream), "sync");
    });
}

int shyft_hip_prefetch_synthetic_forcing(shyft_hip_region* h, uint64_t seed, uint64_t cell_offset, size_t w0_next,
                                         int n_cus) {
    if (!h) return fail(h, "shyft_hip_prefetch_synthetic_forcing: null handle");
    if (h->sh) return guarded(h, [&] { shards::prefetch_synthetic_forcing(h->sh, seed, cell_offset, w0_next, n_cus); });
    return guarded(h, [&] {
        if (h->T == 0 || h->TW == 0) throw std::runtime_error("prefetch_synthetic_forcing: no time axis");
        if (w0_next + h->TW > h->T) throw std::runtime_error("prefetch_synthetic_forcing: window beyond the time axis");
        if (!h->has_geo) throw std::runtime_error("prefetch_synthetic_forcing: geo_cell_data not set");
        if (h->gen_w0 != SIZE_MAX) throw std::runtime_error("prefetch_synthetic_forcing: a prefetched window is pending");
        if (!h->gen_stream || h->gen_cus != n_cus) {
            if (h->gen_stream) {
                hip_check(hipStreamSynchronize(h->gen_stream), "sync");
                hip_check(hipStreamDestroy(h->gen_stream), "hipStreamDestroy");
                h->gen_stream = nullptr;
            }
            int total = 0;
            hip_check(hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, h->device), "CU count");
            if (n_cus > 0 && n_cus < total) {
                // n_cus CUs spread evenly over the device (every XCD keeps most of its CUs for the run kernel)
                std::vector<uint32_t> mask((size_t(total) + 31) / 32, 0u);
                for (int k = 0; k < n_cus; ++k) {
                    const int cu = int((long long)k * total / n_cus);
                    mask[size_t(cu) / 32] |= 1u << (cu % 32);
                }
                hip_check(hipExtStreamCreateWithCUMask(&h->gen_stream, uint32_t(mask.size()), mask.data()),
                          "hipExtStreamCreateWithCUMask");
            } else if (n_cus < 0) {
                // the whole device at the lowest stream priority: the run kernel's workgroups (normal priority,
                // launched first) are dispatched before the generator's, which fill the CUs its tail leaves idle
                int least = 0, greatest = 0;
                hip_check(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange");
                hip_check(hipStreamCreateWithPriority(&h->gen_stream, hipStreamNonBlocking, least),
                          "hipStreamCreateWithPriority");
            } else {
                hip_check(hipStreamCreateWithFlags(&h->gen_stream, hipStreamNonBlocking), "hipStreamCreate");
            }
            h->gen_cus = n_cus;
        }
        if (!h->ev_gen) hip_check(hipEventCreateWithFlags(&h->ev_gen, hipEventDisableTiming), "hipEventCreate");
        h->d_forcing_next.alloc(h->d_forcing.n);
        // the buffer was last read by a run on the region stream: the generator waits for that run -- the event the
        // last swap recorded behind it, or else everything on the region stream so far
        if (h->free_pending) {
            hip_check(hipStreamWaitEvent(h->gen_stream, h->ev_free, 0), "wait");
        } else {
            hip_check(hipEventRecord(h->ev_gen, h->stream), "record");
            hip_check(hipStreamWaitEvent(h->gen_stream, h->ev_gen, 0), "wait");
        }
        const int blocks = 4 * (n_cus > 0 ? n_cus : 256);  // 4 workgroups of 4 waves per CU (grid-stride over cells)
        hip_check(launch_synthetic_forcing_stream(h->d_forcing_next.p, h->TW, 0, h->TW, h->n, seed, cell_offset,
                                                  w0_next, h->d_alt.p, blocks, h->gen_stream, h->d_cell_ids.p),
                  "synthetic_forcing (prefetch)");
        hip_check(hipEventRecord(h->ev_gen, h->gen_stream), "record");
        h->gen_w0 = w0_next;
    });
}

int shyft_hip_swap_forcing_window(shyft_hip_region* h, size_t w0_next) {
    if (!h) return fail(h, "shyft_hip_swap_forcing_window: null handle");
    if (h->sh) return guarded(h, [&] { shards::swap_forcing_window(h->sh, w0_next); });
    return guarded(h, [&] {
        if (h->gen_w0 != w0_next) throw std::runtime_error("swap_forcing_window: no prefetched window at this step");
        if (h->d_forcing_next.n != h->d_forcing.n || w0_next + h->TW > h->T)
            throw std::runtime_error("swap_forcing_window: the prefetched window does not match the region's window");
        // the response / state-series rows still hold the previous window's values (no NaN fill, unlike
        // set_window): the run that follows the swap rewrites them, and reading them before it is the caller's
        // error (shyft_hip.h)
        // later work on the region stream (the next run) waits for the generator, without a host wait
        hip_check(hipStreamWaitEvent(h->stream, h->ev_gen, 0), "wait generator");
        // the buffer swapped out was read by the runs enqueued so far: the next prefetch into it waits for them only
        // (not for the run enqueued after this swap, which reads the other buffer)
        if (!h->ev_free) hip_check(hipEventCreateWithFlags(&h->ev_free, hipEventDisableTiming), "hipEventCreate");
        hip_check(hipEventRecord(h->ev_free, h->stream), "record");
        h->free_pending = true;
        std::swap(h->d_forcing.p, h->d_forcing_next.p);
        std::swap(h->d_forcing.n, h->d_forcing_next.n);
        h->w0 = w0_next;
        h->gen_w0 = SIZE_MAX;
    });
}

int shyft_hip_synthetic_elevation(uint64_t seed, uint64_t cell_offset, size_t n_cells, double* z_host) {
    if (!z_host) return fail(nullptr, "shyft_hip_synthetic_elevation: null argument");
    for (size_t i = 0; i < n_cells; ++i) z_host[i] = synth_elevation(seed, cell_offset + i);
    return 0;
}

int shyft_hip_run_cells(shyft_hip_region* h, size_t use_ncore, int start_step, int n_steps) {
    if (!h) return fail(h, "shyft_hip_run_cells: null handle");
    if (h->sh) return guarded(h, [&] { shards::run_cells(h->sh, use_ncore, start_step, n_steps); });
    return guarded(h, [&] {
        check_run_args(h, use_ncore, start_step, n_steps);
        launch_run(h, start_step, n_steps);
        finish_run(h);
    });
}

int shyft_hip_run_cells_async(shyft_hip_region* h, int start_step, int n_steps) {
    if (!h) return fail(h, "shyft_hip_run_cells_async: null handle");
    if (h->sh) return guarded(h, [&] { shards::run_cells_async(h->sh, start_step, n_steps); });
    return guarded(h, [&] {
        check_run_args(h, 0, start_step, n_steps);
        launch_run(h, start_step, n_steps);
    });
}

int shyft_hip_synchronize(shyft_hip_region* h) {
    if (!h) return fail(h, "shyft_hip_synchronize: null handle");
    if (h->sh) return guarded(h, [&] { shards::synchronize(h->sh); });
    return guarded(h, [&] { finish_run(h); });
}

double shyft_hip_last_run_ms(const shyft_hip_region* h) { return h ? (h->sh ? shards::last_run_ms(h->sh) : h->last_ms) : 0.0; }
double shyft_hip_last_interpolate_ms(const shyft_hip_region* h) {
    return h ? (h->sh ? shards::last_interpolate_ms(h->sh) : h->last_interp_ms) : 0.0;
}

size_t shyft_hip_shard_run_ms(const shyft_hip_region* h, double* ms, size_t n) {
    if (!h) return 0;
    if (h->sh) return shards::shard_run_ms(h->sh, ms, n);
    if (n > 0 && ms) ms[0] = h->last_ms;
    return 1;
}

int shyft_hip_last_run_kernel_ms(const shyft_hip_region* h, double* ms, int n) {
    if (!h) return 0;
    if (h->sh) return shards::last_run_kernel_ms(h->sh, ms, n);
    if (n > 0) ms[0] = h->last_ms;  // every stack runs one kernel per run_cells
    return 1;
}

int shyft_hip_region_clone(const shyft_hip_region* src, shyft_hip_region** out) {
    if (!src || !out) return fail(nullptr, "shyft_hip_region_clone: null argument");
    *out = nullptr;
    if (src->sh) {
        try {
            std::unique_ptr<shyft_hip_region> c = new_handle(src->stack, src->sd, src->n, src->device);
            c->sh = shards::clone(src->sh);
            *out = c.release();
            return 0;
        } catch (const std::exception& e) {
            return fail(nullptr, e.what());
        }
    }
    shyft_hip_region* c = nullptr;
    if (shyft_hip_region_create(src->stack, src->n, src->device, &c)) return 1;
    std::unique_ptr<shyft_hip_region, void (*)(shyft_hip_region*)> h(c, shyft_hip_region_destroy);
    const int rc = guarded(h.get(), [&] {
        hip_check(hipDeviceSynchronize(), "sync");
        // host mirrors (every member that is not a device buffer, stream or event)
        h->err.clear();
        h->geo = src->geo;
        h->cid = src->cid; h->cix = src->cix; h->cix_to_cid = src->cix_to_cid; h->cid_to_cix = src->cid_to_cix;
        h->params = src->params; h->n_sets = src->n_sets; h->set_ix = src->set_ix; h->active = src->active;
        h->t0 = src->t0; h->dt = src->dt; h->T = src->T; h->w0 = src->w0; h->TW = src->TW;
        h->collect = src->collect; h->collect_state = src->collect_state;
        h->derived_dirty = true; h->has_geo = src->has_geo; h->has_params = src->has_params; h->has_state = src->has_state;
        h->dst_dirty = true;
        clone_buf(h->d_state, src->d_state);
        clone_buf(h->d_forcing, src->d_forcing);
        clone_buf(h->d_resp, src->d_resp);
        clone_buf(h->d_state_series, src->d_state_series);
        clone_buf(h->d_doy, src->d_doy);
        clone_buf(h->d_trel, src->d_trel);
        clone_buf(h->d_seg_cells, src->d_seg_cells);
        h->seg_identity = src->seg_identity;
        clone_buf(h->d_seg_off, src->d_seg_off);
        clone_buf(h->d_active, src->d_active);
        clone_buf(h->d_alt, src->d_alt);
        clone_buf(h->d_cell_ids, src->d_cell_ids);
    });
    if (rc) {
        g_last_error = h->err;
        return rc;
    }
    *out = h.release();
    return 0;
}

int shyft_hip_set_test_knob(shyft_hip_region* h, int knob, int64_t value) {
    if (!h) return fail(h, "shyft_hip_set_test_knob: null handle");
    if (h->sh) return guarded(h, [&] { shards::set_test_knob(h->sh, knob, value); });
    return guarded(h, [&] {
        if (knob == SHYFT_HIP_KNOB_PTGSK_INSTANCE) {
            if (value != 0 && value != 2 && value != 4)
                throw std::runtime_error("set_test_knob: pt_gs_k instance must be 0 (auto), 2 or 4");
            h->knob_instance = int(value);
        } else if (knob == SHYFT_HIP_KNOB_SERIAL_SHARDS || knob == SHYFT_HIP_KNOB_CLONE_FAIL_AT) {
            throw std::runtime_error("set_test_knob: this knob needs a sharded region");
        } else if (knob == SHYFT_HIP_KNOB_BRENT_READ_DELAY) {
            if (value < 0 || value > 1000) throw std::runtime_error("set_test_knob: read delay must be in [0, 1000]");
            h->knob_read_delay = int(value);
        } else if (knob == SHYFT_HIP_KNOB_PERCENTILES_PATH) {
            if (value < 0 || value > 2)
                throw std::runtime_error("set_test_knob: percentiles path must be 0 (auto), 1 (LDS sort) or 2 (radix select)");
            h->knob_pct_path = int(value);
        } else {
            throw std::runtime_error("set_test_knob: unknown knob");
        }
    });
}

int shyft_hip_forcing_ok(const shyft_hip_region* hc, int* ok) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !ok) return fail(h, "shyft_hip_forcing_ok: null argument");
    if (h->sh) return guarded(h, [&] { shards::forcing_ok(h->sh, ok); });
    return guarded(h, [&] {
        *ok = 0;
        if (h->T == 0) throw std::runtime_error("is_cell_env_ts_ok: no time axis (initialize_cell_environment)");
        hip_check(hipMemsetAsync(h->d_flag.p, 0, sizeof(int32_t), h->stream), "memset");
        const uint8_t* active = h->active.empty() ? nullptr : h->d_active.p;
        hip_check(launch_nan_scan(h->d_forcing.p, N_FORCING * h->TW, h->n, active, h->d_flag.p, h->stream), "nan_scan");
        int32_t flag = 0;
        hip_check(hipMemcpyAsync(&flag, h->d_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream), "download");
        hip_check(hipStreamSynchronize(h->stream), "sync");
        *ok = flag ? 0 : 1;
    });
}

}  // extern "C"
