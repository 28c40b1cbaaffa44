// Internal: the region handle behind the C ABI (include/shyft_hip.h), shared by region.hip and the region_*.hip
// files (one region on one device) and shards.hip (a region whose cells are split over several regions / devices).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/shyft_hip.h"
#include "kernels.h"
#include "layout.h"
#include "stack_desc.h"

namespace shyft_hip_impl {

extern thread_local std::string g_last_error;  // region.hip

struct hip_error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw hip_error(std::string(what) + ": " + hipGetErrorString(e));
}

template <class T>
struct dbuf {
    T* p = nullptr;
    size_t n = 0;
    dbuf() = default;
    dbuf(const dbuf&) = delete;
    dbuf& operator=(const dbuf&) = delete;
    ~dbuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void alloc(size_t count) {
        if (count == n && p) return;
        release();
        if (count == 0) return;
        hip_check(hipMalloc(&p, count * sizeof(T)), "hipMalloc");
        n = count;
    }
};

struct shard_set;  // shards.hip: the shards of a sharded region

}  // namespace shyft_hip_impl

using shyft_hip_impl::dbuf;

struct shyft_hip_region {
    // a sharded region (shyft_hip_region_create_sharded) owns its shards here and no device buffers of its own;
    // every entry point forwards to shards.hip
    shyft_hip_impl::shard_set* sh = nullptr;
    int stack = 0;
    const stack_desc* sd = nullptr;  // the stack's row of STACK_TABLE, set with `stack` at create and clone
    size_t n = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_copy = nullptr;  // shyft_hip_copy_state: the copy out of this region's state has finished
    std::string err;
    double last_ms = 0.0;
    double last_interp_ms = 0.0;  // the last interpolate's gather kernel
    int knob_instance = 0, knob_read_delay = 0;  // shyft_hip_set_test_knob (pt_gs_k launches)
    int knob_pct_path = 0;                       // SHYFT_HIP_KNOB_PERCENTILES_PATH
    int pct_path = SHYFT_HIP_PERCENTILES_NONE;   // the path of the last percentile call
    double last_pct_ms = 0.0;                    // its kernels, first launch to last (HIP events on the stream)
    hipEvent_t ev_pct0 = nullptr, ev_pct1 = nullptr;

    // host mirrors
    std::vector<double> geo;  // n x 11
    std::vector<int64_t> cid;          // per cell
    std::vector<size_t> cix;           // per cell
    std::vector<int64_t> cix_to_cid;   // region_model::cix_to_cid
    std::map<int64_t, size_t> cid_to_cix;
    std::vector<double> params;        // n_sets x param_width()
    size_t n_sets = 0;
    std::vector<int32_t> set_ix;
    std::vector<uint8_t> active;       // empty = no filter
    int64_t t0 = 0, dt = 0;
    size_t T = 0, w0 = 0, TW = 0;
    int collect = COLLECT_DISCHARGE;
    int collect_state = 0;
    bool derived_dirty = true;
    bool has_geo = false, has_params = false, has_state = false;

    // device
    dbuf<double> d_params, d_cellc, d_state, d_forcing, d_resp, d_state_series;
    // double-buffered forcing window (shyft_hip_prefetch_synthetic_forcing / shyft_hip_swap_forcing_window): the
    // next window is generated on gen_stream (restricted to a few CUs) while the current one runs
    dbuf<double> d_forcing_next;
    hipStream_t gen_stream = nullptr;
    int gen_cus = -1;
    hipEvent_t ev_gen = nullptr;
    hipEvent_t ev_free = nullptr;  // recorded at the last swap: the swapped-out buffer's last reader has finished
    bool free_pending = false;
    size_t gen_w0 = SIZE_MAX;
    dbuf<int32_t> d_set_ix, d_err, d_doy, d_seg_cells, d_seg_off, d_sel;
    dbuf<int64_t> d_trel;
    dbuf<uint8_t> d_active;
    dbuf<double> d_tmp, d_w, d_alt;
    dbuf<int64_t> d_cell_ids;  // a z-balanced shard: the region cell of each of its cells (synthetic forcing keys)
    dbuf<int32_t> d_flag;
    dbuf<int32_t> d_pct_off;       // percentiles of one selection: its segment table {0, n_selected}
    dbuf<unsigned char> d_pct_ws;  // radix-select jobs and histograms (kernels/percentiles.hip)

    // inverse-distance neighbour tables, one per forcing variable, cached by
    // (model, parameters, source geometry)
    struct idw_table {
        std::vector<double> key;
        dbuf<int32_t> idx, cnt;
        dbuf<double> w, aux;
        dbuf<int32_t> wu, wn, ovf;  // wavefront unions of the neighbour lists (idw_wave_union)
        dbuf<uint32_t> lidx;
        bool wave_ok = false;
        int K = 0;
        int last_path = SHYFT_HIP_IDW_NONE;  // the gather the last interpolate of this variable ran
    } idw[N_FORCING];
    dbuf<double> d_dst_xyz, d_slope, d_src_xyz, d_src_vals;
    bool dst_dirty = true;
    // Bayesian temperature kriging destinations (calculated cells) and their window columns
    dbuf<double> d_btk_xyz;
    dbuf<int32_t> d_btk_index;
    std::vector<double> btk_xyz_host;
    std::vector<int32_t> btk_index_host;
    uint64_t btk_dst_version = 0;
    std::unique_ptr<btk_cache, void (*)(btk_cache*)> btk{nullptr, btk_cache_destroy};

    // routing groups (cells sharing river + UHG): segment tables for the group discharge sums
    dbuf<int32_t> d_rseg_cells, d_rseg_off;
    // the catchment / routing-group segments are the identity permutation of the cells (contiguous ranges in cell
    // order): the segment sums do not read the index arrays
    bool seg_identity = false, rseg_identity = false;
    size_t n_route_groups = 0;

    // parameter ensemble (calibration): a lane region of calculated cells x members that reads this
    // region's forcing through d_fcol (see shyft_hip_ensemble_run)
    shyft_hip_region* ens = nullptr;
    const shyft_hip_region* forcing_src = nullptr;  // set on an ensemble lane region: whose forcing it reads
    dbuf<int32_t> d_fcol;                            // [lanes] forcing column (cell of the parent region)
    size_t ens_members = 0, ens_groups = 0, ens_b = 0, ens_e = 0;
    std::vector<int32_t> ens_k_of_cell;  // [n] the cell's rank among the calculated cells of the last ensemble run, -1 = none
    dbuf<double> d_ens_scratch;          // shyft_hip_ensemble_scratch: the caller's device rows between two ensemble entries

    bool hbv() const { return stack == SHYFT_HIP_HBV_STACK; }
    bool ptssk() const { return stack == SHYFT_HIP_PT_SS_K; }
    bool pthsk() const { return stack == SHYFT_HIP_PT_HS_K; }
    bool pthpsk() const { return stack == SHYFT_HIP_PT_HPS_K; }
    size_t n_series() const {
        if (collect == COLLECT_ALL) return sd->n_full_series;
        return collect == COLLECT_DISCHARGE_SNOW ? 4 : 2;
    }
    size_t n_state_fields() const { return sd->n_state_fields; }
    size_t n_state_series() const { return sd->n_state_series; }
    size_t n_ref_params() const { return sd->n_ref_params; }
    size_t param_width() const { return sd->param_width; }
    int snow_dist_index() const { return sd->snow_dist_index; }
};

namespace shyft_hip_impl {

int fail(shyft_hip_region* h, const std::string& msg);

template <class F>
inline int guarded(shyft_hip_region* h, F&& f) {
    try {
        if (h) hip_check(hipSetDevice(h->device), "hipSetDevice");
        f();
        return 0;
    } catch (const std::exception& e) {
        return fail(h, e.what());
    } catch (...) {
        return fail(h, "unknown error");
    }
}

// ---- helpers of the region entries, defined in region.hip and shared by the region_*.hip files
hipError_t region_copy(shyft_hip_region* h, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
void copy_rows(hipStream_t s, double* dst, const double* src, size_t bytes, int dst_dev, int src_dev);
void check_window(const shyft_hip_region* h, size_t step0, size_t n, const char* what);
double* series_rows(const shyft_hip_region* h, int series, size_t step0, size_t n, const char* what);
std::vector<int32_t> select_cells(const shyft_hip_region* h, const int64_t* ids, size_t n_ids, int scope);
void update_derived(shyft_hip_region* h);
void launch_run(shyft_hip_region* h, int start_step, int n_steps);
void finish_run(shyft_hip_region* h);
double btk_prior_gradient(int64_t start_us, int64_t dt_us);

template <class T>
void clone_buf(dbuf<T>& dst, const dbuf<T>& src) {
    dst.release();
    if (!src.p) return;
    dst.alloc(src.n);
    hip_check(hipMemcpy(dst.p, src.p, src.n * sizeof(T), hipMemcpyDeviceToDevice), "clone");
}

// A result of `count` doubles for `dst`: launch(out) writes them to the device, to dst itself when that is on the
// device and else to h->d_tmp, grown to hold them. They are then copied to the host, or h's stream is waited for.
template <class F>
void staged_rows(shyft_hip_region* h, double* dst, size_t count, int dst_on_device, F&& launch) {
    double* out = dst;
    if (!dst_on_device) {
        h->d_tmp.alloc(std::max(h->d_tmp.n, count));
        out = h->d_tmp.p;
    }
    launch(out);
    if (!dst_on_device) copy_rows(h->stream, dst, out, count * sizeof(double), 0, 1);
    else hip_check(hipStreamSynchronize(h->stream), "sync");
}

}  // namespace shyft_hip_impl
