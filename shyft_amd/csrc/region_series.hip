// C-ABI implementation (include/shyft_hip.h): reading a region's series -- rows, single cells, sums over selected
// cells (cell_statistics, core/cell_model.h:198-262), sums and percentiles per catchment.
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "include_internal/kernels.h"
#include "include_internal/region_impl.h"
#include "include_internal/shards.h"

using namespace shyft_hip_impl;

namespace {

constexpr size_t PCT_WS_MAX = size_t(128) << 20;  // radix-select workspace cap: larger calls run in batches of jobs

pct_list percentile_list(const int64_t* pct, size_t n_pct) {
    if (n_pct > size_t(SHYFT_HIP_PERCENTILES_MAX))
        throw std::runtime_error("percentiles: " + std::to_string(n_pct) + " percentiles in one call, the maximum is " +
                                 std::to_string(SHYFT_HIP_PERCENTILES_MAX));
    pct_list pl{};
    pl.n = int(n_pct);
    for (size_t i = 0; i < n_pct; ++i) pl.p[i] = pct[i];
    return pl;
}

// out[n_seg][n_pct][n] on the device; max_count = the largest segment. Picks the path (SHYFT_HIP_KNOB_PERCENTILES_PATH).
void run_percentiles(shyft_hip_region* h, const double* src, size_t n, const int32_t* seg_cells, const int32_t* seg_off,
                     size_t n_seg, size_t max_count, const pct_list& pl, double* out) {
    const bool fits = max_count <= size_t(SHYFT_HIP_PERCENTILES_LDS_MAX);
    if (h->knob_pct_path == SHYFT_HIP_PERCENTILES_LDS_SORT && !fits)
        throw std::runtime_error("percentiles: the LDS sort path is forced and a segment of " + std::to_string(max_count) +
                                 " cells does not fit (at most " + std::to_string(SHYFT_HIP_PERCENTILES_LDS_MAX) + ")");
    const int path = h->knob_pct_path ? h->knob_pct_path : (fits ? SHYFT_HIP_PERCENTILES_LDS_SORT : SHYFT_HIP_PERCENTILES_RADIX);
    size_t ws = 0;
    if (path == SHYFT_HIP_PERCENTILES_RADIX) {
        const size_t per_job = percentiles_job_bytes(pl.n);
        ws = std::max(per_job, std::min(PCT_WS_MAX, n * n_seg * per_job));
        if (h->d_pct_ws.n < ws) h->d_pct_ws.alloc(ws);
        ws = h->d_pct_ws.n;
    }
    if (!h->ev_pct0) {  // events of their own: ev0 / ev1 may belong to a run still queued (run_cells_async)
        hip_check(hipEventCreate(&h->ev_pct0), "hipEventCreate");
        hip_check(hipEventCreate(&h->ev_pct1), "hipEventCreate");
    }
    hip_check(hipEventRecord(h->ev_pct0, h->stream), "hipEventRecord");
    hip_check(launch_percentiles(src, h->n, n, seg_cells, seg_off, n_seg, max_count, pl, path, h->d_pct_ws.p, ws, out,
                                 h->stream),
              "percentiles");
    hip_check(hipEventRecord(h->ev_pct1, h->stream), "hipEventRecord");
    hip_check(hipEventSynchronize(h->ev_pct1), "percentiles");
    float ms = 0.f;
    hip_check(hipEventElapsedTime(&ms, h->ev_pct0, h->ev_pct1), "hipEventElapsedTime");
    h->last_pct_ms = ms;
    h->pct_path = path;
}

// region_model::catchment_discharges (region_model.h:873-885) for any series: [catchment][n] sums over the cells of
// each catchment, value x cell area when `area`
void catchment_sums(shyft_hip_region* h, int series, size_t step0, size_t n, double* dst, int dst_on_device, bool area,
                    const char* what) {
    const double* src = series_rows(h, series, step0, n, what);
    if (area) update_derived(h);  // per-cell constants (cell area) are current
    const size_t C = h->cix_to_cid.size();
    const double* w = area ? h->d_cellc.p + size_t(h->sd->c_area) * h->n : nullptr;
    staged_rows(h, dst, C * n, dst_on_device, [&](double* out) {
        hip_check(launch_segment_sums(src, h->n, n, h->seg_identity ? nullptr : h->d_seg_cells.p, h->d_seg_off.p, C, out,
                                      h->stream, w),
                  "segment_sums");
    });
}

}  // namespace

namespace shyft_hip_impl {

int region_selected_sums(shyft_hip_region* h, int series, const int64_t* ids, size_t n_ids, int scope, int weighted,
                         size_t step0, size_t n, double* dst, double* sum_area_out, size_t* n_selected) {
    return guarded(h, [&] {
        const double* src = series_rows(h, series, step0, n, "statistics");
        std::vector<int32_t> sel = select_cells(h, ids, n_ids, scope);
        if (n_selected) *n_selected = sel.size();
        double sum_area = 0.0;
        if (sel.empty()) {
            for (size_t t = 0; t < n; ++t) dst[t] = 0.0;
            if (sum_area_out) *sum_area_out = 0.0;
            return;
        }
        h->d_sel.alloc(std::max(h->d_sel.n, sel.size()));
        hip_check(region_copy(h, h->d_sel.p, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice), "upload sel");
        const double* w = nullptr;
        if (weighted) {
            std::vector<double> a(sel.size());
            for (size_t k = 0; k < sel.size(); ++k) {
                a[k] = h->geo[size_t(sel[k]) * 11 + 3];
                sum_area += a[k];
            }
            h->d_w.alloc(std::max(h->d_w.n, a.size()));
            hip_check(region_copy(h, h->d_w.p, a.data(), a.size() * sizeof(double), hipMemcpyHostToDevice), "upload w");
            w = h->d_w.p;
        }
        staged_rows(h, dst, n, 0, [&](double* out) {
            hip_check(launch_select_sum(src, h->n, n, h->d_sel.p, sel.size(), w, out, h->stream), "select_sum");
        });
        if (sum_area_out) *sum_area_out = sum_area;
    });
}

}  // namespace shyft_hip_impl

extern "C" {

int shyft_hip_get_series(const shyft_hip_region* hc, int series, size_t step0, size_t n, double* dst, int dst_on_device) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !dst) return fail(h, "shyft_hip_get_series: null argument");
    if (h->sh) return guarded(h, [&] { shards::get_rows(h->sh, 1, series, step0, n, dst, dst_on_device); });
    return guarded(h, [&] {
        if (series >= SHYFT_HIP_SERIES_FORCING)  // response series only
            throw std::runtime_error("get_series: series not collected in this collection mode");
        const double* src = series_rows(h, series, step0, n, "get_series");
        copy_rows(h->stream, dst, src, n * h->n * sizeof(double), dst_on_device, 1);
    });
}

int shyft_hip_get_state_series(const shyft_hip_region* hc, int field, size_t step0, size_t n, double* dst,
                               int dst_on_device) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !dst) return fail(h, "shyft_hip_get_state_series: null argument");
    if (h->sh) return guarded(h, [&] { shards::get_rows(h->sh, 2, field, step0, n, dst, dst_on_device); });
    return guarded(h, [&] {
        if (field < 0 || field > INT32_MAX - SHYFT_HIP_SERIES_STATE) throw std::runtime_error("get_state_series: invalid field");
        const double* src = series_rows(h, SHYFT_HIP_SERIES_STATE + field, step0, n, "get_state_series");
        copy_rows(h->stream, dst, src, n * h->n * sizeof(double), dst_on_device, 1);
    });
}

int shyft_hip_cell_series(shyft_hip_region* h, int series, size_t cell, size_t step0, size_t n, double* buf, int write) {
    if (!h || !buf) return fail(h, "shyft_hip_cell_series: null argument");
    if (h->sh) return guarded(h, [&] { shards::cell_series(h->sh, series, cell, step0, n, buf, write); });
    return guarded(h, [&] {
        if (cell >= h->n) throw std::runtime_error("cell_series: cell index out of range");
        if (write && series < SHYFT_HIP_SERIES_FORCING)
            throw std::runtime_error("cell_series: only forcing (cell env_ts) is writable");
        double* p = series_rows(h, series, step0, n, "cell_series") + cell;
        const size_t pitch = h->n * sizeof(double);
        if (write)
            hip_check(hipMemcpy2DAsync(p, pitch, buf, sizeof(double), sizeof(double), n, hipMemcpyHostToDevice, h->stream),
                      "cell_series write");
        else
            hip_check(hipMemcpy2DAsync(buf, sizeof(double), p, pitch, sizeof(double), n, hipMemcpyDeviceToHost, h->stream),
                      "cell_series read");
        hip_check(hipStreamSynchronize(h->stream), "sync");
    });
}

int shyft_hip_sample_cells(const shyft_hip_region* hc, int series, const int64_t* cells, size_t n_cells, size_t step0,
                           size_t n, double* dst) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || (n_cells && (!cells || !dst))) return fail(h, "shyft_hip_sample_cells: null argument");
    if (n_cells == 0 || n == 0) return 0;
    if (h->sh) return guarded(h, [&] { shards::sample_cells(h->sh, series, cells, n_cells, step0, n, dst); });
    return guarded(h, [&] {
        const double* rows = series_rows(h, series, step0, n, "sample_cells");
        std::vector<int32_t> idx(n_cells);
        for (size_t j = 0; j < n_cells; ++j) {
            if (cells[j] < 0 || size_t(cells[j]) >= h->n) throw std::runtime_error("sample_cells: cell index out of range");
            idx[j] = int32_t(cells[j]);
        }
        h->d_sel.alloc(std::max(h->d_sel.n, n_cells));
        hip_check(region_copy(h, h->d_sel.p, idx.data(), n_cells * sizeof(int32_t), hipMemcpyHostToDevice), "upload cells");
        staged_rows(h, dst, n * n_cells, 0, [&](double* out) {
            hip_check(launch_gather_columns(out, rows, n, h->n, h->d_sel.p, n_cells, h->stream), "gather_columns");
        });
    });
}

int shyft_hip_statistics(const shyft_hip_region* hc, int series, const int64_t* ids, size_t n_ids, int scope, int weighted,
                         size_t step0, size_t n, double* dst) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !dst) return fail(h, "shyft_hip_statistics: null argument");
    if (h->sh) return guarded(h, [&] { shards::statistics(h->sh, series, ids, n_ids, scope, weighted, step0, n, dst); });
    double sum_area = 0.0;
    size_t n_sel = 0;
    const int rc = region_selected_sums(h, series, ids, n_ids, scope, weighted, step0, n, dst, &sum_area, &n_sel);
    if (rc || !weighted) return rc;
    if (n_sel == 0) {  // no match: sum -> empty ts in the reference (0 here); average -> nan
        for (size_t t = 0; t < n; ++t) dst[t] = NAN;
        return 0;
    }
    const double s = 1 / sum_area;  // scale_by(1/sum_area) (cell_model.h:252)
    for (size_t t = 0; t < n; ++t) dst[t] *= s;
    return 0;
}

int shyft_hip_catchment_sums(const shyft_hip_region* hc, int series, size_t step0, size_t n, double* dst,
                             int dst_on_device) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !dst) return fail(h, "shyft_hip_catchment_sums: null argument");
    if (h->sh) return guarded(h, [&] { shards::catchment_sums(h->sh, series, step0, n, dst, dst_on_device, false); });
    return guarded(h, [&] { catchment_sums(h, series, step0, n, dst, dst_on_device, false, "catchment_sums"); });
}

int shyft_hip_catchment_area_sums(const shyft_hip_region* hc, int series, size_t step0, size_t n, double* dst,
                                  int dst_on_device) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !dst) return fail(h, "shyft_hip_catchment_area_sums: null argument");
    if (h->sh) return guarded(h, [&] { shards::catchment_sums(h->sh, series, step0, n, dst, dst_on_device, true); });
    return guarded(h, [&] { catchment_sums(h, series, step0, n, dst, dst_on_device, true, "catchment_area_sums"); });
}

int shyft_hip_percentiles(const shyft_hip_region* hc, int series, const int64_t* ids, size_t n_ids, int scope,
                          const int64_t* pct, size_t n_pct, size_t step0, size_t n, double* dst) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h) return fail(h, "shyft_hip_percentiles: null argument");
    if (h->sh) return fail(h, "percentiles: not available for a sharded region");
    if (n_pct == 0) return 0;
    if (!pct || !dst) return fail(h, "shyft_hip_percentiles: null argument");
    return guarded(h, [&] {
        const pct_list pl = percentile_list(pct, n_pct);
        const double* src = series_rows(h, series, step0, n, "percentiles");
        std::vector<int32_t> sel = select_cells(h, ids, n_ids, scope);
        h->pct_path = SHYFT_HIP_PERCENTILES_NONE;
        if (n == 0) return;
        if (sel.empty()) {
            for (size_t i = 0; i < n_pct * n; ++i) dst[i] = NAN;
            return;
        }
        bool identity = sel.size() == h->n;  // all cells in cell order: the index array is not read
        for (size_t i = 0; i < sel.size() && identity; ++i) identity = sel[i] == int32_t(i);
        if (!identity) {
            h->d_sel.alloc(std::max(h->d_sel.n, sel.size()));
            hip_check(region_copy(h, h->d_sel.p, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice), "upload sel");
        }
        const int32_t off[2] = {0, int32_t(sel.size())};
        h->d_pct_off.alloc(2);
        hip_check(region_copy(h, h->d_pct_off.p, off, sizeof(off), hipMemcpyHostToDevice), "upload segment");
        staged_rows(h, dst, n_pct * n, 0, [&](double* out) {
            run_percentiles(h, src, n, identity ? nullptr : h->d_sel.p, h->d_pct_off.p, 1, sel.size(), pl, out);
        });
    });
}

int shyft_hip_catchment_percentiles(const shyft_hip_region* hc, int series, const int64_t* pct, size_t n_pct,
                                    size_t step0, size_t n, double* dst, int dst_on_device) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h) return fail(h, "shyft_hip_catchment_percentiles: null argument");
    if (h->sh) return fail(h, "percentiles: not available for a sharded region");
    if (n_pct == 0) return 0;
    if (!pct || !dst) return fail(h, "shyft_hip_catchment_percentiles: null argument");
    return guarded(h, [&] {
        const pct_list pl = percentile_list(pct, n_pct);
        const double* src = series_rows(h, series, step0, n, "catchment_percentiles");
        const size_t C = h->cix_to_cid.size();
        h->pct_path = SHYFT_HIP_PERCENTILES_NONE;
        if (n == 0 || C == 0) return;
        std::vector<size_t> count(C, 0);
        for (size_t i = 0; i < h->n; ++i) ++count[h->cix[i]];
        const size_t max_count = *std::max_element(count.begin(), count.end());
        staged_rows(h, dst, C * n_pct * n, dst_on_device, [&](double* out) {
            run_percentiles(h, src, n, h->seg_identity ? nullptr : h->d_seg_cells.p, h->d_seg_off.p, C, max_count, pl, out);
        });
    });
}

int shyft_hip_percentiles_host(const double* rows, size_t n_steps, size_t n_samples_per_step, const int64_t* pct,
                               size_t n_pct, double* dst) {
    if (n_pct == 0 || n_steps == 0) return 0;
    if (!pct || !dst || (!rows && n_samples_per_step)) return fail(nullptr, "shyft_hip_percentiles_host: null argument");
    try {
        percentiles_host(rows, n_steps, n_samples_per_step, pct, n_pct, dst);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_percentiles_path(const shyft_hip_region* h) {
    if (!h) return -1;
    return h->pct_path;
}

double shyft_hip_last_percentiles_ms(const shyft_hip_region* h) { return h ? h->last_pct_ms : 0.0; }

size_t shyft_hip_number_of_catchments(const shyft_hip_region* h) {
    return h ? (h->sh ? shards::number_of_catchments(h->sh) : h->cix_to_cid.size()) : 0;
}

int shyft_hip_catchment_ids(const shyft_hip_region* h, int64_t* cids) {
    if (!h || !cids) return fail(const_cast<shyft_hip_region*>(h), "shyft_hip_catchment_ids: null argument");
    if (h->sh) {
        shards::catchment_ids(h->sh, cids);
        return 0;
    }
    for (size_t c = 0; c < h->cix_to_cid.size(); ++c) cids[c] = h->cix_to_cid[c];
    return 0;
}

}  // extern "C"
