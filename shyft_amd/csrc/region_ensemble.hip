// C-ABI implementation (include/shyft_hip.h): parameter ensembles (core/model_calibration.h:830-899) -- a lane region
// of calculated cells x members next to the region, and the sums over its lanes.
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "include_internal/host_tables.h"
#include "include_internal/kernels.h"
#include "include_internal/region_impl.h"
#include "include_internal/shards.h"

using namespace shyft_hip_impl;

extern "C" {

int shyft_hip_ensemble_run(shyft_hip_region* h, const double* params, size_t n_members, size_t n_per_set,
                           int start_step, int n_steps, int collect) {
    if (!h || !params) return fail(h, "shyft_hip_ensemble_run: null argument");
    if (h->sh) return guarded(h, [&] { shards::ensemble_run(h->sh, params, n_members, n_per_set, start_step, n_steps, collect); });
    return guarded(h, [&] {
        if (n_members == 0) throw std::runtime_error("ensemble_run: n_members must be > 0");
        if (collect != COLLECT_DISCHARGE && collect != COLLECT_DISCHARGE_SNOW)
            throw std::runtime_error("ensemble_run: collect must be discharge or discharge+snow");
        if (!h->has_geo) throw std::runtime_error("region: geo_cell_data not set");
        if (!h->has_state) throw std::runtime_error("region_model::run: no state set");
        if (!(h->T > 0)) throw std::runtime_error("region_model::run with invalid time_axis invoked");
        if (start_step < 0 || n_steps < 0 || size_t(start_step) + size_t(n_steps) > h->T)
            throw std::runtime_error("ensemble_run: steps outside the time axis");
        const size_t b = n_steps > 0 ? size_t(start_step) : 0;
        const size_t e = n_steps > 0 ? size_t(start_step + n_steps) : h->T;
        check_window(h, b, e - b, "ensemble_run");
        // calculated cells (catchment filter), cell order
        std::vector<int32_t> cells;
        for (size_t i = 0; i < h->n; ++i)
            if (h->active.empty() || h->active[i]) cells.push_back(int32_t(i));
        if (cells.empty()) throw std::runtime_error("ensemble_run: no calculated cells");
        const size_t P = n_members, K = cells.size(), L = K * P;
        if (L > size_t(INT32_MAX)) throw std::runtime_error("ensemble_run: cells x members exceeds 2^31 lanes");
        hip_check(hipStreamSynchronize(h->stream), "sync");  // forcing/state writes of the region are complete

        if (h->ens && (h->ens->n != L || h->ens->stack != h->stack)) {
            shyft_hip_region_destroy(h->ens);
            h->ens = nullptr;
        }
        if (!h->ens && shyft_hip_region_create(h->stack, L, h->device, &h->ens)) throw std::runtime_error(g_last_error);
        shyft_hip_region* x = h->ens;
        x->forcing_src = h;
        x->geo.resize(L * 11);
        std::vector<int32_t> fcol(L), lane_set(L);
        for (size_t k = 0; k < K; ++k)
            for (size_t m = 0; m < P; ++m) {
                const size_t l = k * P + m;
                fcol[l] = cells[k];
                std::copy(h->geo.begin() + size_t(cells[k]) * 11, h->geo.begin() + size_t(cells[k]) * 11 + 11,
                          x->geo.begin() + l * 11);
                lane_set[l] = int32_t(m);
            }
        if (shyft_hip_set_parameters(x, params, P, n_per_set, lane_set.data())) throw std::runtime_error(x->err);
        x->active.clear();
        x->t0 = h->t0; x->dt = h->dt; x->T = h->T; x->w0 = h->w0; x->TW = h->TW;
        x->collect = collect;
        x->collect_state = 0;
        x->has_geo = x->has_params = x->has_state = true;
        x->derived_dirty = true;
        update_derived(x);  // per-member parameter rows and per-lane constants
        x->d_fcol.alloc(L);
        hip_check(hipMemcpy(x->d_fcol.p, fcol.data(), L * sizeof(int32_t), hipMemcpyHostToDevice), "upload fcol");
        clone_buf(x->d_doy, h->d_doy);
        clone_buf(x->d_trel, h->d_trel);
        // every member starts from the region's current state
        hip_check(launch_gather_columns(x->d_state.p, h->d_state.p, h->n_state_fields(), h->n, x->d_fcol.p, L, x->stream),
                  "gather state");
        x->d_resp.alloc(x->n_series() * x->TW * L);
        x->d_state_series.release();
        // (member, catchment) segments, lanes in cell order: group m*C + cix
        const size_t C = h->cix_to_cid.size();
        std::vector<int32_t> off, seg;
        build_csr(P * C, off, seg, [&](auto&& emit) {
            for (size_t k = 0; k < K; ++k)
                for (size_t m = 0; m < P; ++m) emit(m * C + h->cix[size_t(cells[k])], int32_t(k * P + m));
        });
        x->d_seg_off.alloc(off.size());
        x->d_seg_cells.alloc(L);
        hip_check(hipMemcpy(x->d_seg_off.p, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice), "upload");
        hip_check(hipMemcpy(x->d_seg_cells.p, seg.data(), L * sizeof(int32_t), hipMemcpyHostToDevice), "upload");
        x->ens_groups = P * C;
        h->ens_members = P;
        h->ens_b = b;
        h->ens_e = e;
        h->ens_k_of_cell.assign(h->n, -1);
        for (size_t k = 0; k < K; ++k) h->ens_k_of_cell[size_t(cells[k])] = int32_t(k);
        launch_run(x, int(b), int(e - b));
        finish_run(x);
    });
}

int shyft_hip_ensemble_sums(const shyft_hip_region* hc, int series, int area_weighted, size_t step0, size_t n,
                            double* dst, int dst_on_device) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !dst) return fail(h, "shyft_hip_ensemble_sums: null argument");
    if (h->sh) return guarded(h, [&] { shards::ensemble_sums(h->sh, series, area_weighted, step0, n, dst, dst_on_device); });
    return guarded(h, [&] {
        shyft_hip_region* x = h->ens;
        if (!x || h->ens_members == 0) throw std::runtime_error("ensemble_sums: no ensemble run");
        if (series < 0 || size_t(series) >= x->n_series())
            throw std::runtime_error("ensemble_sums: series not collected by the ensemble run");
        if (step0 < h->ens_b || step0 + n > h->ens_e)
            throw std::runtime_error("ensemble_sums: steps outside the last ensemble run");
        const size_t L = x->n, G = x->ens_groups;
        const double* src = series_rows(x, series, step0, n, "ensemble_sums");
        const double* w = nullptr;
        if (area_weighted) w = x->d_cellc.p + size_t(x->sd->c_area) * L;
        staged_rows(x, dst, G * n, dst_on_device, [&](double* out) {
            hip_check(launch_segment_sums(src, L, n, x->d_seg_cells.p, x->d_seg_off.p, G, out, x->stream, w), "ensemble sums");
        });
    });
}

int shyft_hip_ensemble_group_sums(const shyft_hip_region* hc, size_t n_members, const int32_t* group_of,
                                  const int64_t* group_row, size_t step0, size_t n, double* dst, int dst_on_device) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !group_of || !group_row) return fail(h, "shyft_hip_ensemble_group_sums: null argument");
    if (h->sh)
        return fail(h, "ensemble_group_sums: sharded regions are out of scope (route each vector with "
                       "shyft_hip_routing_group_sums instead)");
    return guarded(h, [&] {
        shyft_hip_region* x = h->ens;
        if (!x || h->ens_members == 0) throw std::runtime_error("ensemble_group_sums: no ensemble run");
        const size_t P = h->ens_members, N = h->n, L = x->n;
        if (n_members != P)
            throw std::runtime_error("ensemble_group_sums: n_members differs from the last ensemble run's " + std::to_string(P));
        if (step0 < h->ens_b || step0 + n > h->ens_e)
            throw std::runtime_error("ensemble_group_sums: steps outside the last ensemble run");
        if (group_row[0] != 0) throw std::runtime_error("ensemble_group_sums: group_row must start at 0");
        for (size_t m = 0; m < P; ++m)
            if (group_row[m + 1] < group_row[m]) throw std::runtime_error("ensemble_group_sums: group_row must not decrease");
        const size_t G = size_t(group_row[P]);
        // one segment per (member, group): its lanes k * P + m in cell order; n_lanes <= P * K = L <= INT32_MAX
        std::vector<int32_t> off, lanes;
        build_csr(G, off, lanes, [&](auto&& emit) {
            for (size_t m = 0; m < P; ++m) {
                const int64_t Gm = group_row[m + 1] - group_row[m];
                for (size_t i = 0; i < N; ++i) {
                    const int32_t g = group_of[m * N + i];
                    if (g == -1) continue;
                    if (g < -1 || int64_t(g) >= Gm) throw std::runtime_error("ensemble_group_sums: group index out of range");
                    if (h->ens_k_of_cell[i] < 0)
                        throw std::runtime_error("ensemble_group_sums: cell " + std::to_string(i) +
                                                 " has a group but was not a calculated cell of the ensemble run");
                    emit(size_t(group_row[m] + g), int32_t(size_t(h->ens_k_of_cell[i]) * P + m));
                }
            }
        });
        if (G == 0 || n == 0) return;
        if (!dst) throw std::runtime_error("ensemble_group_sums: dst is null");
        if (lanes.empty()) lanes.push_back(0);  // a segment table of no lanes still has a device row
        x->d_rseg_off.alloc(off.size());
        x->d_rseg_cells.alloc(lanes.size());
        hip_check(hipMemcpy(x->d_rseg_off.p, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice), "upload");
        hip_check(hipMemcpy(x->d_rseg_cells.p, lanes.data(), lanes.size() * sizeof(int32_t), hipMemcpyHostToDevice), "upload");
        const double* src = series_rows(x, SHYFT_HIP_AVG_DISCHARGE, step0, n, "ensemble_group_sums");
        staged_rows(x, dst, G * n, dst_on_device, [&](double* out) {
            hip_check(launch_segment_sums(src, L, n, x->d_rseg_cells.p, x->d_rseg_off.p, G, out, x->stream),
                      "ensemble group sums");
        });
    });
}

int shyft_hip_ensemble_scratch(shyft_hip_region* h, size_t n, double** p) {
    if (!h || !p) return fail(h, "shyft_hip_ensemble_scratch: null argument");
    if (h->sh) return fail(h, "ensemble_scratch: sharded regions are out of scope");
    return guarded(h, [&] {
        if (h->d_ens_scratch.n < n) h->d_ens_scratch.alloc(n);
        *p = h->d_ens_scratch.p;
    });
}

int shyft_hip_ensemble_scratch_read(const shyft_hip_region* hc, size_t offset, size_t n, double* dst) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !dst) return fail(h, "shyft_hip_ensemble_scratch_read: null argument");
    return guarded(h, [&] {
        if (offset > h->d_ens_scratch.n || n > h->d_ens_scratch.n - offset)
            throw std::runtime_error("ensemble_scratch_read: range outside the scratch rows");
        if (n) hip_check(hipMemcpy(dst, h->d_ens_scratch.p + offset, n * sizeof(double), hipMemcpyDeviceToHost), "download");
    });
}

double shyft_hip_ensemble_last_ms(const shyft_hip_region* h) {
    if (h && h->sh) return shards::ensemble_last_ms(h->sh);
    return h && h->ens ? h->ens->last_ms : 0.0;
}

}  // extern "C"
