// C-ABI implementation (include/shyft_hip.h): the interpolation step of a region (inverse distance, Bayesian
// temperature kriging into its forcing window) and the kriging entries that take no region.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "include_internal/device_call.h"
#include "include_internal/kernels.h"
#include "include_internal/layout.h"
#include "include_internal/region_impl.h"
#include "include_internal/shards.h"

using namespace shyft_hip_impl;

namespace {

void check_btk_param(const double* p) {
    if (!(p[0] > 0.0) || !std::isfinite(p[0])) throw std::runtime_error("btk: temperature_gradient_sd must be > 0");
    if (!(p[3] > 0.0)) throw std::runtime_error("btk: range must be > 0");
}

// the sources, the steps and the checked btk_param of a kriging call; the caller adds its destinations
btk_args btk_common_args(size_t n_sources, const double* src_xyz, const double* src_values, size_t n,
                         const double* prior_gradient, const double* btk_param) {
    btk_args a{};
    a.n_sources = n_sources;
    a.src_xyz = src_xyz;
    a.src_values = src_values;
    a.n_steps = n;
    a.prior_gradient = prior_gradient;
    a.gradient_sd = btk_param[0];
    a.sill = btk_param[1];
    a.nug = btk_param[2];
    a.range = btk_param[3];
    a.zscale = btk_param[4];
    return a;
}

// ordinary_kriging's parameter checks and its single-source copy (api_interpolation.cpp:88-93, 141-146), shared by
// the device and the host entry. Returns true when `out` is already complete.
bool ok_prepare(size_t n_sources, const double* src_values, size_t n, const double* ok_param, size_t n_dst,
                       double* out, ok_args& a) {
    if (n_sources == 0)
        throw std::runtime_error("the supplied src and dst_points should be non-null and have at least one time-series");
    if (!(ok_param[1] > 0.0))
        throw std::runtime_error("the supplied parameter a, covariance practical range, must be >0.0");
    if (!(ok_param[0] > 0.0)) throw std::runtime_error("the supplied parameter c, covariance sill, must be >0.0");
    if (!(ok_param[2] >= 0.0))
        throw std::runtime_error("the supplied parameter z_scale used to scale vertical distance must be >= 0.0");
    if (ok_param[3] != 0.0 && ok_param[3] != 1.0)
        throw std::runtime_error("ordinary_kriging: cov_type must be 0 (GAUSSIAN) or 1 (EXPONENTIAL)");
    if (!(ok_param[4] >= 0.0)) throw std::runtime_error("ordinary_kriging: dst_block must be >= 0");
    if (n == 0 || n_dst == 0) return true;
    if (n_sources == 1) {
        for (size_t t = 0; t < n; ++t)
            for (size_t d = 0; d < n_dst; ++d) out[t * n_dst + d] = src_values[t];
        return true;
    }
    a.n_sources = n_sources;
    a.src_values = src_values;
    a.n_steps = n;
    a.c = ok_param[0];
    a.a = ok_param[1];
    a.z_scale = ok_param[2];
    a.cov_type = int(ok_param[3]);
    a.dst_block = size_t(ok_param[4]);
    a.n_dst = n_dst;
    return false;
}

}  // namespace

extern "C" {

int shyft_hip_interpolate(shyft_hip_region* h, int var, size_t n_sources, const double* src_xyz, const double* src_values,
                          size_t step0, size_t n, const double* idw_param) {
    if (!h || !src_xyz || !src_values || !idw_param) return fail(h, "shyft_hip_interpolate: null argument");
    if (h->sh) return guarded(h, [&] { shards::interpolate(h->sh, var, n_sources, src_xyz, src_values, step0, n, idw_param); });
    return guarded(h, [&] {
        if (var < 0 || var >= N_FORCING) throw std::runtime_error("interpolate: invalid variable");
        if (!h->has_geo) throw std::runtime_error("interpolate: geo_cell_data not set");
        if (n_sources == 0) throw std::runtime_error("interpolate: no sources");
        double* out = series_rows(h, SHYFT_HIP_SERIES_FORCING + var, step0, n, "interpolate");
        const size_t N = h->n;
        const uint8_t* active = h->active.empty() ? nullptr : h->d_active.p;
        h->d_src_vals.alloc(std::max(h->d_src_vals.n, n * n_sources));
        hip_check(hipMemcpyAsync(h->d_src_vals.p, src_values, n * n_sources * sizeof(double), hipMemcpyHostToDevice,
                                 h->stream),
                  "upload source values");
        if (var == FV_TEMPERATURE && n_sources == 1) {
            // one temperature source: copied to the cells (region_model.h:470-481)
            hip_check(launch_copy_source(h->d_src_vals.p, int(n), int(N), active, out, h->stream), "copy_source");
            hip_check(hipStreamSynchronize(h->stream), "sync");
            h->idw[var].last_path = SHYFT_HIP_IDW_COPY;
            return;
        }
        static const int kind_of_var[N_FORCING] = {IDW_TEMPERATURE, IDW_PRECIPITATION, IDW_WIND_SPEED, IDW_REL_HUM,
                                                    IDW_RADIATION};
        const int kind = kind_of_var[var];
        const int K = int(idw_param[0]);
        if (K < 1 || K > IDW_KMAX)
            throw std::runtime_error("interpolate: max_members must be in [1, " + std::to_string(IDW_KMAX) + "]");
        if (h->dst_dirty) {
            std::vector<double> xyz(3 * N), slope(N);
            for (size_t i = 0; i < N; ++i) {
                for (int k = 0; k < 3; ++k) xyz[3 * i + k] = h->geo[i * 11 + k];
                slope[i] = h->geo[i * 11 + 5];
            }
            h->d_dst_xyz.alloc(3 * N);
            h->d_slope.alloc(N);
            hip_check(region_copy(h, h->d_dst_xyz.p, xyz.data(), 3 * N * sizeof(double), hipMemcpyHostToDevice), "upload dst");
            hip_check(region_copy(h, h->d_slope.p, slope.data(), N * sizeof(double), hipMemcpyHostToDevice), "upload slope");
            h->dst_dirty = false;
        }
        auto& tab = h->idw[var];
        std::vector<double> key = {double(kind), double(n_sources), idw_param[0], idw_param[1], idw_param[2],
                                   idw_param[3], idw_param[6]};
        key.insert(key.end(), src_xyz, src_xyz + 3 * n_sources);
        h->d_src_xyz.alloc(std::max(h->d_src_xyz.n, 3 * n_sources));
        hip_check(hipMemcpyAsync(h->d_src_xyz.p, src_xyz, 3 * n_sources * sizeof(double), hipMemcpyHostToDevice, h->stream),
                  "upload source xyz");
        if (key != tab.key) {
            tab.idx.alloc(size_t(K) * N);
            tab.w.alloc(size_t(K) * N);
            tab.aux.alloc(size_t(K) * N);
            tab.cnt.alloc(N);
            tab.K = K;
            idw_nb_args nb;
            nb.n_cells = int(N);
            nb.n_sources = int(n_sources);
            nb.kind = kind;
            nb.max_members = K;
            nb.max_distance = idw_param[1];
            nb.distance_measure_factor = idw_param[2];
            nb.zscale = idw_param[3];
            nb.scale_factor = idw_param[6];
            nb.src_xyz = h->d_src_xyz.p;
            nb.dst_xyz = h->d_dst_xyz.p;
            nb.idx = tab.idx.p;
            nb.w = tab.w.p;
            nb.aux = tab.aux.p;
            nb.count = tab.cnt.p;
            hip_check(launch_idw_neighbours(nb, h->stream), "idw_neighbours");
            // each wavefront's union of neighbour stations (the gather's compacted path when every union fits 64)
            const size_t n_waves = (N + 63) / 64;
            tab.wu.alloc(n_waves * 64);
            tab.wn.alloc(n_waves);
            tab.lidx.alloc(size_t((K + 3) / 4) * N);
            tab.ovf.alloc(1);
            hip_check(hipMemsetAsync(tab.ovf.p, 0, sizeof(int32_t), h->stream), "memset overflow");
            idw_union_args ua;
            ua.n_cells = int(N);
            ua.max_members = K;
            ua.idx = tab.idx.p;
            ua.count = tab.cnt.p;
            ua.wu = tab.wu.p;
            ua.wn = tab.wn.p;
            ua.lidx = tab.lidx.p;
            ua.overflow = tab.ovf.p;
            hip_check(launch_idw_wave_union(ua, h->stream), "idw_wave_union");
            int32_t ovf = 1;
            hip_check(region_copy(h, &ovf, tab.ovf.p, sizeof(int32_t), hipMemcpyDeviceToHost), "read overflow");
            tab.wave_ok = ovf == 0;
            tab.key.swap(key);
        }
        idw_gather_args g;
        g.n_cells = int(N);
        g.n_sources = int(n_sources);
        g.n_rows = int(n);
        g.kind = kind;
        g.by_equation = idw_param[5] != 0.0;
        g.max_members = tab.K;
        g.default_gradient = idw_param[4];
        g.src_xyz = h->d_src_xyz.p;
        g.src_values = h->d_src_vals.p;
        g.dst_xyz = h->d_dst_xyz.p;
        g.slope = h->d_slope.p;
        g.idx = tab.idx.p;
        g.w = tab.w.p;
        g.aux = tab.aux.p;
        g.count = tab.cnt.p;
        g.active = active;
        g.out = out;
        // SHYFT_IDW_TILE=1: the row-tile gather even where the wavefront unions fit (tests cover both paths)
        const bool wave = tab.wave_ok && !getenv("SHYFT_IDW_TILE");
        g.wu = wave ? tab.wu.p : nullptr;
        g.wn = wave ? tab.wn.p : nullptr;
        g.lidx = wave ? tab.lidx.p : nullptr;
        hip_check(hipEventRecord(h->ev0, h->stream), "hipEventRecord");
        hip_check(launch_idw_gather(g, h->stream), "idw_gather");
        hip_check(hipEventRecord(h->ev1, h->stream), "hipEventRecord");
        hip_check(hipStreamSynchronize(h->stream), "idw");
        float ms = 0.0f;
        hip_check(hipEventElapsedTime(&ms, h->ev0, h->ev1), "hipEventElapsedTime");
        h->last_interp_ms = ms;
        tab.last_path = wave ? SHYFT_HIP_IDW_WAVE : SHYFT_HIP_IDW_TILE;
    });
}

int shyft_hip_interpolation_path(const shyft_hip_region* h, int var) {
    if (!h || var < 0 || var >= N_FORCING) return -1;
    if (h->sh) return shards::interpolation_path(h->sh, var);
    return h->idw[var].last_path;
}

int shyft_hip_interpolate_btk(shyft_hip_region* h, size_t n_sources, const double* src_xyz, const double* src_values,
                              size_t step0, size_t n, const double* prior_gradient, const double* btk_param) {
    if (!h || !src_xyz || !src_values || !btk_param) return fail(h, "shyft_hip_interpolate_btk: null argument");
    if (h->sh) return guarded(h, [&] { shards::interpolate_btk(h->sh, n_sources, src_xyz, src_values, step0, n, prior_gradient, btk_param); });
    return guarded(h, [&] {
        if (!h->has_geo) throw std::runtime_error("interpolate: geo_cell_data not set");
        if (n_sources == 0) throw std::runtime_error("interpolate: no sources");
        double* out = series_rows(h, SHYFT_HIP_SERIES_FORCING + FV_TEMPERATURE, step0, n, "interpolate_btk");
        check_btk_param(btk_param);
        const size_t N = h->n;
        if (n_sources == 1) {  // one temperature source: copied to the cells (region_model.h:470-481)
            const uint8_t* active = h->active.empty() ? nullptr : h->d_active.p;
            h->d_src_vals.alloc(std::max(h->d_src_vals.n, n));
            hip_check(hipMemcpyAsync(h->d_src_vals.p, src_values, n * sizeof(double), hipMemcpyHostToDevice, h->stream),
                      "upload source values");
            hip_check(launch_copy_source(h->d_src_vals.p, int(n), int(N), active, out, h->stream), "copy_source");
            hip_check(hipStreamSynchronize(h->stream), "sync");
            return;
        }
        std::vector<double> prior;
        if (!prior_gradient) {
            prior.resize(n);
            for (size_t i = 0; i < n; ++i) prior[i] = btk_prior_gradient(h->t0 + int64_t(step0 + i) * h->dt, h->dt);
            prior_gradient = prior.data();
        }
        // destinations: the calculated cells (region_model.h:420-423), written in place of the window
        std::vector<double> xyz;
        std::vector<int32_t> index;
        xyz.reserve(3 * N);
        for (size_t i = 0; i < N; ++i) {
            if (!h->active.empty() && !h->active[i]) continue;
            for (int k = 0; k < 3; ++k) xyz.push_back(h->geo[i * 11 + k]);
            index.push_back(int32_t(i));
        }
        const size_t D = index.size();
        if (D == 0) return;
        const bool all = D == N;
        if (xyz != h->btk_xyz_host || index != h->btk_index_host || h->btk_dst_version == 0) {
            h->d_btk_xyz.alloc(3 * D);
            hip_check(region_copy(h, h->d_btk_xyz.p, xyz.data(), 3 * D * sizeof(double), hipMemcpyHostToDevice),
                      "upload btk destinations");
            if (!all) {
                h->d_btk_index.alloc(D);
                hip_check(region_copy(h, h->d_btk_index.p, index.data(), D * sizeof(int32_t), hipMemcpyHostToDevice),
                          "upload btk index");
            }
            h->btk_xyz_host.swap(xyz);
            h->btk_index_host.swap(index);
            ++h->btk_dst_version;
        }
        if (!h->btk) h->btk.reset(btk_cache_create());
        btk_args a = btk_common_args(n_sources, src_xyz, src_values, n, prior_gradient, btk_param);
        a.cache = h->btk.get();
        a.dst_version = h->btk_dst_version;
        a.n_dst = D;
        a.d_dst_xyz = h->d_btk_xyz.p;
        a.d_dst_index = all ? nullptr : h->d_btk_index.p;
        a.d_out = out;
        a.ld_out = N;
        btk_run(a, h->stream);
        hip_check(hipStreamSynchronize(h->stream), "btk");
    });
}

int shyft_hip_btk(int device, size_t n_sources, const double* src_xyz, const double* src_values, size_t n,
                  const double* prior_gradient, const double* btk_param, size_t n_dst, const double* dst_xyz,
                  double* out) {
    return shyft_hip_btk_blocked(device, n_sources, src_xyz, src_values, n, prior_gradient, btk_param, n_dst, dst_xyz,
                                 out, 0);
}

int shyft_hip_btk_blocked(int device, size_t n_sources, const double* src_xyz, const double* src_values, size_t n,
                          const double* prior_gradient, const double* btk_param, size_t n_dst, const double* dst_xyz,
                          double* out, size_t block_steps) {
    if (!src_xyz || !src_values || !prior_gradient || !btk_param || !dst_xyz || !out)
        return fail(nullptr, "shyft_hip_btk: null argument");
    try {
        if (n_sources == 0) throw std::runtime_error("bayesian_kriging_temperature: no sources");
        check_btk_param(btk_param);
        if (n == 0 || n_dst == 0) return 0;
        if (n_sources == 1) {  // api_interpolation.cpp:63-69: a clean copy to the destinations
            for (size_t t = 0; t < n; ++t)
                for (size_t d = 0; d < n_dst; ++d) out[t * n_dst + d] = src_values[t];
            return 0;
        }
        device_call c(device);
        dbuf<double> d_xyz, d_out;
        c.upload(d_xyz, dst_xyz, 3 * n_dst, "upload");
        d_out.alloc(n * n_dst);
        btk_args a = btk_common_args(n_sources, src_xyz, src_values, n, prior_gradient, btk_param);
        a.n_dst = n_dst;
        a.d_dst_xyz = d_xyz.p;
        a.d_dst_index = nullptr;
        a.d_out = d_out.p;
        a.ld_out = n_dst;
        a.max_block_steps = block_steps;
        btk_run(a, c.s);
        c.download(out, d_out.p, n * n_dst, "download");
        c.sync("sync");
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ordinary_kriging(int device, size_t n_sources, const double* src_xyz, const double* src_values, size_t n,
                               const double* ok_param, size_t n_dst, const double* dst_xyz, double* out) {
    if (!src_xyz || !src_values || !ok_param || !dst_xyz || !out)
        return fail(nullptr, "shyft_hip_ordinary_kriging: null argument");
    try {
        ok_args a{};
        if (ok_prepare(n_sources, src_values, n, ok_param, n_dst, out, a)) return 0;
        device_call c(device);
        dbuf<double> d_xyz, d_out;
        c.upload(d_xyz, dst_xyz, 3 * n_dst, "upload");
        d_out.alloc(n * n_dst);
        a.src_xyz = src_xyz;
        a.dst_xyz = dst_xyz;
        a.d_dst_xyz = d_xyz.p;
        a.d_out = d_out.p;
        a.ld_out = n_dst;
        ok_run(a, c.s);
        c.download(out, d_out.p, n * n_dst, "download");
        c.sync("sync");
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_ordinary_kriging_host(size_t n_sources, const double* src_xyz, const double* src_values, size_t n,
                                    const double* ok_param, size_t n_dst, const double* dst_xyz, double* out) {
    if (!src_xyz || !src_values || !ok_param || !dst_xyz || !out)
        return fail(nullptr, "shyft_hip_ordinary_kriging_host: null argument");
    try {
        ok_args a{};
        if (ok_prepare(n_sources, src_values, n, ok_param, n_dst, out, a)) return 0;
        a.src_xyz = src_xyz;
        a.dst_xyz = dst_xyz;
        ok_host_run(a, out);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

}  // extern "C"
