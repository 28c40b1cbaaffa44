// C-ABI implementation (include/shyft_hip.h): routing (core/routing.h:239-421) -- the routing groups of a region and
// their discharge sums, and the river network aggregation of such sums.
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "include_internal/host_tables.h"
#include "include_internal/kernels.h"
#include "include_internal/region_impl.h"
#include "include_internal/shards.h"

using namespace shyft_hip_impl;

extern "C" {

int shyft_hip_set_routing_groups(shyft_hip_region* h, const int32_t* group_of_cell, size_t n_groups) {
    if (!h) return fail(h, "shyft_hip_set_routing_groups: null handle");
    if (h->sh) return guarded(h, [&] { shards::set_routing_groups(h->sh, group_of_cell, n_groups); });
    return guarded(h, [&] {
        if (n_groups > 0 && !group_of_cell) throw std::runtime_error("set_routing_groups: group_of_cell is null");
        std::vector<int32_t> off, cells;  // the cells of each group, in cell order; group -1 = not routed
        const bool identity = build_csr(n_groups, off, cells, [&](auto&& emit) {
            for (size_t i = 0; i < h->n && n_groups; ++i) {
                const int32_t g = group_of_cell[i];
                if (g < -1 || g >= int32_t(n_groups)) throw std::runtime_error("set_routing_groups: group index out of range");
                if (g >= 0) emit(size_t(g), int32_t(i));
            }
        });
        h->rseg_identity = identity && cells.size() == h->n;
        h->d_rseg_off.alloc(n_groups + 1);
        h->d_rseg_cells.alloc(std::max<size_t>(1, cells.size()));
        hip_check(region_copy(h, h->d_rseg_off.p, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice), "upload");
        if (!cells.empty())
            hip_check(region_copy(h, h->d_rseg_cells.p, cells.data(), cells.size() * sizeof(int32_t), hipMemcpyHostToDevice),
                      "upload");
        h->n_route_groups = n_groups;
    });
}

int shyft_hip_routing_group_sums(const shyft_hip_region* hc, size_t step0, size_t n, double* dst, int dst_on_device) {
    shyft_hip_region* h = const_cast<shyft_hip_region*>(hc);
    if (!h || !dst) return fail(h, "shyft_hip_routing_group_sums: null argument");
    if (h->sh) return guarded(h, [&] { shards::routing_group_sums(h->sh, step0, n, dst, dst_on_device); });
    return guarded(h, [&] {
        const size_t G = h->n_route_groups;
        if (G == 0) return;
        const double* src = series_rows(h, SHYFT_HIP_AVG_DISCHARGE, step0, n, "routing_group_sums");
        staged_rows(h, dst, G * n, dst_on_device, [&](double* out) {
            hip_check(launch_segment_sums(src, h->n, n, h->rseg_identity ? nullptr : h->d_rseg_cells.p, h->d_rseg_off.p, G, out,
                                          h->stream),
                      "routing group sums");
        });
    });
}

int shyft_hip_route(int device, size_t n_groups, size_t T, const double* group_sums, int src_on_device,
                    const double* group_uhg, const int32_t* group_len, const int32_t* group_river, size_t n_rivers,
                    const double* river_uhg, const int32_t* river_len, const int32_t* river_downstream, size_t max_len,
                    double* local, double* upstream, double* output, int dst_on_device) {
    if (!group_sums || !group_uhg || !group_len || !group_river || !river_uhg || !river_len || !river_downstream ||
        !local || !upstream || !output)
        return fail(nullptr, "shyft_hip_route: null argument");
    try {
        if (device < 0) hip_check(hipGetDevice(&device), "hipGetDevice");
        hip_check(hipSetDevice(device), "hipSetDevice");
        const size_t R = n_rivers, G = n_groups;
        if (R == 0 || T == 0) return 0;
        if (max_len == 0) throw std::runtime_error("route: max_len == 0");
        for (size_t g = 0; g < G; ++g) {
            if (group_river[g] < 0 || size_t(group_river[g]) >= R) throw std::runtime_error("route: group river out of range");
            if (group_len[g] < 1 || size_t(group_len[g]) > max_len) throw std::runtime_error("route: group UHG length");
        }
        for (size_t r = 0; r < R; ++r) {
            if (river_len[r] < 1 || size_t(river_len[r]) > max_len) throw std::runtime_error("route: river UHG length");
            if (river_downstream[r] >= int32_t(R) || river_downstream[r] == int32_t(r))
                throw std::runtime_error("route: invalid downstream river");
        }
        // one member that owns every group: the groups of each river (ascending g), the upstream rivers, the levels
        const int64_t group_row[2] = {0, int64_t(G)};
        river_tables<int32_t> tb;
        if (!build_river_tables(1, group_row, group_river, R, river_downstream, tb))
            throw std::runtime_error("adding this river caused circular reference");
        hipStream_t s = nullptr;
        hip_check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
        struct stream_guard { hipStream_t s; ~stream_guard() { (void)hipStreamDestroy(s); } } sg{s};
        dbuf<double> d_sums, d_gw, d_rw, d_local, d_up, d_in, d_out;
        dbuf<int32_t> d_glen, d_gro, d_grs, d_rlen, d_upo, d_ups, d_lvl;
        auto up_d = [&](dbuf<double>& b, const double* src, size_t n, int on_dev) {
            b.alloc(std::max<size_t>(1, n));
            if (n) hip_check(hipMemcpy(b.p, src, n * sizeof(double), on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice), "upload");
        };
        auto up_i = [&](dbuf<int32_t>& b, const int32_t* src, size_t n) {
            b.alloc(std::max<size_t>(1, n));
            if (n) hip_check(hipMemcpy(b.p, src, n * sizeof(int32_t), hipMemcpyHostToDevice), "upload");
        };
        up_d(d_sums, group_sums, G * T, src_on_device);
        up_d(d_gw, group_uhg, G * max_len, 0);
        up_d(d_rw, river_uhg, R * max_len, 0);
        up_i(d_glen, group_len, G);
        up_i(d_gro, tb.pair_off.data(), tb.pair_off.size());
        up_i(d_grs, tb.pair_groups.data(), tb.pair_groups.size());
        up_i(d_rlen, river_len, R);
        up_i(d_upo, tb.up_off.data(), tb.up_off.size());
        up_i(d_ups, tb.ups.data(), tb.ups.size());
        up_i(d_lvl, tb.lvl_rivers.data(), tb.lvl_rivers.size());
        double* o_local = local;
        double* o_up = upstream;
        double* o_out = output;
        if (!dst_on_device) {
            d_local.alloc(R * T); d_up.alloc(R * T); d_out.alloc(R * T);
            o_local = d_local.p; o_up = d_up.p; o_out = d_out.p;
        }
        d_in.alloc(R * T);
        routing_args a;
        a.n_steps = int(T);
        a.n_rivers = int(R);
        a.max_len = int(max_len);
        a.group_sums = d_sums.p; a.group_w = d_gw.p; a.group_len = d_glen.p;
        a.river_group_off = d_gro.p; a.river_groups = d_grs.p;
        a.river_w = d_rw.p; a.river_len = d_rlen.p;
        a.river_up_off = d_upo.p; a.river_up = d_ups.p; a.level_rivers = d_lvl.p;
        a.local = o_local; a.upstream = o_up; a.inflow = d_in.p; a.output = o_out;
        hip_check(launch_route(a, tb.lvl_off.data(), tb.n_levels(), s), "route");
        hip_check(hipStreamSynchronize(s), "route sync");
        if (!dst_on_device) {
            hip_check(hipMemcpy(local, o_local, R * T * sizeof(double), hipMemcpyDeviceToHost), "download");
            hip_check(hipMemcpy(upstream, o_up, R * T * sizeof(double), hipMemcpyDeviceToHost), "download");
            hip_check(hipMemcpy(output, o_out, R * T * sizeof(double), hipMemcpyDeviceToHost), "download");
        }
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
    return 0;
}

}  // extern "C"
