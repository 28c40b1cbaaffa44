// routing::uhg river aggregation for a parameter ensemble on gfx950: shyft_hip_route (kernels/routing.hip) for P
// independent sets of routing groups over ONE shared river network, the member dimension inside each launch.
//
// Calibration varies routing.velocity / alpha / beta with the parameter vector, so every ensemble member partitions the
// cells into its own (river, UHG) groups. Member m owns the global group rows [group_row[m], group_row[m+1]); the
// rivers, their UHGs and the network are shared. Three stages, as in routing.hip, 1 + 2 x levels launches for the
// whole batch:
//
//   rm_local_kernel : local[m][r][t] = sum_{g of m in r} sum_{j < L_g, j <= t} w_g[j] S[g][t-j]
//   rm_in_kernel    : in[m][r][t]    = local[m][r][t] + sum_{u upstream of r} out[m][u][t]      (one network level)
//   rm_out_kernel   : out[m][r][t]   = sum_{j < L_r, j <= t} w_r[j] in[m][r][t-j]               (one network level)
//
// The additions follow routing.hip, which is what shyft_hip_route_members_host states as literal loops: within a river
// the groups in ascending row, within a group the taps in ascending j with the group's sum completed before it is added
// to the river's accumulator, upstream rivers in ascending index, no contraction (-ffp-contract=off). routing.hip adds
// 0.0 for the taps j > t; an accumulator that starts at +0.0 never becomes -0.0 by adding products, so stopping the tap
// loop at min(L, t + 1) gives the same bits, and that is what both the kernels and the host twin do.
//
// Convolution form: a workgroup of RM_TILE lanes owns RM_TILE consecutive steps of one (member, river); for each chunk
// of up to RM_CHUNK taps it stages the taps and the RM_TILE + cnt - 1 series values the tile reads in LDS (at most
// 6 KB), then every lane runs its in-order accumulator out of LDS. The window is sized by the chunk's own tap count, so
// a two-tap cell UHG stages 258 values, not 511. (member x river x tile) is flattened into grid.x and strided over.
//
// Index safety. Before any launch the host checks (rm_check): group_row starts at 0 and does not decrease, so
// group_row[P] rows of sums, taps, lengths and rivers were uploaded; every group's river lies in [0, R); every UHG
// length lies in [1, max_len], so w[j] with j < L stays inside the row; every downstream index is -1 or another river in
// [0, R) and the network has no cycle, so the upstream table holds rivers in [0, R) and every river has a level. The
// (member, river) group table is built from those checked values. A work item q < pairs * tiles gives pair < pairs and
// a tile with i0 < T; a lane reads s[g] only for 0 <= g < T and writes only for t < T.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/shyft_hip.h"
#include "../include_internal/device_call.h"
#include "../include_internal/host_tables.h"

using namespace shyft_hip_impl;

namespace {

constexpr int RM_TILE = 256;   // steps per workgroup, one lane each
constexpr int RM_CHUNK = 256;  // taps per staged chunk
constexpr int RM_WINDOW = RM_TILE + RM_CHUNK - 1;
constexpr int64_t RM_MAX_GRID = 1 << 20;

struct rm_args {
    int64_t T, tiles;  // steps, tiles per (member, river)
    int32_t P, R, max_len;
    const double* group_sums;     // [G][T]
    const double* group_w;        // [G][max_len]
    const int32_t* group_len;     // [G]
    const int64_t* pair_off;      // [P*R + 1] CSR of the group rows of (member, river), ascending row
    const int32_t* pair_groups;   // [G]
    const double* river_w;        // [R][max_len]
    const int32_t* river_len;     // [R]
    const int32_t* river_up_off;  // [R+1] CSR of upstream rivers, ascending index
    const int32_t* river_up;
    const int32_t* level_rivers;  // rivers by network level, upstream levels first
    double* local;                // [P][R][T]
    double* upstream;             // [P][R][T] or null
    double* inflow;               // [P][R][T]
    double* output;               // [P][R][T]
};

// sum_{j < L, j <= t} w[j] s[t-j] for t = i0 + lane, taps ascending; uniform control flow over the workgroup
__device__ __forceinline__ double rm_conv_tile(const double* __restrict__ s, int64_t T, int64_t i0,
                                               const double* __restrict__ w, int L, double* xs, double* ws) {
    const int l = int(threadIdx.x);
    const int64_t t = i0 + l;
    double v = 0.0;
    for (int j0 = 0; j0 < L; j0 += RM_CHUNK) {
        const int cnt = L - j0 < RM_CHUNK ? L - j0 : RM_CHUNK;
        const int64_t lo = i0 - j0 - (cnt - 1);  // the series index of window slot 0
        __syncthreads();                         // the previous chunk (or convolution) has been read
        for (int m = l; m < RM_TILE + cnt - 1; m += RM_TILE) {
            const int64_t g = lo + m;
            xs[m] = (g >= 0 && g < T) ? s[g] : 0.0;
        }
        if (l < cnt) ws[l] = w[j0 + l];
        __syncthreads();
        if (t < T) {
            const double* __restrict__ x = xs + l + (cnt - 1);  // x[-jj] is series index t - j0 - jj
            const int64_t left = t - j0 + 1;                    // the taps of this chunk with j <= t
            const int inside = left <= 0 ? 0 : (left < cnt ? int(left) : cnt);
#pragma unroll 4
            for (int jj = 0; jj < inside; ++jj) v += ws[jj] * x[-jj];
        }
    }
    return v;
}

__global__ __launch_bounds__(RM_TILE) void rm_local_kernel(const rm_args a) {
    __shared__ double xs[RM_WINDOW];
    __shared__ double ws[RM_CHUNK];
    const int64_t total = int64_t(a.P) * a.R * a.tiles;
    for (int64_t q = blockIdx.x; q < total; q += gridDim.x) {  // uniform over the workgroup
        const int64_t pair = q / a.tiles, i0 = (q - pair * a.tiles) * RM_TILE;
        const int64_t t = i0 + threadIdx.x;
        double acc = 0.0;
        for (int64_t k = a.pair_off[pair]; k < a.pair_off[pair + 1]; ++k) {
            const int32_t g = a.pair_groups[k];
            acc += rm_conv_tile(a.group_sums + size_t(g) * a.T, a.T, i0, a.group_w + size_t(g) * a.max_len,
                                a.group_len[g], xs, ws);
        }
        if (t < a.T) a.local[size_t(pair) * a.T + t] = acc;
    }
}

__global__ __launch_bounds__(RM_TILE) void rm_in_kernel(const rm_args a, int level_begin, int level_n) {
    const int64_t total = int64_t(a.P) * level_n * a.tiles;
    for (int64_t q = blockIdx.x; q < total; q += gridDim.x) {
        const int64_t pl = q / a.tiles, t = (q - pl * a.tiles) * RM_TILE + threadIdx.x;
        const int64_t m = pl / level_n;
        const int32_t r = a.level_rivers[level_begin + int(pl - m * level_n)];
        if (t >= a.T) continue;
        const size_t row = size_t(m) * a.R;
        double up = 0.0;
        for (int k = a.river_up_off[r]; k < a.river_up_off[r + 1]; ++k) up += a.output[(row + a.river_up[k]) * a.T + t];
        if (a.upstream) a.upstream[(row + r) * a.T + t] = up;
        a.inflow[(row + r) * a.T + t] = a.local[(row + r) * a.T + t] + up;
    }
}

__global__ __launch_bounds__(RM_TILE) void rm_out_kernel(const rm_args a, int level_begin, int level_n) {
    __shared__ double xs[RM_WINDOW];
    __shared__ double ws[RM_CHUNK];
    const int64_t total = int64_t(a.P) * level_n * a.tiles;
    for (int64_t q = blockIdx.x; q < total; q += gridDim.x) {  // uniform over the workgroup
        const int64_t pl = q / a.tiles, i0 = (q - pl * a.tiles) * RM_TILE;
        const int64_t m = pl / level_n;
        const int32_t r = a.level_rivers[level_begin + int(pl - m * level_n)];
        const size_t row = (size_t(m) * a.R + r) * a.T;
        const int64_t t = i0 + threadIdx.x;
        const double v = rm_conv_tile(a.inflow + row, a.T, i0, a.river_w + size_t(r) * a.max_len, a.river_len[r], xs, ws);
        if (t < a.T) a.output[row + t] = v;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
using rm_tables = river_tables<int64_t>;

// The argument checks shared by the device entry and its host twin, before the device is touched; builds the tables.
// Returns false when there is nothing to do.
bool rm_check(size_t P, const int64_t* group_row, size_t T, const double* group_sums, const double* group_uhg,
              const int32_t* group_len, const int32_t* group_river, size_t R, const double* river_uhg,
              const int32_t* river_len, const int32_t* river_downstream, size_t max_len, const double* output,
              rm_tables& tb) {
    if (!group_row || !river_uhg || !river_len || !river_downstream || !output)
        throw std::runtime_error("route_members: null argument");
    if (P == 0 || R == 0 || T == 0) return false;
    if (group_row[0] != 0) throw std::runtime_error("route_members: group_row must start at 0");
    for (size_t m = 0; m < P; ++m)
        if (group_row[m + 1] < group_row[m]) throw std::runtime_error("route_members: group_row must not decrease");
    const size_t G = size_t(group_row[P]);
    if (G > size_t(INT32_MAX)) throw std::runtime_error("route_members: more than 2^31 groups");
    if (P * R > size_t(INT32_MAX)) throw std::runtime_error("route_members: members x rivers exceeds 2^31");
    if (G && (!group_sums || !group_uhg || !group_len || !group_river))
        throw std::runtime_error("route_members: null argument");
    if (max_len == 0 || max_len > size_t(INT32_MAX)) throw std::runtime_error("route_members: max_len out of range");
    for (size_t g = 0; g < G; ++g) {
        if (group_river[g] < 0 || size_t(group_river[g]) >= R)
            throw std::runtime_error("route_members: group river out of range");
        if (group_len[g] < 1 || size_t(group_len[g]) > max_len) throw std::runtime_error("route_members: group UHG length");
    }
    for (size_t r = 0; r < R; ++r) {
        if (river_len[r] < 1 || size_t(river_len[r]) > max_len) throw std::runtime_error("route_members: river UHG length");
        if (river_downstream[r] < -1 || river_downstream[r] >= int32_t(R) || river_downstream[r] == int32_t(r))
            throw std::runtime_error("route_members: invalid downstream river");
    }
    if (!build_river_tables(P, group_row, group_river, R, river_downstream, tb))
        throw std::runtime_error("route_members: the river network has a cycle");
    return true;
}

// sum_{j < L, j <= t} w[j] s[t-j], taps ascending
inline double rm_conv_at(const double* w, int L, const double* s, size_t t) {
    double v = 0.0;
    for (int j = 0; j < L && size_t(j) <= t; ++j) v += w[j] * s[t - size_t(j)];
    return v;
}

call_record g_rm;

unsigned rm_grid(int64_t items) { return unsigned(std::min<int64_t>(items, RM_MAX_GRID)); }

}  // namespace

extern "C" {

int shyft_hip_route_members_host(size_t n_members, const int64_t* group_row, size_t T, const double* group_sums,
                                 const double* group_uhg, const int32_t* group_len, const int32_t* group_river,
                                 size_t n_rivers, const double* river_uhg, const int32_t* river_len,
                                 const int32_t* river_downstream, size_t max_len, double* local, double* upstream,
                                 double* output) {
    try {
        rm_tables tb;
        const size_t P = n_members, R = n_rivers;
        if (!rm_check(P, group_row, T, group_sums, group_uhg, group_len, group_river, R, river_uhg, river_len,
                      river_downstream, max_len, output, tb))
            return 0;
        std::vector<double> loc(R * T), in(T);
        for (size_t m = 0; m < P; ++m) {
            double* out = output + m * R * T;
            for (size_t r = 0; r < R; ++r)  // local_inflow: the member's groups of the river, ascending
                for (size_t t = 0; t < T; ++t) {
                    double acc = 0.0;
                    for (int64_t g = group_row[m]; g < group_row[m + 1]; ++g)
                        if (size_t(group_river[g]) == r)
                            acc += rm_conv_at(group_uhg + size_t(g) * max_len, group_len[g], group_sums + size_t(g) * T, t);
                    loc[r * T + t] = acc;
                }
            for (int32_t r : tb.lvl_rivers) {  // upstream levels first: a river's upstream outputs are complete
                for (size_t t = 0; t < T; ++t) {
                    double up = 0.0;
                    for (size_t u = 0; u < R; ++u)  // upstream_inflow: ascending river index
                        if (river_downstream[u] == r) up += out[u * T + t];
                    if (upstream) upstream[(m * R + size_t(r)) * T + t] = up;
                    in[t] = loc[size_t(r) * T + t] + up;
                }
                for (size_t t = 0; t < T; ++t)
                    out[size_t(r) * T + t] = rm_conv_at(river_uhg + size_t(r) * max_len, river_len[r], in.data(), t);
            }
            if (local) std::copy(loc.begin(), loc.end(), local + m * R * T);
        }
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
    return 0;
}

int shyft_hip_route_members(int device, size_t n_members, const int64_t* group_row, size_t T, const double* group_sums,
                            int src_on_device, const double* group_uhg, const int32_t* group_len,
                            const int32_t* group_river, size_t n_rivers, const double* river_uhg,
                            const int32_t* river_len, const int32_t* river_downstream, size_t max_len, double* local,
                            double* upstream, double* output, int dst_on_device) {
    try {
        rm_tables tb;
        const size_t P = n_members, R = n_rivers;
        if (!rm_check(P, group_row, T, group_sums, group_uhg, group_len, group_river, R, river_uhg, river_len,
                      river_downstream, max_len, output, tb))
            return 0;
        const size_t G = size_t(group_row[P]), PRT = P * R * T;
        device_call dc(device);
        dbuf<double> d_sums, d_gw, d_rw, d_local, d_up, d_in, d_out;
        dbuf<int32_t> d_glen, d_pg, d_rlen, d_upo, d_ups, d_lvl;
        dbuf<int64_t> d_po;
        const double* sums = group_sums;
        if (!src_on_device) {
            dc.upload(d_sums, group_sums, G * T, "upload group sums");
            sums = d_sums.p;
        }
        dc.upload(d_gw, group_uhg, G * max_len, "upload group uhg");
        dc.upload(d_glen, group_len, G, "upload group len");
        dc.upload(d_po, tb.pair_off.data(), tb.pair_off.size(), "upload pair offsets");
        dc.upload(d_pg, tb.pair_groups.data(), G, "upload pair groups");
        dc.upload(d_rw, river_uhg, R * max_len, "upload river uhg");
        dc.upload(d_rlen, river_len, R, "upload river len");
        dc.upload(d_upo, tb.up_off.data(), tb.up_off.size(), "upload upstream offsets");
        dc.upload(d_ups, tb.ups.data(), tb.ups.size(), "upload upstream rivers");
        dc.upload(d_lvl, tb.lvl_rivers.data(), tb.lvl_rivers.size(), "upload levels");
        rm_args a;
        a.T = int64_t(T);
        a.tiles = int64_t((T + RM_TILE - 1) / RM_TILE);
        a.P = int32_t(P); a.R = int32_t(R); a.max_len = int32_t(max_len);
        a.group_sums = sums; a.group_w = d_gw.p; a.group_len = d_glen.p;
        a.pair_off = d_po.p; a.pair_groups = d_pg.p;
        a.river_w = d_rw.p; a.river_len = d_rlen.p;
        a.river_up_off = d_upo.p; a.river_up = d_ups.p; a.level_rivers = d_lvl.p;
        d_in.alloc(PRT);
        a.inflow = d_in.p;
        if (dst_on_device && local) a.local = local;
        else { d_local.alloc(PRT); a.local = d_local.p; }
        if (!upstream) a.upstream = nullptr;
        else if (dst_on_device) a.upstream = upstream;
        else { d_up.alloc(PRT); a.upstream = d_up.p; }
        if (dst_on_device) a.output = output;
        else { d_out.alloc(PRT); a.output = d_out.p; }
        dc.begin();
        hipLaunchKernelGGL(rm_local_kernel, dim3(rm_grid(int64_t(P * R) * a.tiles)), dim3(RM_TILE), 0, dc.s, a);
        for (size_t l = 0; l + 1 < tb.lvl_off.size(); ++l) {
            const int b = tb.lvl_off[l], n = tb.lvl_off[l + 1] - b;
            if (n == 0) continue;
            const unsigned grid = rm_grid(int64_t(P) * n * a.tiles);
            hipLaunchKernelGGL(rm_in_kernel, dim3(grid), dim3(RM_TILE), 0, dc.s, a, b, n);
            hipLaunchKernelGGL(rm_out_kernel, dim3(grid), dim3(RM_TILE), 0, dc.s, a, b, n);
        }
        hip_check(hipGetLastError(), "route_members");
        dc.end();
        if (!dst_on_device) {
            if (local) dc.download(local, a.local, PRT, "download local");
            if (upstream) dc.download(upstream, a.upstream, PRT, "download upstream");
            dc.download(output, a.output, PRT, "download output");
        }
        g_rm.record(dc.dev, dc.finish("route_members sync"));
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
    return 0;
}

double shyft_hip_route_members_last_ms(int device) { return g_rm.last_ms.load(device, 0.0); }

}  // extern "C"
