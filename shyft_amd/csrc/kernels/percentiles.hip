// Cell percentiles of a [step][cell] series (gfx950): calculate_percentiles with skip_nans
// (core/time_series_statistics.h:112-246) over the cells of one or more segments, selected on the device.
//
// A segment is (offset, count) into an int32 cell-index array (or the identity); the result is [segment][pct][step].
// The samples of one (segment, step) "job" are the finite values of the segment's cells at that step.
//
//  - Every fp64 sample maps to an order-preserving 64-bit key, so order statistics are exact integer selections and
//    every non-AVERAGE result is bit-identical to a full sort (time_series_statistics.h:124-153). +0.0 and -0.0 are
//    different keys that compare equal as doubles: the sign of a zero result is unspecified.
//  - LDS-sort path (segments of at most SHYFT_HIP_PERCENTILES_LDS_MAX cells): one workgroup compacts the job's
//    finite keys into LDS, bitonic-sorts them there and reads the ranks off.
//  - Radix-select path: an MSD radix select over 8 passes of 8-bit digits for all ranks of a job at once (a
//    percentile needs at most two adjacent ranks; equal ranks share one selection). Per pass one histogram launch
//    (a job's row is split over workgroups; integer counts in LDS, flushed with integer atomics to a global histogram,
//    so the order of the atomics cannot change a count) and one pick launch (per job: prefix-scan the 256 counts, fix
//    the next digit of every rank). The finite count, the ranks and the prefixes stay on the device: there is no
//    host round trip per step or per pass.
//  - AVERAGE: the finite samples summed by lanes striding in cell order, then the fixed wavefront shuffle tree + LDS
//    combine of kernels/stats.hip, divided by the finite count: reproducible run to run, and the same for both
//    paths (it is not the reference's sorted sequential sum, time_series_statistics.h:127-132). The combine is
//    block_sum of device/workgroup.h, the one kernels/stats.hip calls.
//  - No floating-point atomics anywhere.
//
// Index safety: cell indexes come from select_cells / the region's segment tables (< n_cells); a digit is key bits
// masked to 0..255; histogram rows are indexed by a selection number < 2 * n_pct; the LDS sort pads and sorts slots
// below Q <= P (device/workgroup.h states its own reads) and reads rank min(rank, nf - 1) of the at least nf keys; a
// job without finite samples writes NaNs only.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <limits>
#include <stdint.h>
#include <vector>

#include "../device/pct_plan.h"
#include "../device/workgroup.h"
#include "../include_internal/kernels.h"

namespace {

constexpr int PB = 256;                 // 4 wavefronts
constexpr int PCT_MAX = SHYFT_HIP_PERCENTILES_MAX;
constexpr int PCT_SEL = 2 * PCT_MAX;    // selections (ranks) per job: lower and upper of every percentile
constexpr int PCT_CHUNK = 16384;        // cells of a job's row per histogram workgroup

// pct_plan / pct_make_plan and pct_value: device/pct_plan.h, shared with kernels/ts_percentiles.hip; key_of / value_of,
// the workgroup sum and scan and the LDS sort: device/workgroup.h

// ---------------------------------------------------------------------------------------------- AVERAGE
// One workgroup per job (blockIdx.x = seg * n_steps + t). Lane l adds the finite ones of the segment's elements
// l, l + 256, ... in that order (four loads ahead, added in the same order).
template <bool ID>
__global__ __launch_bounds__(PB) void pct_average_kernel(const double* __restrict__ series, size_t n_cells, int n_steps,
                                                         const int32_t* __restrict__ seg_cells,
                                                         const int32_t* __restrict__ seg_off, pct_list pl,
                                                         double* __restrict__ out) {
    const int job = blockIdx.x;
    const int c = job / n_steps, t = job - c * n_steps;
    const double* __restrict__ row = series + (size_t)t * n_cells;
    const int32_t b = seg_off[c], e = seg_off[c + 1];
    double acc = 0.0;
    uint32_t cnt = 0;
    int32_t k = b + (int32_t)threadIdx.x;
    for (; k + 3 * PB < e; k += 4 * PB) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = row[ID ? k + u * PB : seg_cells[k + u * PB]];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            uint64_t key;
            if (key_of(v[u], key)) {
                acc += v[u];
                ++cnt;
            }
        }
    }
    for (; k < e; k += PB) {
        const double v = row[ID ? k : seg_cells[k]];
        uint64_t key;
        if (key_of(v, key)) {
            acc += v;
            ++cnt;
        }
    }
    const double s = block_sum<PB>(acc);
    const uint32_t n = block_sum<PB>(cnt);
    if (threadIdx.x == 0) {
        const double r = n > 0 ? s / double(n) : rs_nan();
        for (int i = 0; i < pl.n; ++i)
            if (pl.p[i] == -1) out[((size_t)c * pl.n + i) * n_steps + t] = r;
    }
}

// ---------------------------------------------------------------------------------------------- LDS sort
// One workgroup per job. keys[P], P = the launch's power of two >= the largest segment, then the finite counter
// (dynamic LDS).
template <bool ID>
__global__ __launch_bounds__(PB) void pct_lds_sort_kernel(const double* __restrict__ series, size_t n_cells, int n_steps,
                                                          const int32_t* __restrict__ seg_cells,
                                                          const int32_t* __restrict__ seg_off, pct_list pl, int P,
                                                          double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pct_smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(pct_smem);
    uint32_t& n_fin = *reinterpret_cast<uint32_t*>(keys + P);  // after the keys: no static LDS in front of them
    const int job = blockIdx.x;
    const int c = job / n_steps, t = job - c * n_steps;
    const double* __restrict__ row = series + (size_t)t * n_cells;
    const int32_t b = seg_off[c], e = seg_off[c + 1];
    if (e - b > P) return;  // never: the launcher sizes P from the largest segment
    if (threadIdx.x == 0) n_fin = 0u;
    __syncthreads();
    // compact the finite keys (their order in LDS is arbitrary: the sort follows); at most e - b <= P slots are taken
    for (int32_t k = b + (int32_t)threadIdx.x; k < e; k += PB) {
        uint64_t key;
        if (key_of(row[ID ? k : seg_cells[k]], key)) keys[atomicAdd(&n_fin, 1u)] = key;
    }
    __syncthreads();
    const int nf = (int)n_fin;
    const int Q = lds_sort_pad<false>(keys, nullptr, nf, (int)threadIdx.x, PB);  // power of two >= nf, <= P
    __syncthreads();
    lds_bitonic_sort<false, false>(keys, nullptr, Q, (int)threadIdx.x, PB);
    for (int i = threadIdx.x; i < pl.n; i += PB) {
        const pct_plan q = pct_make_plan(pl.p[i], nf);
        if (q.kind == PCT_AVG) continue;  // pct_average_kernel writes these
        double r = rs_nan();
        if (q.kind != PCT_NAN) {
            const uint32_t last = uint32_t(nf - 1);
            r = pct_value(q, value_of(keys[q.lo < last ? q.lo : last]), value_of(keys[q.hi < last ? q.hi : last]));
        }
        out[((size_t)c * pl.n + i) * n_steps + t] = r;
    }
}

// ---------------------------------------------------------------------------------------------- radix select
// Per-job selection state, device resident between the passes.
struct pct_job {
    uint32_t nf;               // finite samples
    int32_t n_u;               // distinct ranks to select
    uint32_t urank[PCT_SEL];   // rank of selection u inside its current prefix bucket
    uint64_t uprefix[PCT_SEL]; // the key digits fixed so far (high digits first)
    int32_t lo_u[PCT_MAX], hi_u[PCT_MAX];  // selection of each percentile's lower / upper rank
};

// Histogram of digit `pass` (0 = the top 8 bits). Grid (chunks, jobs of the batch). Pass 0 counts every finite key
// into row 0; later passes count, for every selection u, the keys whose higher digits equal uprefix[u] (in LDS once
// per distinct prefix, flushed to the global row of every selection that has it).
template <bool ID, bool PASS0>
__global__ __launch_bounds__(PB) void pct_hist_kernel(const double* __restrict__ series, size_t n_cells, int n_steps,
                                                      const int32_t* __restrict__ seg_cells,
                                                      const int32_t* __restrict__ seg_off, int job0, int pass, int rows,
                                                      const pct_job* __restrict__ jobs, uint32_t* __restrict__ ghist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pct_smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(pct_smem);  // [n_q][256]
    __shared__ uint64_t pre[PCT_SEL];   // the distinct prefixes of the job's selections
    __shared__ int32_t row_of[PCT_SEL];  // selection u counts in histogram row row_of[u]
    __shared__ int32_t n_q_s;
    const int jb = blockIdx.y;
    const int job = job0 + jb;
    const int c = job / n_steps, t = job - c * n_steps;
    const int32_t b = seg_off[c], e = seg_off[c + 1];
    const int32_t cb = b + (int32_t)blockIdx.x * PCT_CHUNK;
    if (cb >= e) return;
    const int32_t ce = e - cb > PCT_CHUNK ? cb + PCT_CHUNK : e;
    int n_u = 1;
    if (!PASS0) {
        n_u = jobs[jb].n_u;
        if (n_u > rows) n_u = rows;  // never: n_u <= 2 * n_pct == rows
        if (n_u <= 0) return;
        // selections that share a prefix (near ranks, clustered data) share one histogram row
        if (threadIdx.x == 0) {
            int n_q = 0;
            for (int u = 0; u < n_u; ++u) {
                const uint64_t p = jobs[jb].uprefix[u];
                int q = 0;
                while (q < n_q && pre[q] != p) ++q;
                if (q == n_q) pre[n_q++] = p;
                row_of[u] = q;
            }
            n_q_s = n_q;
        }
        __syncthreads();
    }
    const int n_q = PASS0 ? 1 : n_q_s;  // <= n_u
    for (int i = threadIdx.x; i < n_q * 256; i += PB) hist[i] = 0u;
    __syncthreads();
    const double* __restrict__ row = series + (size_t)t * n_cells;
    const int sh_d = 56 - 8 * pass;  // the digit's shift
    auto count = [&](double v) {
        uint64_t key;
        if (!key_of(v, key)) return;
        const uint32_t d = uint32_t(key >> sh_d) & 255u;
        if (PASS0) {
            atomicAdd(&hist[d], 1u);
        } else {
            const uint64_t hi = key >> (sh_d + 8);  // sh_d + 8 <= 56
            for (int q = 0; q < n_q; ++q)
                if (hi == pre[q]) atomicAdd(&hist[q * 256 + d], 1u);
        }
    };
    int32_t k = cb + (int32_t)threadIdx.x;
    for (; k + 3 * PB < ce; k += 4 * PB) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = row[ID ? k + u * PB : seg_cells[k + u * PB]];
#pragma unroll
        for (int u = 0; u < 4; ++u) count(v[u]);
    }
    for (; k < ce; k += PB) count(row[ID ? k : seg_cells[k]]);
    __syncthreads();
    uint32_t* g = ghist + (size_t)jb * rows * 256;
    for (int i = threadIdx.x; i < n_u * 256; i += PB) {
        const uint32_t n = hist[(PASS0 ? 0 : row_of[i >> 8]) * 256 + (i & 255)];
        if (n) atomicAdd(&g[i], n);
    }
}

static_assert(PB == SCAN_BLOCK, "block_scan takes a workgroup of PB lanes");

// One workgroup per job, one lane per digit value. Pass 0: the finite count, the plan of every percentile, the distinct
// ranks; every pass: the digit bucket each rank falls in. The histogram rows are zeroed for the next pass.
__global__ __launch_bounds__(PB) void pct_pick_kernel(int pass, int rows, pct_list pl, pct_job* jobs,
                                                      uint32_t* __restrict__ ghist) {
    __shared__ uint32_t wtot[PB / 64];
    __shared__ pct_job js;
    const int jb = blockIdx.x;
    uint32_t* g = ghist + (size_t)jb * rows * 256;
    const int d = threadIdx.x;
    if (pass == 0) {
        const uint32_t n = g[d];
        g[d] = 0u;
        uint32_t total;
        const uint32_t ex = block_scan(n, op_add(), 0u, wtot, total) - n;  // exclusive
        if (threadIdx.x == 0) {
            js.nf = total;
            int n_u = 0;
            const int ns = total > 0x7fffffffu ? 0x7fffffff : (int)total;
            for (int i = 0; i < pl.n; ++i) {
                const pct_plan q = pct_make_plan(pl.p[i], ns);
                js.lo_u[i] = js.hi_u[i] = -1;
                if (q.kind != PCT_SINGLE && q.kind != PCT_LERP) continue;
                for (int s = 0; s < (q.kind == PCT_LERP ? 2 : 1); ++s) {
                    const uint32_t rank = s ? q.hi : q.lo;
                    int u = 0;
                    while (u < n_u && js.urank[u] != rank) ++u;
                    if (u == n_u && n_u < PCT_SEL) {
                        js.urank[u] = rank;
                        ++n_u;
                    }
                    if (s) js.hi_u[i] = u < n_u ? u : 0;
                    else js.lo_u[i] = u < n_u ? u : 0;
                }
            }
            js.n_u = n_u;
        }
        __syncthreads();
        const int n_u = js.n_u;
        for (int u = 0; u < n_u; ++u) {
            const uint32_t rank = js.urank[u];  // < total
            if (n > 0u && ex <= rank && rank - ex < n) {
                jobs[jb].urank[u] = rank - ex;
                jobs[jb].uprefix[u] = (uint64_t)d;
            }
        }
        if (threadIdx.x == 0) {
            jobs[jb].nf = js.nf;
            jobs[jb].n_u = n_u;
        }
        if ((int)threadIdx.x < PCT_MAX) {
            jobs[jb].lo_u[threadIdx.x] = (int)threadIdx.x < pl.n ? js.lo_u[threadIdx.x] : -1;
            jobs[jb].hi_u[threadIdx.x] = (int)threadIdx.x < pl.n ? js.hi_u[threadIdx.x] : -1;
        }
        return;
    }
    int n_u = jobs[jb].n_u;
    if (n_u > rows) n_u = rows;
    for (int u = 0; u < n_u; ++u) {
        const uint32_t n = g[u * 256 + d];
        g[u * 256 + d] = 0u;
        uint32_t rank = jobs[jb].urank[u];  // every lane reads before the scan's barriers, one writes after them
        const uint64_t prefix = jobs[jb].uprefix[u];
        uint32_t total;
        const uint32_t ex = block_scan(n, op_add(), 0u, wtot, total) - n;  // exclusive
        if (total > 0u && rank >= total) rank = total - 1u;  // never: the rank lies inside its bucket
        if (n > 0u && ex <= rank && rank - ex < n) {
            jobs[jb].urank[u] = rank - ex;
            jobs[jb].uprefix[u] = (prefix << 8) | (uint64_t)d;
        }
    }
}

// After the last pass uprefix[u] is the whole key of rank u. One lane per (job, percentile).
__global__ __launch_bounds__(PB) void pct_finish_kernel(int job0, int n_jobs, int n_steps, pct_list pl,
                                                        const pct_job* __restrict__ jobs, double* __restrict__ out) {
    const int i = blockIdx.x * PB + threadIdx.x;
    if (i >= n_jobs * pl.n) return;
    const int jb = i / pl.n, ip = i - jb * pl.n;
    const int job = job0 + jb;
    const int c = job / n_steps, t = job - c * n_steps;
    const uint32_t nf = jobs[jb].nf;
    const pct_plan q = pct_make_plan(pl.p[ip], nf > 0x7fffffffu ? 0x7fffffff : (int)nf);
    if (q.kind == PCT_AVG) return;  // pct_average_kernel writes these
    double r = rs_nan();
    if (q.kind != PCT_NAN) {
        int lu = jobs[jb].lo_u[ip], hu = jobs[jb].hi_u[ip];
        lu = lu < 0 ? 0 : (lu >= PCT_SEL ? PCT_SEL - 1 : lu);
        hu = hu < 0 ? lu : (hu >= PCT_SEL ? PCT_SEL - 1 : hu);
        r = pct_value(q, value_of(jobs[jb].uprefix[lu]), value_of(jobs[jb].uprefix[hu]));
    }
    out[((size_t)c * pl.n + ip) * n_steps + t] = r;
}

}  // namespace

size_t percentiles_job_bytes(int n_pct) { return sizeof(pct_job) + size_t(2 * n_pct) * 256 * sizeof(uint32_t); }

hipError_t launch_percentiles(const double* series, size_t n_cells, size_t n_steps, const int32_t* seg_cells,
                              const int32_t* seg_off, size_t n_seg, size_t max_count, const pct_list& pl, int path,
                              void* ws, size_t ws_bytes, double* out, hipStream_t stream) {
    if (n_steps == 0 || n_seg == 0 || pl.n <= 0) return hipSuccess;
    if (pl.n > PCT_MAX || n_steps * n_seg > (size_t)INT32_MAX || max_count > (size_t)INT32_MAX) return hipErrorInvalidValue;
    const int jobs = int(n_steps * n_seg), T = int(n_steps);
    const bool id = seg_cells == nullptr;
    bool any_avg = false, any_sel = false;
    for (int i = 0; i < pl.n; ++i) (pl.p[i] == -1 ? any_avg : any_sel) = true;
    if (any_avg) {
        if (id) hipLaunchKernelGGL((pct_average_kernel<true>), dim3(jobs), dim3(PB), 0, stream, series, n_cells, T, seg_cells, seg_off, pl, out);
        else hipLaunchKernelGGL((pct_average_kernel<false>), dim3(jobs), dim3(PB), 0, stream, series, n_cells, T, seg_cells, seg_off, pl, out);
    }
    if (!any_sel) return hipGetLastError();
    if (path == SHYFT_HIP_PERCENTILES_LDS_SORT) {
        if (max_count > (size_t)SHYFT_HIP_PERCENTILES_LDS_MAX) return hipErrorInvalidValue;
        int P = 1;
        while ((size_t)P < max_count) P <<= 1;
        const size_t lds = size_t(P) * sizeof(uint64_t) + 16;  // keys + the finite counter
        if (id) hipLaunchKernelGGL((pct_lds_sort_kernel<true>), dim3(jobs), dim3(PB), lds, stream, series, n_cells, T, seg_cells, seg_off, pl, P, out);
        else hipLaunchKernelGGL((pct_lds_sort_kernel<false>), dim3(jobs), dim3(PB), lds, stream, series, n_cells, T, seg_cells, seg_off, pl, P, out);
        return hipGetLastError();
    }
    if (path != SHYFT_HIP_PERCENTILES_RADIX) return hipErrorInvalidValue;
    const int rows = 2 * pl.n;
    const size_t per_job = percentiles_job_bytes(pl.n);
    size_t batch = ws_bytes / per_job;
    if (batch > 65535) batch = 65535;  // grid.y
    if (!ws || batch == 0) return hipErrorInvalidValue;
    pct_job* d_jobs = static_cast<pct_job*>(ws);
    // the histogram block follows the job block (sizeof(pct_job) is a multiple of 8)
    uint32_t* d_hist = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(ws) + batch * sizeof(pct_job));
    const unsigned chunks = unsigned(std::max<size_t>(1, (max_count + PCT_CHUNK - 1) / PCT_CHUNK));
    for (int j0 = 0; j0 < jobs; j0 += int(batch)) {
        const int nj = std::min<int>(int(batch), jobs - j0);
        hipError_t e = hipMemsetAsync(ws, 0, batch * per_job, stream);
        if (e != hipSuccess) return e;
        for (int pass = 0; pass < 8; ++pass) {
            const dim3 grid(chunks, (unsigned)nj);
            const size_t lds = size_t(pass == 0 ? 1 : rows) * 256 * sizeof(uint32_t);
            if (pass == 0) {
                if (id) hipLaunchKernelGGL((pct_hist_kernel<true, true>), grid, dim3(PB), lds, stream, series, n_cells, T, seg_cells, seg_off, j0, pass, rows, d_jobs, d_hist);
                else hipLaunchKernelGGL((pct_hist_kernel<false, true>), grid, dim3(PB), lds, stream, series, n_cells, T, seg_cells, seg_off, j0, pass, rows, d_jobs, d_hist);
            } else {
                if (id) hipLaunchKernelGGL((pct_hist_kernel<true, false>), grid, dim3(PB), lds, stream, series, n_cells, T, seg_cells, seg_off, j0, pass, rows, d_jobs, d_hist);
                else hipLaunchKernelGGL((pct_hist_kernel<false, false>), grid, dim3(PB), lds, stream, series, n_cells, T, seg_cells, seg_off, j0, pass, rows, d_jobs, d_hist);
            }
            hipLaunchKernelGGL(pct_pick_kernel, dim3((unsigned)nj), dim3(PB), 0, stream, pass, rows, pl, d_jobs, d_hist);
        }
        const unsigned fin = unsigned((size_t(nj) * pl.n + PB - 1) / PB);
        hipLaunchKernelGGL(pct_finish_kernel, dim3(fin), dim3(PB), 0, stream, j0, nj, T, pl, d_jobs, out);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

// The host restatement (no device call): per step drop the non-finite samples, full sort, then every entry as
// calculate_percentiles_excel_method_full_sort does (time_series_statistics.h:115-160), AVERAGE summed sequentially
// over the sorted samples (:127-132); the extremes are the smallest / largest finite sample (:25-39, :221-226).
void percentiles_host(const double* rows, size_t n_steps, size_t n_per_step, const int64_t* pct, size_t n_pct,
                      double* dst) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> samples;
    samples.reserve(n_per_step);
    for (size_t t = 0; t < n_steps; ++t) {
        samples.clear();
        for (size_t i = 0; i < n_per_step; ++i) {
            const double v = rows[t * n_per_step + i];
            if (std::isfinite(v)) samples.push_back(v);
        }
        const int n_samples = (int)samples.size();
        std::sort(samples.begin(), samples.end());
        for (size_t k = 0; k < n_pct; ++k) {
            const int64_t i = pct[k];
            double r = nan;
            if (n_samples == 0) {
                r = nan;
            } else if (i == -1) {
                double sum = 0;
                for (double x : samples) sum += x;
                r = sum / n_samples;
            } else if (i == -1000) {
                r = samples.front();
            } else if (i == 1000) {
                r = samples.back();
            } else if (i >= 0 && i <= 100) {
                const double eps = 1e-30;
                double nd = 1.0 + (n_samples - 1) * double(i) / 100.0;
                int n = int(nd);
                double delta = nd - n;
                --n;
                if (n <= 0 && delta <= eps) {
                    r = samples.front();
                } else if (n >= n_samples) {
                    r = samples.back();
                } else if (delta < eps) {
                    r = samples[n];
                } else {
                    const double lower = samples[n];
                    if (n < n_samples - 1) n++;
                    const double upper = samples[n];
                    r = lower + delta * (upper - lower);
                }
            }
            dst[k * n_steps + t] = r;
        }
    }
}
