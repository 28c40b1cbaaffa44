// Quantile mapping of weighted forecasts onto historical scenarios for gfx950 (core/time_series_qm.h:34-351).
//
// B independent problems share the time axis, the weights and the shapes: fc [B][T][F], pri [B][T][P], out [B][T][P],
// w [F], mode [T], interp_weight [T]. One job is one (problem, step); its F and P values are contiguous. The host
// decides from the times what a step is (host/qm.hpp step_modes): PRIOR (the row is copied), QM or QM_BLEND; the
// kernel never sees a time. A job without a finite forecast is a copy too (time_series_qm.h:328, :345-347).
//
// Per job (host/qm.hpp map_step is the same arithmetic in plain C++, and the definition of correct):
//  1. the finite forecasts and the finite scenarios are compacted into LDS as (order key, series index) pairs: the
//     order-preserving key of device/workgroup.h, -0.0 given the key of +0.0 so that zeros tie;
//  2. both sets are bitonic-sorted lexicographically by (key, index). The index breaks every tie, so the order is
//     total and the network's instability cannot show: ties go by ascending series index, as on the host. Values are
//     read back through the index, never through the key;
//  3. one lane forms w_sum, the normalised weights and the cum (or mid and width) prefix arrays sequentially in rank
//     order, one rounded add each, exactly as the host does: a parallel scan would reassociate the sums;
//  4. every scenario rank i finds its j by binary search in that array (it is non-decreasing: the weights are > 0),
//     evaluates the quantile and the blend as written in host/qm.hpp (no FMA: -ffp-contract=off) and stores to
//     out[idx_i]; scenarios that are not finite at the step get NaN.
//
// Two launch shapes. WAVE: the padded max(F, P) is at most 64, one wavefront per job, four jobs per 256-lane
// workgroup, each with its own LDS slice; its lanes synchronise with a fence and a wave barrier, never with a
// workgroup barrier, so a wave whose job is past the end or is a copy leaves alone. GROUP: one workgroup per job, up to
// SHYFT_HIP_QM_MAX_SERIES series; every exit is uniform over the workgroup. No floating-point atomics; the only
// atomics are the two integer slot counters of the compaction, whose order the sort removes.
//
// Index safety: SF and SP are the powers of two >= F and P, and the LDS arrays have SF and SP slots; the compaction
// takes at most F <= SF and P <= SP slots; a sort runs over the power of two >= the finite count, which is <= SF or
// SP (lds_sort_pad and lds_bitonic_sort, device/workgroup.h, state their own reads), and its padding pairs (key and
// index all ones) sort last and are never read: only ranks < nf and < np are.
// Series indexes in LDS are loop indexes < F or < P. The rank j of a quantile is clamped to nf - 1, and j - 1 is read
// only when j > 0. A job with no finite forecast copies its row and a job with no finite scenario writes NaNs: neither
// reaches the prefix arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../device/workgroup.h"
#include "../host/qm.hpp"
#include "../include_internal/device_call.h"

using namespace shyft_hip_impl;

namespace {

constexpr int QM_BLOCK = 256;                 // 4 wavefronts
constexpr int QM_WAVE_JOBS = QM_BLOCK / 64;   // jobs per workgroup on the WAVE path

struct qm_args {
    size_t jobs;  // B * T
    size_t T, F, P;
    int SF, SP;   // powers of two >= max(F, 1), P
    const double* fc;
    const double* w;
    const double* pri;
    const int32_t* mode;
    const double* interp_weight;
    int interpolated;
    double* out;
};

// LDS of one job: fa, fval, fwid [SF] double, fkey [SF], pkey [SP] u64, fidx [SF], pidx [SP] u32, two counters
__host__ __device__ inline size_t qm_job_bytes(int SF, int SP) {
    const size_t b = size_t(SF) * (4 * 8 + 4) + size_t(SP) * (8 + 4) + 8;
    return (b + 15) & ~size_t(15);
}

// key_of with the zeros merged; false for NaN and +-inf
__device__ inline bool qm_key_of(double v, uint64_t& key) {
    if ((uint64_t)__double_as_longlong(v) == RS_SIGN) v = 0.0;  // -0.0 ties with +0.0
    return key_of(v, key);
}

template <bool WAVE>
__global__ __launch_bounds__(QM_BLOCK) void qm_kernel(qm_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qm_smem[];
    const int nt = WAVE ? 64 : QM_BLOCK;
    const int tid = WAVE ? int(threadIdx.x & 63) : int(threadIdx.x);
    const size_t job = WAVE ? size_t(blockIdx.x) * QM_WAVE_JOBS + (threadIdx.x >> 6) : size_t(blockIdx.x);
    if (job >= a.jobs) return;  // WAVE: the whole wavefront; GROUP: never
    const int F = int(a.F), P = int(a.P);
    const size_t t = job % a.T;
    const double* __restrict__ fc = a.fc + job * a.F;
    const double* __restrict__ pri = a.pri + job * a.P;
    double* __restrict__ out = a.out + job * a.P;
    const int mode = a.mode[t];

    unsigned char* base = qm_smem + (WAVE ? size_t(threadIdx.x >> 6) * qm_job_bytes(a.SF, a.SP) : size_t(0));
    double* fa = reinterpret_cast<double*>(base);   // cum[j+1] or mid[j]
    double* fval = fa + a.SF;                       // value(j)
    double* fwid = fval + a.SF;                     // w[idx_j], then width[j]
    uint64_t* fkey = reinterpret_cast<uint64_t*>(fwid + a.SF);
    uint64_t* pkey = fkey + a.SF;
    uint32_t* fidx = reinterpret_cast<uint32_t*>(pkey + a.SP);
    uint32_t* pidx = fidx + a.SF;
    uint32_t* cnt = pidx + a.SP;

    if (mode != SHYFT_HIP_QM_PRIOR) {  // uniform over the job
        if (tid == 0) cnt[0] = cnt[1] = 0u;
        lds_sync<WAVE>();
        for (int i = tid; i < F; i += nt) {
            uint64_t key;
            if (qm_key_of(fc[i], key)) {
                const uint32_t pos = atomicAdd(&cnt[0], 1u);  // < F <= SF
                fkey[pos] = key;
                fidx[pos] = uint32_t(i);
            }
        }
        for (int i = tid; i < P; i += nt) {
            uint64_t key;
            if (qm_key_of(pri[i], key)) {
                const uint32_t pos = atomicAdd(&cnt[1], 1u);  // < P <= SP
                pkey[pos] = key;
                pidx[pos] = uint32_t(i);
            }
        }
        lds_sync<WAVE>();
    }
    const int nf = mode != SHYFT_HIP_QM_PRIOR ? int(cnt[0]) : 0;
    if (nf == 0) {  // time_series_qm.h:345-347
        for (int i = tid; i < P; i += nt) out[i] = pri[i];
        return;
    }
    const int np = int(cnt[1]);
    for (int i = tid; i < P; i += nt) {
        uint64_t key;
        if (!qm_key_of(pri[i], key)) out[i] = rs_nan();
    }
    if (np == 0) return;
    const int QF = lds_sort_pad<true>(fkey, fidx, nf, tid, nt), QP = lds_sort_pad<true>(pkey, pidx, np, tid, nt);  // <= SF, SP
    lds_sync<WAVE>();
    lds_bitonic_sort<WAVE, true>(fkey, fidx, QF, tid, nt);  // ascending by (key, index)
    lds_bitonic_sort<WAVE, true>(pkey, pidx, QP, tid, nt);
    for (int j = tid; j < nf; j += nt) {
        const uint32_t ix = fidx[j];  // < F
        fval[j] = fc[ix];
        fwid[j] = a.w[ix];
    }
    lds_sync<WAVE>();
    if (tid == 0) {  // sequential in rank order (wvo_accessor, time_series_qm.h:197-208; :88-98, :146-153)
        double w_sum = 0.0;
        for (int j = 0; j < nf; ++j) w_sum += fwid[j];
        if (!a.interpolated) {
            double c = 0.0;
            for (int j = 0; j < nf; ++j) {
                c = c + fwid[j] / w_sum;
                fa[j] = c;
            }
        } else {
            double mid = 0.0, w_j = 0.0;
            for (int j = 0; j < nf; ++j) {
                double width = 0.5 * w_j;
                w_j = fwid[j] / w_sum;
                width += 0.5 * w_j;
                mid += width;
                fa[j] = mid;
                fwid[j] = width;
            }
        }
    }
    lds_sync<WAVE>();
    const double q_step = 1.0 / double(np - 1);  // inf for one quantile, q_i NaN then
    const double iw = a.interp_weight[t];
    for (int i = tid; i < np; i += nt) {
        const double q_i = q_step * double(i);
        double q;
        if (!a.interpolated) {  // first j with !(cum[j+1] < q_i)
            const int lo = first_false(0, nf, [&](int m) { return fa[m] < q_i; });
            q = fval[lo < nf - 1 ? lo : nf - 1];
        } else if (np == 1) {
            q = fval[0];
        } else {
            // first j with mid[j] > q_i
            const int lo = first_false(0, nf, [&](int m) { return !(fa[m] > q_i); });
            const int j = lo < nf - 1 ? lo : nf - 1;
            if (j == 0 || (j == nf - 1 && q_i >= fa[j])) {
                q = fval[j];
            } else {
                const double interp_start = fval[j - 1];
                const double interp_end = fval[j];
                const double inclination = (interp_end - interp_start) / fwid[j];
                const double offset = fa[j] - fwid[j];
                q = interp_start + inclination * (q_i - offset);
            }
        }
        const uint32_t k = pidx[i];  // < P
        out[k] = mode == SHYFT_HIP_QM_BLEND ? (1.0 - iw) * q + iw * pri[k] : q;
    }
}

// argument checks shared by the device and the host entry; true when there is nothing to do
bool qm_prepare(const char* who, size_t B, size_t T, size_t F, size_t P, const double* fc, const double* w,
                const double* pri, const int32_t* mode, const double* interp_weight, const double* out, bool device) {
    if (device && (F > size_t(SHYFT_HIP_QM_MAX_SERIES) || P > size_t(SHYFT_HIP_QM_MAX_SERIES)))
        throw std::runtime_error("quantile_map: at most " + std::to_string(SHYFT_HIP_QM_MAX_SERIES) +
                                 " forecasts and scenarios on the device");
    if (B == 0 || T == 0 || P == 0) return true;
    const size_t max_elements = std::numeric_limits<size_t>::max() / sizeof(double);
    if (B > max_elements / T || B * T > max_elements / P || (F && B * T > max_elements / F))
        throw std::runtime_error("quantile_map: the batch is too large");
    if ((F && (!fc || !w)) || !pri || !mode || !interp_weight || !out)
        throw std::runtime_error(std::string(who) + ": null argument");
    for (size_t i = 0; i < F; ++i)
        if (!(std::isfinite(w[i]) && w[i] > 0.0)) throw std::runtime_error("quantile_map: every weight must be finite and > 0");
    for (size_t t = 0; t < T; ++t)
        if (mode[t] != SHYFT_HIP_QM_PRIOR && mode[t] != SHYFT_HIP_QM_QM && mode[t] != SHYFT_HIP_QM_BLEND)
            throw std::runtime_error("quantile_map: mode must be PRIOR, QM or QM_BLEND");
    return false;
}

call_record g_qm;
constexpr const char* QM_UPLOAD = "quantile_map upload";

}  // namespace

extern "C" {

int shyft_hip_quantile_map(int device, size_t B, size_t T, size_t F, size_t P, const double* fc, const double* w,
                           const double* pri, const int32_t* mode, const double* interp_weight,
                           int interpolated_quantiles, double* out) {
    try {
        if (qm_prepare("shyft_hip_quantile_map", B, T, F, P, fc, w, pri, mode, interp_weight, out, true)) return 0;
        if (F == 0) {  // no forecast at any step: every step keeps its scenarios (time_series_qm.h:345-347)
            std::memcpy(out, pri, B * T * P * sizeof(double));
            return 0;
        }
        if (B * T > size_t(std::numeric_limits<int>::max()))
            throw std::runtime_error("quantile_map: too many (problem, step) jobs for one launch");
        device_call c(device);
        dbuf<double> d_fc, d_w, d_pri, d_iw, d_out;
        dbuf<int32_t> d_mode;
        c.upload(d_fc, fc, B * T * F, QM_UPLOAD);
        c.upload(d_w, w, F, QM_UPLOAD);
        c.upload(d_pri, pri, B * T * P, QM_UPLOAD);
        c.upload(d_mode, mode, T, QM_UPLOAD);
        c.upload(d_iw, interp_weight, T, QM_UPLOAD);
        d_out.alloc(B * T * P);
        qm_args a{};
        a.jobs = B * T;
        a.T = T;
        a.F = F;
        a.P = P;
        a.SF = 1;
        a.SP = 1;
        while (size_t(a.SF) < F) a.SF <<= 1;
        while (size_t(a.SP) < P) a.SP <<= 1;
        a.fc = d_fc.p;
        a.w = d_w.p;
        a.pri = d_pri.p;
        a.mode = d_mode.p;
        a.interp_weight = d_iw.p;
        a.interpolated = interpolated_quantiles ? 1 : 0;
        a.out = d_out.p;
        const bool wave = a.SF <= 64 && a.SP <= 64;
        const size_t job_bytes = qm_job_bytes(a.SF, a.SP);  // <= 48 KiB + 16 at the cap
        c.begin();
        if (wave) {
            const unsigned grid = unsigned((a.jobs + QM_WAVE_JOBS - 1) / QM_WAVE_JOBS);
            hipLaunchKernelGGL(qm_kernel<true>, dim3(grid), dim3(QM_BLOCK), QM_WAVE_JOBS * job_bytes, c.s, a);
        } else {
            hipLaunchKernelGGL(qm_kernel<false>, dim3(unsigned(a.jobs)), dim3(QM_BLOCK), job_bytes, c.s, a);
        }
        hip_check(hipGetLastError(), "quantile_map");
        g_qm.finish(c, "quantile_map", out, d_out.p, B * T * P, wave ? SHYFT_HIP_QM_PATH_WAVE : SHYFT_HIP_QM_PATH_GROUP);
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_quantile_map_host(size_t B, size_t T, size_t F, size_t P, const double* fc, const double* w,
                                const double* pri, const int32_t* mode, const double* interp_weight,
                                int interpolated_quantiles, double* out) {
    try {
        if (qm_prepare("shyft_hip_quantile_map_host", B, T, F, P, fc, w, pri, mode, interp_weight, out, false)) return 0;
        shyft_hip::host::qm::step_scratch scratch;
        for (size_t job = 0; job < B * T; ++job) {
            const size_t t = job % T;
            shyft_hip::host::qm::map_step(F, P, F ? fc + job * F : nullptr, w, pri + job * P, mode[t], interp_weight[t],
                                          interpolated_quantiles != 0, out + job * P, scratch);
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_quantile_map_last_path(int device) { return g_qm.last_path.load(device, SHYFT_HIP_QM_PATH_NONE); }

double shyft_hip_quantile_map_last_ms(int device) { return g_qm.last_ms.load(device, 0.0); }

}  // extern "C"
