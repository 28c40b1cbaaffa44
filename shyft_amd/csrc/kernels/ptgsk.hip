// pt_gs_k cell kernel for gfx950.
//
// region_model::run_cells -> cell::run -> run_pt_gs_k (core/region_model.h:578-597,
// core/pt_gs_k_cell_model.h:243-262, core/pt_gs_k.h:312-398) for every cell of
// the region in ONE launch: lane = cell, the time loop runs inside the kernel
// with the cell state held in registers, forcing read [step][cell] (coalesced,
// 512 B per wave per variable per step) and collector series written
// [series][step][cell].
//
// Brent compaction (COMPACT = true): gamma_snow's corr_lwc Brent minimisation
// (gamma_snow.h:425-435) costs ~30 incomplete-gamma evaluations and fires for a
// random ~10% of cells on a snowfall step, so nearly every wavefront would run
// it for a few lanes. Each step the workgroup queues its lanes' Brent jobs in LDS
// and the first ceil(jobs/64) wavefronts solve them (one job per lane), then
// every lane picks up its own result. Results are bit-identical to the
// per-lane version: the same function on the same arguments.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../device/ptgsk_dev.h"
#include "../device/gs_brent.h"
#include "../device/stream.h"
#include "../device/wave_place.h"
#include "../include_internal/kernels.h"
#include "../../../include/shyft_hip.h"

using namespace shyft_dev;

// the Brent job of the solving wavefront: gs_corr_lwc_lean (device/gs_brent.h), the arithmetic of the
// reference-shaped gs_corr_lwc (device/ptgsk_dev.h) in fewer instructions
#define GS_BRENT_JOB gs_corr_lwc_lean

#ifdef SHYFT_PROF
// phase timing (profiling builds only): per-wavefront s_memtime deltas summed over the launch
__device__ unsigned long long g_ptgsk_prof[12];
extern "C" int shyft_ptgsk_prof_read(unsigned long long* out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ptgsk_prof), sizeof(g_ptgsk_prof)) != hipSuccess) return 1;
    unsigned long long z[12] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_ptgsk_prof), z, sizeof z) != hipSuccess;
}
#define PROF_DECL unsigned long long prof_acc[6] = {0, 0, 0, 0, 0, 0}, prof_lg = 0; unsigned long long prof_t = __builtin_amdgcn_s_memtime();
#define PROF_MARK(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); prof_acc[k] += t_ - prof_t; prof_t = t_; } while (0)
#define PROF_FLUSH() do { if ((threadIdx.x & 63) == 0) { for (int k_ = 0; k_ < 6; ++k_) atomicAdd(&g_ptgsk_prof[k_], prof_acc[k_]); atomicAdd(&g_ptgsk_prof[11], prof_lg); } } while (0)
#else
#define PROF_DECL
#define PROF_MARK(k) ((void)0)
#define PROF_FLUSH() ((void)0)
#endif

namespace {

// forcing loads / response stores with the nontemporal hint (device/stream.h). r06, 1M cells, the year in 730-step
// chunks: 74.0 -> 73.1 ms per chunk, January HBM traffic 1.84x -> 1.33x the algorithmic bytes
// (profiles/r06/ptgsk_nt_variants.txt, tools/traffic_variants.sh)
#ifndef SHYFT_PTGSK_NT
#define SHYFT_PTGSK_NT 1
#endif
constexpr bool STREAM_NT = SHYFT_PTGSK_NT != 0;

// (128- and 512-lane workgroups measured 7 % and 4 % slower over the year, r05)
constexpr int BLOCK = 256;

#ifndef SHYFT_LB_WAVES
#define SHYFT_LB_WAVES 4
#endif

// the lean instances (LEAN below) take the discharge-only launches (0: every launch takes the general instance, for
// A/B builds). r06, 1M cells, 20 x 438 steps: 9.81-9.84e9 -> 9.92-9.94e9 cell-steps/s, with machine LICM off for this
// file (Makefile) 10.17-10.25e9, bit-exact (profiles/r06/ptgsk_lean_instance_ab.txt)
#ifndef SHYFT_PTGSK_LEAN
#define SHYFT_PTGSK_LEAN 1
#endif

// issue priority (s_setprio) of the Brent-solving wavefront: 138.2 -> 134.5 ms per chunk (year mean, 1M cells)
constexpr int BRENT_PRIO = 3;

// the lgamma queue of the 256-lane instances (LGQ below; 0: every lane evaluates its new shapes in place, for A/B
// builds), and what a step with queued shapes and no Brent job does: 0, the owners evaluate their own shape in
// place (no second barrier, as without the queue); n > 0, from n queued shapes on all four wavefronts evaluate the
// compacted list and a second barrier follows (profiles/r06/ptgsk_lgamma_queue_ab.txt)
#ifndef SHYFT_PTGSK_LGQ
#define SHYFT_PTGSK_LGQ 1
#endif
#ifndef SHYFT_PTGSK_LGQ_NOBRENT
#define SHYFT_PTGSK_LGQ_NOBRENT 0
#endif
// 1: the lgamma(a2) of a Brent job is evaluated by the wavefront that solves the job, ahead of its solves, and
// written to the owner's cache slot; 0: by every wavefront that holds a job lane, in gs_front (as before the queue).
// r06, 1M cells, 20 x 438 steps, 5 alternating runs: parent 10.212e9 - 10.249e9 cell-steps/s, the queue alone
// 10.321e9 - 10.336e9, with this 10.412e9 - 10.449e9, bit-exact (profiles/r06/ptgsk_lgamma_queue_ab.txt)
#ifndef SHYFT_PTGSK_LGQ_JOBLG
#define SHYFT_PTGSK_LGQ_JOBLG 1
#endif

// the Brent opening on the solving wavefront's idle lanes in the 256-lane instances (gs_brent_job_open,
// device/gs_brent.h): 0, one lane per job whatever the job count (gs_corr_lwc_lean, for A/B builds); 1, four lanes
// per job in a workgroup-step with at most 16 jobs; 2, that and two lanes per job with 17-32 jobs. A step with more
// jobs has one lane per job as before, through the same entry
#ifndef SHYFT_PTGSK_BOPEN
#define SHYFT_PTGSK_BOPEN 2
#endif

// UNIFORM: every cell of the launch uses parameter set 0 (the region parameter, no catchment overrides):
// the parameter row is then wave-uniform and lives in SGPRs (scalar loads), which frees the VGPRs the
// per-lane copies would take in the register-bound time loop.
// ENS: a parameter-ensemble launch (lanes = cells x members): forcing is read from the shared column fcol[lane].
// The per-cell constants and the lane's lgamma cache live in LDS (9 rows, 18 KB per workgroup, 35.3 KB with the job
// queue: 4 workgroups = 16 waves per CU still fit the 160 KB) instead of VGPRs live across the Brent phase. Scratch
// 400 -> 320 B/lane; 124.8 -> 119.1 ms per 1M-cell chunk over the bench year, bit-exact.
// WAVES: the occupancy target. 4 waves per SIMD (128 VGPRs, spilling) is the measured best when the launch fills
// the GPU; a region too small to give every SIMD 4 waves (<= 2 workgroups per CU, e.g. a strong-scaled shard of
// 131K cells) gets the 2-wave instance instead (256 VGPRs, no spills): it cannot be 4-deep anyway.
// B: cells (lanes) per workgroup. SPEC: the speculative Brent opening (device/gs_brent.h), for small regions.
// LEAN: the instance for the common launch (discharge collector only, no state series, no read_delay test knob), as
// in kernels/hbv.hip: it has no code for response series 2-7, the state series or the knob and holds no pointers for
// them, which the general instance keeps in SGPRs (spilled to VGPR lanes) across the whole step loop.
template <bool COMPACT, bool UNIFORM, bool ENS = false, int WAVES = SHYFT_LB_WAVES, int B = BLOCK, bool SPEC = false,
          bool LEAN = false>
__global__ __launch_bounds__(B, WAVES) void ptgsk_run_kernel(const ptgsk_kargs a) {
    static_assert(COMPACT, "the Brent jobs always go through the workgroup queue");
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = cell < a.n_cells;
    if (valid && a.active && !a.active[cell]) valid = false;
    const int lc = valid ? cell : 0;  // out-of-range lanes of a COMPACT block read cell 0 and store nothing
    const size_t N = (size_t)a.n_cells;
    const size_t NF = ENS ? (size_t)a.f_cols : N;
    const size_t fcl = ENS ? (size_t)a.fcol[lc] : (size_t)lc;
    const double* __restrict__ Pg = UNIFORM ? a.params : a.params + (size_t)a.set_ix[lc] * PTGSK_NP;
    // the uniform parameter row in LDS (288 B next to the 35 KB of job queue and cell constants): the step loop
    // reads it with ds_read_b64 where it is used instead of holding 36 doubles in SGPRs, which spilled to VGPR lanes
    // (a v_readlane per use) beside the inline exp / log constant table. r05: 80.8 -> 79.0 ms per 730-step chunk,
    // v_readlane_b32 326 -> 270 in the kernel's code. (Read after the first barrier below.)
    __shared__ double lpar[UNIFORM ? PTGSK_NP : 1];
    if (UNIFORM && threadIdx.x < PTGSK_NP) lpar[threadIdx.x] = a.params[threadIdx.x];
    const double* __restrict__ P = UNIFORM ? (const double*)lpar : Pg;

    // per-cell constants (pt_gs_k.h:347-357)
    const double* __restrict__ cc = a.cellc;
    gs_cell gcell;
    gcell.cv2 = cc[PC_CV2 * N + lc];
    gcell.inv_cv2 = cc[PC_INV_CV2 * N + lc];
    // the cell constants live in LDS, not in VGPRs: each use reloads its lane's slot (the barriers of the
    // step keep the compiler from hoisting the loads), so none of them is live across the Brent phase
    // rows 0-6: the cell constants; rows 7-8: the lane's lgamma cache (shape, value), so that every per-lane LDS
    // slot is one address register plus an immediate offset. Two constants are formed from the others with the
    // host's own expressions (region.hip update_derived): kirchner_fraction = 1 - direct_response_fraction and
    // glacier_area_m2 = area * glacier, the same operations on the same doubles
    __shared__ double lcc[9][B];
    {
        const int t = threadIdx.x;
        lcc[0][t] = gcell.cv2;
        lcc[1][t] = gcell.inv_cv2;
        lcc[2][t] = cc[PC_GLACIER * N + lc];
        lcc[3][t] = cc[PC_SNOW_STORAGE * N + lc];
        lcc[4][t] = cc[PC_KIRCHNER_ROUTED_PREC * N + lc];
        lcc[5][t] = cc[PC_DIRECT_RESPONSE * N + lc];
        lcc[6][t] = cc[PC_AREA * N + lc];
    }
#define glacier_fraction (lcc[2][threadIdx.x])
#define snow_storage_fraction (lcc[3][threadIdx.x])
#define kirchner_routed_prec (lcc[4][threadIdx.x])
#define direct_response_fraction (lcc[5][threadIdx.x])
#define kirchner_fraction (1 - lcc[5][threadIdx.x])                   // PC_KIRCHNER_FRACTION = 1 - direct
#define cell_area_m2 (lcc[6][threadIdx.x])
#define glacier_area_m2 (lcc[6][threadIdx.x] * lcc[2][threadIdx.x])  // PC_GLACIER_AREA = area * glacier
#define LOAD_GCELL()                                   \
    do {                                               \
        gcell.cv2 = lcc[0][threadIdx.x];               \
        gcell.inv_cv2 = lcc[1][threadIdx.x];           \
    } while (0)

    const double mmh_to_m3s_scale_factor = 1 / (3600.0 * 1000.0);

    // state -> registers
    double* __restrict__ st = a.state;
    gs_state s;
    s.albedo = st[PS_ALBEDO * N + lc];
    s.lwc = st[PS_LWC * N + lc];
    s.surface_heat = st[PS_SURFACE_HEAT * N + lc];
    s.alpha = st[PS_ALPHA * N + lc];
    s.sdc_melt_mean = st[PS_SDC_MELT_MEAN * N + lc];
    s.acc_melt = st[PS_ACC_MELT * N + lc];
    s.iso_pot_energy = st[PS_ISO_POT_ENERGY * N + lc];
    s.temp_swe = st[PS_TEMP_SWE * N + lc];
    double q = st[PS_KIRCHNER_Q * N + lc];
    lcc[7][threadIdx.x] = -1.0;  // the lgamma cache (device/ptgsk_dev.h)
    lcc[8][threadIdx.x] = 0.0;
    constexpr bool LGQ = SHYFT_PTGSK_LGQ != 0 && B == 256 && !SPEC;
    constexpr bool JOBLG = LGQ && SHYFT_PTGSK_LGQ_JOBLG != 0;
    constexpr int BOPEN = (B == 256 && !SPEC) ? SHYFT_PTGSK_BOPEN : 0;
    lgamma_cache_lds<JOBLG> lgc{lcc[7], lcc[8]};
    gs_carry carry;
    int32_t err = 0;

    const size_t TW = (size_t)a.win_len;
    const double* __restrict__ f_temp = a.forcing + (size_t)FV_TEMPERATURE * TW * NF;
    const double* __restrict__ f_prec = a.forcing + (size_t)FV_PRECIPITATION * TW * NF;
    const double* __restrict__ f_ws = a.forcing + (size_t)FV_WIND_SPEED * TW * NF;
    const double* __restrict__ f_rh = a.forcing + (size_t)FV_REL_HUM * TW * NF;
    const double* __restrict__ f_rad = a.forcing + (size_t)FV_RADIATION * TW * NF;
    double* __restrict__ R = a.resp;
    const size_t RS = TW * N;  // stride between response series
    double* __restrict__ SS = LEAN ? nullptr : a.state_series;
    const size_t SSS = (TW + 1) * N;
    const int wed = (int)Pg[PK_WED];
    const int64_t snow_lo = (int64_t)((int)(Pg[PK_WED] * 24) - (int)(Pg[PK_NWD] * 24)) * 3600000000LL;
    const int64_t snow_hi = (int64_t)(int)(Pg[PK_WED] * 24) * 3600000000LL;

    // Brent job queue of the workgroup (COMPACT)
    // (jres is not aliased with a job array: a lane reads its result after the step's second barrier, and another
    // wavefront may already be enqueueing the next step's jobs by then)
    // (the 256-lane instances: one array, rows GSQ_* of device/gs_brent.h, whose base gs_brent_job_open takes. The
    // 64-lane instance keeps its eight arrays: with one array its code needs 168 VGPRs instead of 175, which lets a
    // third wavefront onto a SIMD, and a small region's two workgroups per SIMD then spread unevenly: 25 % slower at
    // 131,072 cells)
    __shared__ double jq[SPEC ? 1 : GSQ_ROWS][SPEC ? 1 : B];
    __shared__ double sz1[SPEC ? B : 1], sa1[SPEC ? B : 1], sb1[SPEC ? B : 1], sa2[SPEC ? B : 1], sb2[SPEC ? B : 1],
        sq1[SPEC ? B : 1], slg2[SPEC ? B : 1], sres[SPEC ? B : 1];
    double* const jz1 = SPEC ? sz1 : jq[GSQ_Z1];
    double* const ja1 = SPEC ? sa1 : jq[GSQ_A1];
    double* const jb1 = SPEC ? sb1 : jq[GSQ_B1];
    double* const ja2 = SPEC ? sa2 : jq[GSQ_A2];
    double* const jb2 = SPEC ? sb2 : jq[GSQ_B2];
    double* const jq1 = SPEC ? sq1 : jq[GSQ_Q1];
    double* const jlg2 = SPEC ? slg2 : jq[GSQ_LG2];
    double* const jres = SPEC ? sres : jq[GSQ_RES];
    __shared__ double jsz[SPEC ? 64 : 1], jsf[SPEC ? 64 : 1];  // speculative opening: point and f of lane t
    __shared__ int jcount[2];
    // lgamma queue of the workgroup (LGQ): the lanes whose final calc_snow_state of the step will want lgamma of a
    // shape their cache slot does not hold (gs_front's new_shape, device/ptgsk_dev.h). The owner writes the shape
    // into its key slot lcc[7][t] and its lane id into lq; between the step's two barriers the wavefronts that are
    // not solving Brent jobs evaluate dlgamma of the queued shapes, one per lane, into the owners' value slots
    // lcc[8][owner], so the owners' gs_back hits the cache instead of every wavefront running dlgamma for a few
    // of its lanes. Invariant: a slot whose key has been set holds dlgamma(key) by the time its owner next reads it
    // (DESIGN.md 3.1). The same function of the same argument: the same bits as the owner's own evaluation.
    __shared__ unsigned short lq[LGQ ? B : 1];
    __shared__ unsigned short jown[JOBLG ? B : 1];  // JOBLG: the lane that owns job j
    __shared__ int lcount[2];
    __shared__ int wsimd[B / 64];
    publish_wave_simd(wsimd);
    if (COMPACT) {
        if (threadIdx.x == 0) {  // both: the first step may be odd (start_step)
            jcount[0] = jcount[1] = 0;
            if (LGQ) lcount[0] = lcount[1] = 0;
        }
        __syncthreads();
    }
    // the lane that solves job 0: the first lane of the solving wavefront (device/wave_place.h)
    const int jrot = solver_lane0<B>(wsimd);

    auto collect_state = [&](size_t wi) {
        // state_collector::collect of state.scale_snow(snow_storage_fraction)
        SS[0 * SSS + wi * N + cell] = cell_area_m2 * q * mmh_to_m3s_scale_factor;
        SS[1 * SSS + wi * N + cell] = s.albedo;
        SS[2 * SSS + wi * N + cell] = s.lwc * snow_storage_fraction;
        SS[3 * SSS + wi * N + cell] = s.surface_heat;
        SS[4 * SSS + wi * N + cell] = s.alpha;
        SS[5 * SSS + wi * N + cell] = s.sdc_melt_mean;
        SS[6 * SSS + wi * N + cell] = s.acc_melt;
        SS[7 * SSS + wi * N + cell] = s.iso_pot_energy;
        SS[8 * SSS + wi * N + cell] = s.temp_swe * snow_storage_fraction;
    };

    const int i_end = a.step0 + a.n_steps;
    PROF_DECL
    for (int i = a.step0; i < i_end; ++i) {
        const double gm_direct = P[PK_GM_DIRECT];
        const double gm_routed = 1 - gm_direct;
        const double dtf = P[PK_DTF];
        const double p_corr = P[PK_PCORR];
        const double kc1 = P[PK_C1], kc2 = P[PK_C2], kc3 = P[PK_C3];
        const size_t wi = (size_t)(i - a.win0);
        const size_t fo = wi * N + lc;
        const size_t ff = ENS ? wi * NF + fcl : fo;
        double temp = 0, rad = 0, rel_hum = 0, prec = 0, wind_speed = 0;
        if (valid) {
            temp = stream_ld<STREAM_NT && !ENS>(&f_temp[ff]);
            rad = stream_ld<STREAM_NT && !ENS>(&f_rad[ff]);
            rel_hum = stream_ld<STREAM_NT && !ENS>(&f_rh[ff]);
            prec = stream_ld<STREAM_NT && !ENS>(&f_prec[ff]) * p_corr;
            wind_speed = stream_ld<STREAM_NT && !ENS>(&f_ws[ff]);
            if (SS) collect_state(wi);
        }
        const bool start_melt = a.doy[i] == wed;
        const int64_t trel = a.t_rel_year_us[i];
        const bool snow_season = trel >= snow_lo && trel < snow_hi;

        gs_mid m;
        m.need = false;
        m.done = true;
        LOAD_GCELL();
        if (threadIdx.x == 0) {  // next step's counters (race-free: see DESIGN.md)
            jcount[(i + 1) & 1] = 0;
            if (LGQ) lcount[(i + 1) & 1] = 0;
        }
        int slot = -1;
        bool queued = false;  // this lane has a shape in the step's lgamma queue
        auto new_shape = [&](double shape) {
            if (LGQ && shape != lcc[7][threadIdx.x]) {
                lq[atomicAdd(&lcount[i & 1], 1)] = (unsigned short)threadIdx.x;
                lcc[7][threadIdx.x] = shape;
                queued = true;
            }
        };
        // JOBLG: the jobs' lgamma(a2) ahead of the solves, by the lane that solves the job; it also goes to the
        // owner's slot unless the owner has queued another shape since (the keys are final after the first barrier)
        // t: the lane in the solver's lane order (0-63: the solving wavefront, whose hardware lanes they are).
        // With at most 16 (32) jobs the solving wavefront has 4 (2) lanes per job: lane t enters job t / L with its
        // group, which opens the search on its L lanes at once (gs_brent_job_open); the lgamma(a2) of job j has
        // been written by lane j of the same wavefront just before (LDS operations of a wavefront execute in order;
        // the fence keeps the compiler from moving them).
        auto brent_jobs = [&](int t, int nj) {
            if (JOBLG)
                for (int j = t; j < nj; j += B) {
                    const double lga2 = dlgamma(ja2[j]);
                    jlg2[j] = lga2;
                    const int o = jown[j];
                    if (lcc[7][o] == ja2[j]) lcc[8][o] = lga2;
                }
            if (BOPEN) {
                // (a group's lanes are all below 64: L nj <= 64)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                const int L = gs_brent_group<BOPEN>(nj);
                for (int tt = t; tt < L * nj; tt += B) gs_brent_job_open<B>((gsq_lds*)&jq[0][0], tt, L);
                return;
            }
            for (int j = t; j < nj; j += B)
                jres[j] = GS_BRENT_JOB(jz1[j], ja1[j], jb1[j], ja2[j], jb2[j], jq1[j], jlg2[j]);
        };
        // dlgamma of the queued shapes first, first + stride, ... into their owners' value slots
        auto lgamma_jobs = [&](int first, int stride, int nl) {
            for (int j = first; j < nl; j += stride) {
                const int o = lq[j];
                lcc[8][o] = dlgamma(lcc[7][o]);
            }
        };
        // the step's Brent job goes into the queue where gs_front forms it
        auto enqueue = [&](double z1, double a1, double b1, double a2, double b2, double q1, double lga2) {
            slot = atomicAdd(&jcount[i & 1], 1);
            jz1[slot] = z1; ja1[slot] = a1; jb1[slot] = b1; ja2[slot] = a2; jb2[slot] = b2;
            jq1[slot] = q1; jlg2[slot] = lga2;
            if (JOBLG) jown[slot] = (unsigned short)threadIdx.x;
        };
#ifndef SHYFT_ABLATE_SNOW
        if (valid)
            gs_front(s, m, start_melt, a.dt_s, a.dt_us, P, gcell, temp, rad, prec, wind_speed, rel_hum, lgc, carry, enqueue,
                     new_shape);
#endif
        PROF_MARK(0);  // forcing + gs_front
        double z = 0.0;
        {
            __syncthreads();
            PROF_MARK(1);  // job queue + barrier
            // both counts are uniform: written before the barrier above, and not rewritten before the next step's
            // first barrier (thread 0 zeroes the other pair)
            const int nj = jcount[i & 1];
            const int nl = LGQ ? lcount[i & 1] : 0;
            // the wavefronts behind the solving ones (lanes ns .. B-1 in the solver's lane order t) evaluate the
            // queued shapes during the Brent phase, at priority 0; when every wavefront solves, all of them do it
            // after their jobs. Either way before the second barrier, after which the owners read their slots.
            auto lgamma_phase = [&](int t) {
                const int ns = (nj + 63) & ~63;
                if (ns >= B) lgamma_jobs(t, B, nl);
                else if (t >= ns) lgamma_jobs(t - ns, B - ns, nl);
            };
            if (nj > 0) {
#ifdef SHYFT_PROF
                const unsigned long long tb = __builtin_amdgcn_s_memtime();
                if (threadIdx.x < nj) __builtin_amdgcn_s_setprio(BRENT_PRIO);
                brent_jobs((int)threadIdx.x, nj);
                __builtin_amdgcn_s_setprio(0);
                if (threadIdx.x < nj && (threadIdx.x & 63) == 0)
                    atomicAdd(&g_ptgsk_prof[8], (unsigned long long)(__builtin_amdgcn_s_memtime() - tb));
                if (LGQ && nl > 0) {
                    const unsigned long long tl = __builtin_amdgcn_s_memtime();
                    lgamma_phase((int)threadIdx.x);
                    prof_lg += __builtin_amdgcn_s_memtime() - tl;  // ([11]: summed per wavefront, flushed at the end)
                }
#else
                const int t = SPEC ? (int)threadIdx.x : (int)((threadIdx.x - jrot) & (B - 1));
                // the solving wavefront is the workgroup's critical path (its other wavefronts wait at the
                // barrier below): it gets issue priority over the other workgroups' wavefronts on its SIMD
                if (t < nj) __builtin_amdgcn_s_setprio(BRENT_PRIO);
                // the speculative opening when the jobs' point lanes fit the solving wavefront: 4 lanes per job
                // (z1, u1, u2a, u2b: two f rounds saved) or 2 (z1, u1: one round saved)
                const int L = SPEC ? (4 * nj <= 64 ? 4 : 2 * nj <= 64 ? 2 : 0) : 0;
                if (L) {
                    const int jj = L == 4 ? t >> 2 : t >> 1;
                    if (t < 64 && jj < nj) {
                        const gsb_zf r = gs_corr_lwc_spec(jz1[jj], ja1[jj], jb1[jj], ja2[jj], jb2[jj], jq1[jj], jlg2[jj], t & (L - 1));
                        jsz[t] = r.z;
                        jsf[t] = r.f;
                    }
                    __syncthreads();
                    if (t < nj) {
                        gsb_memo mm;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {  // with 2 points, entries 2 and 3 repeat entry 0
                            const int e = L * t + (k < L ? k : 0);
                            mm.z[k] = jsz[e];
                            mm.f[k] = jsf[e];
                        }
                        jres[t] = gs_corr_lwc_memo(jz1[t], ja1[t], jb1[t], ja2[t], jb2[t], jq1[t], jlg2[t], mm);
                    }
                } else {
                    brent_jobs(t, nj);
                }
                __builtin_amdgcn_s_setprio(0);
                if (LGQ && nl > 0) lgamma_phase(t);
#endif
                __syncthreads();
                // test knob: the other wavefronts read their results late, so a fast first wavefront is already
                // enqueueing the next step's jobs (jres must not alias the job arrays for this to stay exact)
                if (!LEAN && a.read_delay > 0 && (threadIdx.x >> 6) != 0)
                    for (int k = 0; k < a.read_delay; ++k) __builtin_amdgcn_s_sleep(127);
                if (slot >= 0) z = jres[slot];
            } else if (LGQ && SHYFT_PTGSK_LGQ_NOBRENT > 0 && nl >= SHYFT_PTGSK_LGQ_NOBRENT) {
                // no Brent job and many shapes: all four wavefronts evaluate the compacted list, then the barrier
                // (a wavefront that reads nl late, after thread 0 zeroed it for the step after next, reads 0 only
                // where the others read less than the threshold: with the barrier here nobody is a step ahead)
                lgamma_jobs((int)threadIdx.x, B, nl);
                __syncthreads();
            } else if (LGQ && queued) {
                // no Brent job: nobody waits, so the owner evaluates its own shape (no second barrier, as before)
                lcc[8][threadIdx.x] = dlgamma(lcc[7][threadIdx.x]);
            }
        }
        PROF_MARK(2);  // Brent phase
        if (!valid) {
            carry = gs_carry();  // (dead: keeps the carry out of the values live across the Brent phase)
            continue;
        }
        double gs_sca, gs_storage, gs_outflow;
        LOAD_GCELL();
#ifdef SHYFT_ABLATE_SNOW  // instruction-budget ablation only (wrong results): no snow routine at all
        gs_sca = 0.0; gs_storage = 0.0; gs_outflow = prec + 0.0 * z;
#else
        gs_back(s, m, z, gs_sca, gs_storage, gs_outflow, snow_season, a.dt_us, P, gcell, prec, lgc, carry);
#endif
        PROF_MARK(3);  // gs_back

        // glacier_melt::step (glacier_melt.h:47-52)
        const double sca_area = cell_area_m2 * gs_sca;
        double gm_melt_m3s = 0.0;
        if (!(glacier_area_m2 <= sca_area || temp <= 0.0))
            gm_melt_m3s = dtf * temp * (glacier_area_m2 - sca_area) * (0.001 / 86400.0);
        // Priestley-Taylor's saturation-pressure exp beside actual_evapotranspiration's exp: kmath<true>::exp2, both
        // inline bodies interleaved in one basic block (device/pt_dev.h)
        double ae_exp;
        const double pot_evap =
            pt_pot_evap_exp<true>(P[PK_PT_ALBEDO], P[PK_PT_ALPHA], temp, rad, rel_hum, -q * 3.0 / P[PK_AE_SCALE], ae_exp) *
            3600.0;
        const double ae = pot_evap * (1.0 - ae_exp) * (1.0 - smax(gs_sca, glacier_fraction));
        const double gm_mmh = gm_melt_m3s / (mmh_to_m3s_scale_factor * cell_area_m2);
        PROF_MARK(4);  // glacier, PT, AE
        double q_avg;
        if (!kirchner_step<true>(q, q_avg, gs_outflow * snow_storage_fraction + prec * kirchner_routed_prec + gm_routed * gm_mmh,
                           ae, a.t1_hours, kc1, kc2, kc3))
            err = ERR_KIRCHNER_MAX_ITER;
        const double total_discharge = smax(0.0, prec - ae) * direct_response_fraction + gm_direct * gm_mmh +
                                       q_avg * kirchner_fraction;
        const double charge_m3s = +(cell_area_m2 * prec * mmh_to_m3s_scale_factor) -
                                  (cell_area_m2 * ae * mmh_to_m3s_scale_factor) + gm_melt_m3s -
                                  (cell_area_m2 * total_discharge * mmh_to_m3s_scale_factor);
        // collectors (pt_gs_k_cell_model.h:80-89, 116-124) of response.scale_snow(snow_storage_fraction)
        stream_st<STREAM_NT>(&R[0 * RS + fo], cell_area_m2 * total_discharge * mmh_to_m3s_scale_factor);
        stream_st<STREAM_NT>(&R[1 * RS + fo], charge_m3s);
        if (!LEAN && a.collect >= 1) {
            R[2 * RS + fo] = gs_sca;
            R[3 * RS + fo] = gs_storage * snow_storage_fraction;
        }
        if (!LEAN && a.collect >= 2) {
            R[4 * RS + fo] = cell_area_m2 * (gs_outflow * snow_storage_fraction) * mmh_to_m3s_scale_factor;
            R[5 * RS + fo] = gm_melt_m3s;
            R[6 * RS + fo] = ae;
            R[7 * RS + fo] = pot_evap;
        }
        if (SS && i + 1 == i_end) collect_state(wi + 1);
        PROF_MARK(5);  // kirchner, outputs
    }
    PROF_FLUSH();
    if (!valid) return;
    st[PS_ALBEDO * N + cell] = s.albedo;
    st[PS_LWC * N + cell] = s.lwc;
    st[PS_SURFACE_HEAT * N + cell] = s.surface_heat;
    st[PS_ALPHA * N + cell] = s.alpha;
    st[PS_SDC_MELT_MEAN * N + cell] = s.sdc_melt_mean;
    st[PS_ACC_MELT * N + cell] = s.acc_melt;
    st[PS_ISO_POT_ENERGY * N + cell] = s.iso_pot_energy;
    st[PS_TEMP_SWE * N + cell] = s.temp_swe;
    st[PS_KIRCHNER_Q * N + cell] = q;
    if (err) a.err[cell] = err;
}
#undef LOAD_GCELL
#undef glacier_fraction
#undef snow_storage_fraction
#undef kirchner_routed_prec
#undef direct_response_fraction
#undef kirchner_fraction
#undef cell_area_m2
#undef glacier_area_m2

// The step's out-of-line device functions (dexp / dexp2 / dlog / dlgamma, the Brent job) are shared by every
// kernel of this file, and the AMDGPU attributor compiles a shared callee for the range of its callers' occupancy.
// This never-launched 8-wave caller makes that range tight: the callees are register-allocated for 64 VGPRs, so
// they clobber fewer registers and the 4-wave step loop keeps more values live across its calls (VGPR spills of
// the bench instance 164 -> 127). Measured on the 1M-cell bench year, 730-step chunks: 105.3 -> 100.0 ms per chunk,
// bit-exact (tools/ptgsk_variants.py). Round 6 re-measured the budget against the current step
// (detmath's one-division log and degree-11 exp): 7 waves (72 VGPRs for the callees) 75.5 -> 74.2 ms per chunk,
// 6 waves 74.8, bit-exact (profiles/r06/ptgsk_budget_variants.txt); the caller spills a few more VGPRs (32 -> 39)
// but saves more in the calls.
#ifndef SHYFT_PTGSK_BUDGET_WAVES
#define SHYFT_PTGSK_BUDGET_WAVES 7
#endif
constexpr int ST_BOPEN = SHYFT_PTGSK_BOPEN ? SHYFT_PTGSK_BOPEN : 2;  // the job entry that the selftest kernel runs
__global__ __launch_bounds__(256, SHYFT_PTGSK_BUDGET_WAVES) void ptgsk_callee_budget_kernel(const ptgsk_kargs a) {
    if (a.n_cells >= 0) return;  // never runs: launch_ptgsk_run only references it
    const int c = threadIdx.x;
    gs_state s{};
    gs_mid m{};
    lgamma_cache lgc;
    gs_carry carry;
    gs_cell gc{};
    double q = a.dt_s, qa = 0.0, sca, sto, outf;
    double j[7] = {};
    gs_front(s, m, c == 0, a.dt_s, a.dt_us, a.params, gc, q, q, q, q, q, lgc, carry,
             [&](double z1, double a1, double b1, double a2, double b2, double q1, double lga2) {
                 j[0] = z1; j[1] = a1; j[2] = b1; j[3] = a2; j[4] = b2; j[5] = q1; j[6] = lga2;
             });
    double z = gs_corr_lwc_lean(j[0], j[1], j[2], j[3], j[4], j[5], j[6]);
    __shared__ double jq[GSQ_ROWS][BLOCK];
    for (int r = 0; r < 7; ++r) jq[r][c] = j[r];
    gs_brent_job_open<BLOCK>((gsq_lds*)&jq[0][0], c, 4);
    z += jq[GSQ_RES][c];
    gs_back(s, m, z, sca, sto, outf, c == 1, a.dt_us, a.params, gc, q, lgc, carry);
    double e;
    const double pe = pt_pot_evap_exp<true>(0.2, 1.26, q, q, q, q, e);
    kirchner_step<true>(q, qa, outf, pe * e, a.t1_hours, -2.4, 0.9, -0.1);
    a.resp[c] = q + qa + sca + sto + s.lwc;
}

// ---- diagnostic kernels (shyft_hip_device_selftest): this file's device functions on chosen inputs, one thread per
// row, in [col][n] -> out [col][n]. They live here so that the out-of-line functions they call (dexp, dlog, dexp2,
// dlgamma, gs_gamma_pq_general, gs_corr_lwc_lean, gs_brent_job_open, gs_corr_lwc_spec ...) are the instances the run
// kernels call, and they carry the occupancy bounds of a kernel that already calls those functions (the callee
// budget kernel's, or the speculative instance's), so the functions are compiled as before.
constexpr int ST_BLOCK = 256;

__global__ __launch_bounds__(ST_BLOCK, SHYFT_PTGSK_BUDGET_WAVES) void ptgsk_st_explog_inline_kernel(
    const double* __restrict__ in, size_t n, double* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)ST_BLOCK + threadIdx.x;
    if (i >= n) return;
    const kmath<true> km;  // the step loop's inline exp / log (device/pt_dev.h)
    const double x = in[i];
    out[i] = km.exp(x);
    out[n + i] = km.log(x);
}

// the step loop's two-argument inline exp and log (kmath<true>::exp2 / log2p: both fast paths side by side, one
// merged test for the general path)
__global__ __launch_bounds__(ST_BLOCK, SHYFT_PTGSK_BUDGET_WAVES) void ptgsk_st_explog_pairs_kernel(
    const double* __restrict__ in, size_t n, double* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)ST_BLOCK + threadIdx.x;
    if (i >= n) return;
    const kmath<true> km;
    const double x = in[i], y = in[n + i];
    const dexp_pair e = km.exp2(x, y);
    const dexp_pair l = km.log2p(x, y);
    out[i] = e.a;
    out[n + i] = e.b;
    out[2 * n + i] = l.a;
    out[3 * n + i] = l.b;
}

__global__ __launch_bounds__(ST_BLOCK, SHYFT_PTGSK_BUDGET_WAVES) void ptgsk_st_explog_calls_kernel(
    const double* __restrict__ in, size_t n, double* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)ST_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double x = in[i], y = in[n + i];
    out[i] = dexp(x);
    out[n + i] = dlog(x);
    const dexp_pair e = dexp2(x, y);
    out[2 * n + i] = e.a;
    out[3 * n + i] = e.b;
}

__global__ __launch_bounds__(ST_BLOCK, SHYFT_PTGSK_BUDGET_WAVES) void ptgsk_st_powers_kernel(
    const double* __restrict__ in, size_t n, double* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)ST_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double x = in[i], y = in[n + i];
    out[i] = dpowr(x, y);
    out[n + i] = dpow4(x);
    out[2 * n + i] = dpow8(x);
    out[3 * n + i] = dpow(x, y);
}

// the lean incomplete gamma's own verdict (ok) beside calc_snow_state's evaluation, which redoes a lane that is not ok
__global__ __launch_bounds__(ST_BLOCK, SHYFT_PTGSK_BUDGET_WAVES) void ptgsk_st_gamma_kernel(
    const double* __restrict__ in, size_t n, double* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)ST_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double a = in[i], x = in[n + i];
    const double lga = dlgamma(a);
    bool ok;
    (void)gsb_gamma_pq(a, x, lga, detmath::gamma_snow_policy_eps(a), a + 1.0, gsb_load(), ok);
    const gamma_p_result r = gs_gamma_pq_cs(a, x, lga);
    out[i] = r.p;
    out[n + i] = r.p1;
    out[2 * n + i] = r.prefix;
    out[3 * n + i] = ok ? 1.0 : 0.0;
}

// Q1 as the job's lane supplies it: NaN (mode 0), or calc_q at the opening point (mode 1)
__device__ __forceinline__ double st_brent_q1(double mode, double z1, double a1, double b1) {
    return mode != 0.0 ? gs_calc_q(a1, b1, z1, dlgamma(a1)) : __builtin_nan("");
}

__global__ __launch_bounds__(ST_BLOCK, SHYFT_PTGSK_BUDGET_WAVES) void ptgsk_st_brent_kernel(
    const double* __restrict__ in, size_t n, double* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)ST_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double z1 = in[i], a1 = in[n + i], b1 = in[2 * n + i], a2 = in[3 * n + i], b2 = in[4 * n + i];
    const double q1 = st_brent_q1(in[5 * n + i], z1, a1, b1);
    const double lga2 = dlgamma(a2);
#ifdef SHYFT_PROF
    int nf_evals = 0;
    out[i] = gs_corr_lwc(z1, a1, b1, a2, b2, q1, lga2, nf_evals);
#else
    out[i] = gs_corr_lwc(z1, a1, b1, a2, b2, q1, lga2);
#endif
    out[n + i] = GS_BRENT_JOB(z1, a1, b1, a2, b2, q1, lga2);
}

// the speculative opening as the small-region instance of ptgsk_run_kernel runs it: one wavefront per workgroup,
// its 64 / L jobs queued in LDS, L point lanes per job, a barrier, then the memo solve by lane t for job t
template <int L>
__global__ __launch_bounds__(64, 2) void ptgsk_st_brent_spec_kernel(const double* __restrict__ in, size_t n,
                                                                    double* __restrict__ out) {
    static_assert(L == 4 || L == 2, "4 or 2 point lanes per job");
    constexpr int JOBS = 64 / L;
    __shared__ double jz1[JOBS], ja1[JOBS], jb1[JOBS], ja2[JOBS], jb2[JOBS], jq1[JOBS], jlg2[JOBS];
    __shared__ double jsz[64], jsf[64];
    const int t = threadIdx.x;
    const size_t j0 = blockIdx.x * (size_t)JOBS;
    const int nj = n - j0 < (size_t)JOBS ? (int)(n - j0) : JOBS;  // the launch has no workgroup beyond the jobs
    if (t < nj) {
        const size_t i = j0 + t;
        jz1[t] = in[i]; ja1[t] = in[n + i]; jb1[t] = in[2 * n + i]; ja2[t] = in[3 * n + i]; jb2[t] = in[4 * n + i];
        jq1[t] = st_brent_q1(in[5 * n + i], jz1[t], ja1[t], jb1[t]);
        jlg2[t] = dlgamma(ja2[t]);
    }
    __syncthreads();
    const int jj = L == 4 ? t >> 2 : t >> 1;
    if (t < 64 && jj < nj) {
        const gsb_zf r = gs_corr_lwc_spec(jz1[jj], ja1[jj], jb1[jj], ja2[jj], jb2[jj], jq1[jj], jlg2[jj], t & (L - 1));
        jsz[t] = r.z;
        jsf[t] = r.f;
    }
    __syncthreads();
    if (t < nj) {
        gsb_memo mm;
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // with 2 points, entries 2 and 3 repeat entry 0
            const int e = L * t + (k < L ? k : 0);
            mm.z[k] = jsz[e];
            mm.f[k] = jsf[e];
        }
        out[j0 + t] = gs_corr_lwc_memo(jz1[t], ja1[t], jb1[t], ja2[t], jb2[t], jq1[t], jlg2[t], mm);
    }
}

// gs_brent_job_open as the 256-lane run kernels call it: a 256-lane workgroup with the [GSQ_ROWS][256] queue, JOBS
// jobs per workgroup (16: groups of 4 lanes; 32: groups of 2), the first wavefront's lanes in groups per job. The
// last workgroup is ragged and takes the group size of its own job count, as a workgroup-step does.
template <int JOBS>
__global__ __launch_bounds__(ST_BLOCK, SHYFT_PTGSK_BUDGET_WAVES) void ptgsk_st_brent_open_kernel(
    const double* __restrict__ in, size_t n, double* __restrict__ out) {
    static_assert(JOBS == 16 || JOBS == 32, "16 or 32 jobs per workgroup");
    __shared__ double jq[GSQ_ROWS][ST_BLOCK];
    const int t = threadIdx.x;
    const size_t j0 = blockIdx.x * (size_t)JOBS;
    const int nj = n - j0 < (size_t)JOBS ? (int)(n - j0) : JOBS;  // the launch has no workgroup beyond the jobs
    if (t < nj) {
        const size_t i = j0 + t;
        jq[GSQ_Z1][t] = in[i]; jq[GSQ_A1][t] = in[n + i]; jq[GSQ_B1][t] = in[2 * n + i];
        jq[GSQ_A2][t] = in[3 * n + i]; jq[GSQ_B2][t] = in[4 * n + i];
        jq[GSQ_Q1][t] = st_brent_q1(in[5 * n + i], jq[GSQ_Z1][t], jq[GSQ_A1][t], jq[GSQ_B1][t]);
        jq[GSQ_LG2][t] = dlgamma(jq[GSQ_A2][t]);
    }
    __syncthreads();
    const int L = gs_brent_group<ST_BOPEN>(nj);
    if (t < L * nj) gs_brent_job_open<ST_BLOCK>((gsq_lds*)&jq[0][0], t, L);
    __syncthreads();
    if (t < nj) out[j0 + t] = jq[GSQ_RES][t];
}

}  // namespace


hipError_t launch_ptgsk_run(const ptgsk_kargs& a, hipStream_t stream) {
    const int grid = (a.n_cells + BLOCK - 1) / BLOCK;
    if (grid == 0) return hipSuccess;
    // workgroups resident at 4 waves per SIMD: 4 per CU (16 waves of 256-lane workgroups)
    int n_cu = 256;
    {
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess) {
            int v = 0;
            if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n_cu = v;
        }
    }
    static const char* force = getenv("SHYFT_PTGSK_WAVES");  // measurement knob: "2" / "4" forces an instance
    const bool small = a.instance ? a.instance == 2 : force ? force[0] == '2' : grid <= 2 * n_cu;
    // the discharge-only launch takes the lean instance; every other combination the general one
    const bool lean = SHYFT_PTGSK_LEAN && a.collect == 0 && !a.state_series && a.read_delay == 0;
    if (a.n_cells < 0)  // never (n_cells > 0): keeps ptgsk_callee_budget_kernel in the module
        hipLaunchKernelGGL(ptgsk_callee_budget_kernel, dim3(1), dim3(BLOCK), 0, stream, a);
    if (a.fcol) {
        hipLaunchKernelGGL((ptgsk_run_kernel<true, false, true>), dim3(grid), dim3(BLOCK), 0, stream, a);
    } else if (small) {
        // small regions: one-wavefront workgroups (each wavefront solves its own ~7 winter Brent jobs: no workgroup
        // barrier wait) with the speculative Brent opening (4 lanes per job, free in a wavefront that has the lanes)
        const int g64 = (a.n_cells + 63) / 64;
        if (lean) {
            if (a.uniform_params) hipLaunchKernelGGL((ptgsk_run_kernel<true, true, false, 2, 64, true, true>), dim3(g64), dim3(64), 0, stream, a);
            else hipLaunchKernelGGL((ptgsk_run_kernel<true, false, false, 2, 64, true, true>), dim3(g64), dim3(64), 0, stream, a);
        } else if (a.uniform_params) hipLaunchKernelGGL((ptgsk_run_kernel<true, true, false, 2, 64, true>), dim3(g64), dim3(64), 0, stream, a);
        else hipLaunchKernelGGL((ptgsk_run_kernel<true, false, false, 2, 64, true>), dim3(g64), dim3(64), 0, stream, a);
    } else if (lean) {
        if (a.uniform_params) hipLaunchKernelGGL((ptgsk_run_kernel<true, true, false, SHYFT_LB_WAVES, BLOCK, false, true>), dim3(grid), dim3(BLOCK), 0, stream, a);
        else hipLaunchKernelGGL((ptgsk_run_kernel<true, false, false, SHYFT_LB_WAVES, BLOCK, false, true>), dim3(grid), dim3(BLOCK), 0, stream, a);
    } else {
        // (the small-region instance's speculative opening -- a memo the step loop loads and hands to the solver, a
        // workgroup barrier between the points and the solve -- measured slower in the 256-lane instances, twice;
        // they open the search inside the job entry instead: gs_brent_job_open)
        if (a.uniform_params) hipLaunchKernelGGL((ptgsk_run_kernel<true, true>), dim3(grid), dim3(BLOCK), 0, stream, a);
        else hipLaunchKernelGGL((ptgsk_run_kernel<true, false>), dim3(grid), dim3(BLOCK), 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_ptgsk_selftest(int fn, const double* in, size_t n, double* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + ST_BLOCK - 1) / ST_BLOCK)), block(ST_BLOCK);
    switch (fn) {
        case SHYFT_HIP_DST_EXPLOG_INLINE: hipLaunchKernelGGL(ptgsk_st_explog_inline_kernel, grid, block, 0, stream, in, n, out); break;
        case SHYFT_HIP_DST_EXPLOG_CALLS: hipLaunchKernelGGL(ptgsk_st_explog_calls_kernel, grid, block, 0, stream, in, n, out); break;
        case SHYFT_HIP_DST_EXPLOG_PAIRS: hipLaunchKernelGGL(ptgsk_st_explog_pairs_kernel, grid, block, 0, stream, in, n, out); break;
        case SHYFT_HIP_DST_POWERS: hipLaunchKernelGGL(ptgsk_st_powers_kernel, grid, block, 0, stream, in, n, out); break;
        case SHYFT_HIP_DST_GAMMA_LEAN: hipLaunchKernelGGL(ptgsk_st_gamma_kernel, grid, block, 0, stream, in, n, out); break;
        case SHYFT_HIP_DST_BRENT: hipLaunchKernelGGL(ptgsk_st_brent_kernel, grid, block, 0, stream, in, n, out); break;
        case SHYFT_HIP_DST_BRENT_SPEC4:  // 16 jobs per one-wavefront workgroup
            hipLaunchKernelGGL(ptgsk_st_brent_spec_kernel<4>, dim3((unsigned)((n + 15) / 16)), dim3(64), 0, stream, in, n, out);
            break;
        case SHYFT_HIP_DST_BRENT_SPEC2:  // 32 jobs
            hipLaunchKernelGGL(ptgsk_st_brent_spec_kernel<2>, dim3((unsigned)((n + 31) / 32)), dim3(64), 0, stream, in, n, out);
            break;
        case SHYFT_HIP_DST_BRENT_OPEN4:  // 16 jobs per workgroup, on its first wavefront
            hipLaunchKernelGGL(ptgsk_st_brent_open_kernel<16>, dim3((unsigned)((n + 15) / 16)), block, 0, stream, in, n, out);
            break;
        case SHYFT_HIP_DST_BRENT_OPEN2:  // 32 jobs
            hipLaunchKernelGGL(ptgsk_st_brent_open_kernel<32>, dim3((unsigned)((n + 31) / 32)), block, 0, stream, in, n, out);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
