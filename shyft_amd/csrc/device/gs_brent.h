// gamma_snow's corr_lwc Brent job (gamma_snow.h:214-227), written for the one solver wavefront that runs it.
//
// In the pt_gs_k kernels a workgroup's Brent jobs are solved by one wavefront while the workgroup's other
// wavefronts wait at a barrier (kernels/ptgsk.hip), so the job is a latency problem: a lone wavefront issues about
// one instruction per 4-7 cycles whatever the instruction, so the solve costs its instruction count. This is the
// same arithmetic as gs_corr_lwc (device/ptgsk_dev.h) -- the same Brent iterations (boost brent_find_minima), the
// same f = (calc_q(a2, b2, z) - Q1)^2, the same incomplete-gamma terms and detmath exp / log fast paths -- with
// fewer instructions around it:
//  - no calls: exp, log, the series and the continued fraction are inline in the one loop;
//  - the polynomial constants of exp and log are read once per job from a constant table into SGPRs and used as
//    SGPR operands of v_fma_f64 (gs_fma_s), instead of two v_mov_b32 per constant per evaluation;
//  - the series and continued fraction run without their 2^-200 rescale test (device/gamma_lean.h): a lane whose
//    evaluation would have rescaled, or that leaves the fast domain (x <= 0, x not normal, a <= 0, |exp argument|
//    > 708), is re-evaluated by the general gs_calc_q.
// Bit-identical to gs_corr_lwc (tests: test_ptgsk_parity.py, tools/mb/mb_brent.cpp's device check).
#pragma once
#include <hip/hip_runtime.h>

#include "ptgsk_dev.h"
#include "gamma_lean.h"

namespace shyft_dev {

// calc_q(a, b, z) = a b P(a+1, z/b) + z (1 - P(a, z/b)) for the fast domain (device/gamma_lean.h); ok = false:
// take gs_calc_q
__device__ __forceinline__ double gsb_calc_q(double a, double b, double z, double lga, double eps, double ap1,
                                             const gsb_k& k, bool& ok) {
    const gamma_p_result g = gsb_gamma_pq(a, z / b, lga, eps, ap1, k, ok);
    return a * b * g.p1 + z * (1.0 - g.p);
}

// the general evaluation, out of line (rare: Q1 without the opening state's gamma pair, or a lane outside the
// fast domain)
__device__ __noinline__ double gs_calc_q_general(double a, double b, double z, double lga) {
    return gs_calc_q(a, b, z, lga);
}

// f = (calc_q(a2, b2, z) - Q1)^2 of the job, fast path with the general fallback
struct gsb_f {
    double a2, b2, lga2, Q1, eps, ap1;
    bool a_ok;
    gsb_k k;
    __device__ __forceinline__ gsb_f(double z1, double a1, double b1, double a2_, double b2_, double q1, double lga2_)
        : a2(a2_), b2(b2_), lga2(lga2_) {
        Q1 = q1 == q1 ? q1 : gs_calc_q_general(a1, b1, z1, dlgamma(a1));
        k = gsb_load();
        eps = detmath::gamma_snow_policy_eps(a2);
        ap1 = a2 + 1.0;
        a_ok = a2 > 0.0;
    }
    // with Q1 already formed
    __device__ __forceinline__ gsb_f(double a2_, double b2_, double lga2_, double Q1_)
        : a2(a2_), b2(b2_), lga2(lga2_), Q1(Q1_) {
        k = gsb_load();
        eps = detmath::gamma_snow_policy_eps(a2);
        ap1 = a2 + 1.0;
        a_ok = a2 > 0.0;
    }
    __device__ __forceinline__ double operator()(double z) const {
        bool ok;
        double cq = gsb_calc_q(a2, b2, z, lga2, eps, ap1, k, ok);
        if (!(ok && a_ok)) cq = gs_calc_q_general(a2, b2, z, lga2);  // the general path (rare)
        const double v = cq - Q1;
        return v * v;
    }
};

// Speculative opening of the Brent search (small regions, where the solve is a latency problem). The first three
// points boost's brent_find_minima evaluates do not depend on f's values: x = w = v = z1 opens; iteration 1 takes
// the golden step u1 (delta2 starts at 0); iteration 2's parabola through (z1, u1) is degenerate whichever of
// f(u1) <= f(z1) holds (r == q, so p = q = 0 and the golden step is taken again), so its point is u2a (x = u1,
// max = z1) or u2b (x = z1, min = u1). gs_brent_point gives point k of {z1, u1, u2a, u2b} by the solver's own
// formulas; four lanes evaluate f at the four points at once and the solver then looks each of its f arguments up
// among them (bitwise) before evaluating. f is a pure function of its argument, so a hit returns the same bits;
// where an assumption fails (non-finite f values, an early exit) the argument simply misses and is evaluated.
__device__ __forceinline__ double gs_brent_point(double z1, int k) {
    const double tolerance = 0x1p-11;
    const double golden = (double)0.3819660f;
    auto golden_step = [&](double x, double lo, double hi) {
        const double mid = (lo + hi) / 2;
        const double fract1 = tolerance * fabs(x) + tolerance / 4;
        const double d2 = (x >= mid) ? lo - x : hi - x;
        const double delta = golden * d2;
        return (fabs(delta) >= fract1) ? (x + delta) : (delta > 0 ? x + fabs(fract1) : x - fabs(fract1));
    };
    if (k == 0) return z1;
    const double u1 = golden_step(z1, 0.0, z1);
    if (k == 1) return u1;
    double lo = 0.0, hi = z1, x = z1;
    if (k == 2) {  // f(u1) <= f(z1): x = u1, the old x bounds the side u1 moved from
        if (u1 >= x) lo = x; else hi = x;
        x = u1;
    } else {  // f(u1) > f(z1): u1 bounds its side
        if (u1 < x) lo = u1; else hi = u1;
    }
    return golden_step(x, lo, hi);
}

struct gsb_zf {
    double z, f;
};
__device__ __noinline__ gsb_zf gs_corr_lwc_spec(double z1, double a1, double b1, double a2, double b2, double q1,
                                                double lga2, int k) {
    const gsb_f f(z1, a1, b1, a2, b2, q1, lga2);
    gsb_zf r;
    r.z = gs_brent_point(z1, k);
    r.f = f(r.z);
    return r;
}

struct gsb_memo {
    double z[4], f[4];
};

template <bool MEMO>
__device__ __forceinline__ double gs_corr_lwc_lean_t(double z1, double a1, double b1, double a2, double b2, double q1,
                                                     double lga2, const gsb_memo* memo) {
#ifdef SHYFT_ABLATE_BRENT
    return z1 * 0.5;  // instruction-budget ablation only (wrong results)
#endif
    const gsb_f fe(z1, a1, b1, a2, b2, q1, lga2);
    gsb_memo mm;
    if (MEMO) mm = *memo;
    auto f = [&](double z) {
        if (MEMO) {
            const long long zb = __double_as_longlong(z);
            bool hit = false;
            double r = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (!hit && zb == __double_as_longlong(mm.z[i])) { hit = true; r = mm.f[i]; }
            if (hit) return r;
        }
        return fe(z);
    };
    double min = 0.0, max = z1;
    const double tolerance = 0x1p-11;  // ldexp(1, 1-12)
    const double golden = (double)0.3819660f;
    double x, w, v, u, delta, delta2, fu, fv, fw, fx, mid, fract1, fract2;
    x = w = v = max;
    fw = fv = fx = f(x);
    delta2 = delta = 0;
    int count = 60;
    do {
        mid = (min + max) / 2;
        fract1 = tolerance * fabs(x) + tolerance / 4;
        fract2 = 2 * fract1;
        if (fabs(x - mid) <= (fract2 - (max - min) / 2)) break;
        if (fabs(delta2) > fract1) {
            double r = (x - w) * (fx - fv);
            double q = (x - v) * (fx - fw);
            double p = (x - v) * q - (x - w) * r;
            q = 2 * (q - r);
            if (q > 0) p = -p;
            q = fabs(q);
            double td = delta2;
            delta2 = delta;
            if ((fabs(p) >= fabs(q * td / 2)) || (p <= q * (min - x)) || (p >= q * (max - x))) {
                delta2 = (x >= mid) ? min - x : max - x;
                delta = golden * delta2;
            } else {
                delta = p / q;
                u = x + delta;
                if (((u - min) < fract2) || ((max - u) < fract2)) delta = (mid - x) < 0 ? -fabs(fract1) : fabs(fract1);
            }
        } else {
            delta2 = (x >= mid) ? min - x : max - x;
            delta = golden * delta2;
        }
        u = (fabs(delta) >= fract1) ? (x + delta) : (delta > 0 ? x + fabs(fract1) : x - fabs(fract1));
        fu = f(u);
        if (fu <= fx) {
            if (u >= x) min = x; else max = x;
            v = w; w = x; x = u;
            fv = fw; fw = fx; fx = fu;
        } else {
            if (u < x) min = u; else max = u;
            if ((fu <= fw) || (w == x)) {
                v = w; w = u; fv = fw; fw = fu;
            } else if ((fu <= fv) || (v == x) || (v == w)) {
                v = u; fv = fu;
            }
        }
    } while (--count);
    return x;
}

__device__ __noinline__ double gs_corr_lwc_lean(double z1, double a1, double b1, double a2, double b2, double q1,
                                                double lga2) {
    return gs_corr_lwc_lean_t<false>(z1, a1, b1, a2, b2, q1, lga2, nullptr);
}

__device__ __noinline__ double gs_corr_lwc_memo(double z1, double a1, double b1, double a2, double b2, double q1,
                                                double lga2, const gsb_memo& memo) {
    return gs_corr_lwc_lean_t<true>(z1, a1, b1, a2, b2, q1, lga2, &memo);
}

// ---- the job entry of the 256-lane instances: the opening on the solving wavefront's idle lanes.
//
// The workgroup's job queue is one LDS array [GSQ_ROWS][B] (kernels/ptgsk.hip). A group of L = 4 or 2 neighbouring
// lanes of the solving wavefront (lanes L j .. L j + L - 1, in hardware lane order) enters with job j; L = 1 is one
// lane per job without an opening. Lane k of the group evaluates f at gs_brent_point(z1, k) -- one pass of the
// wavefront for the points that brent_find_minima would visit in two (L = 2) or three (L = 4) -- the group's first
// lane takes the siblings' (z, f) by cross-lane reads, the siblings return, and the first lane runs the solver from
// its first iteration: in iteration 1 (and 2 when L = 4) fu is the sibling's f when u's bits equal the sibling's
// point; otherwise the lane leaves the peeled iterations as it entered that iteration and the loop evaluates f(u)
// as ever. f is a pure function of its argument, so a hit is the same bits and a wrong guess is only a miss. The
// loop that follows the peeled iterations is gs_corr_lwc_lean's with its live state (no memo). The result goes to
// row GSQ_RES of job j. Every lane of a group must enter together (the cross-lane reads return 0 from a lane that
// is not executing).
enum { GSQ_Z1, GSQ_A1, GSQ_B1, GSQ_A2, GSQ_B2, GSQ_Q1, GSQ_LG2, GSQ_RES, GSQ_ROWS };
typedef __attribute__((address_space(3))) double gsq_lds;

// brent_find_minima's iteration on the solver's local variables, in two halves (statement macros: the state stays
// in registers): up to its point u (go = false: the tolerance test ended the search), and from fu = f(u) on
#define GSB_NEXT_POINT(go)                                                                                          \
    do {                                                                                                            \
        mid = (min + max) / 2;                                                                                      \
        fract1 = tolerance * fabs(x) + tolerance / 4;                                                               \
        fract2 = 2 * fract1;                                                                                        \
        go = !(fabs(x - mid) <= (fract2 - (max - min) / 2));                                                        \
        if (!go) break;                                                                                             \
        if (fabs(delta2) > fract1) {                                                                                \
            double r = (x - w) * (fx - fv);                                                                         \
            double q = (x - v) * (fx - fw);                                                                         \
            double p = (x - v) * q - (x - w) * r;                                                                   \
            q = 2 * (q - r);                                                                                        \
            if (q > 0) p = -p;                                                                                      \
            q = fabs(q);                                                                                            \
            double td = delta2;                                                                                     \
            delta2 = delta;                                                                                         \
            if ((fabs(p) >= fabs(q * td / 2)) || (p <= q * (min - x)) || (p >= q * (max - x))) {                    \
                delta2 = (x >= mid) ? min - x : max - x;                                                            \
                delta = golden * delta2;                                                                            \
            } else {                                                                                                \
                delta = p / q;                                                                                      \
                u = x + delta;                                                                                      \
                if (((u - min) < fract2) || ((max - u) < fract2))                                                   \
                    delta = (mid - x) < 0 ? -fabs(fract1) : fabs(fract1);                                           \
            }                                                                                                       \
        } else {                                                                                                    \
            delta2 = (x >= mid) ? min - x : max - x;                                                                \
            delta = golden * delta2;                                                                                \
        }                                                                                                           \
        u = (fabs(delta) >= fract1) ? (x + delta) : (delta > 0 ? x + fabs(fract1) : x - fabs(fract1));              \
    } while (0)
#define GSB_TAKE()                                                                                                  \
    do {                                                                                                            \
        if (fu <= fx) {                                                                                             \
            if (u >= x) min = x; else max = x;                                                                      \
            v = w; w = x; x = u;                                                                                    \
            fv = fw; fw = fx; fx = fu;                                                                              \
        } else {                                                                                                    \
            if (u < x) min = u; else max = u;                                                                       \
            if ((fu <= fw) || (w == x)) {                                                                           \
                v = w; w = u; fv = fw; fw = fu;                                                                     \
            } else if ((fu <= fv) || (v == x) || (v == w)) {                                                        \
                v = u; fv = fu;                                                                                     \
            }                                                                                                       \
        }                                                                                                           \
    } while (0)

// lanes per job in a workgroup-step with nj jobs. MODE 2: four with at most 16 jobs, two with at most 32, else one;
// MODE 1: four or one; MODE 0: one
template <int MODE>
__device__ __forceinline__ int gs_brent_group(int nj) {
    return (MODE >= 1 && nj <= 16) ? 4 : (MODE >= 2 && nj <= 32) ? 2 : 1;
}

// t: the lane in the solver's lane order (kernels/ptgsk.hip), L: the step's lanes per job (uniform). The caller
// enters with the lanes t < L nj.
template <int B>
__device__ __noinline__ void gs_brent_job_open(gsq_lds* jq_, int t, int L_) {
    // (the queue's base and L are uniform: scalar registers)
    const int L = __builtin_amdgcn_readfirstlane(L_);
    gsq_lds* const jq = (gsq_lds*)(uintptr_t)__builtin_amdgcn_readfirstlane((int)(uintptr_t)jq_);
    const int j = L == 4 ? t >> 2 : L == 2 ? t >> 1 : t;
    const double z1 = jq[GSQ_Z1 * B + j];
#ifdef SHYFT_ABLATE_BRENT
    if (((int)__lane_id() & (L - 1)) == 0) jq[GSQ_RES * B + j] = z1 * 0.5;  // instruction-budget ablation only (wrong results)
    return;
#endif
    const gsb_f fe(z1, jq[GSQ_A1 * B + j], jq[GSQ_B1 * B + j], jq[GSQ_A2 * B + j], jq[GSQ_B2 * B + j],
                   jq[GSQ_Q1 * B + j], jq[GSQ_LG2 * B + j]);
    double min = 0.0, max = z1;
    const double tolerance = 0x1p-11;  // ldexp(1, 1-12)
    const double golden = (double)0.3819660f;
    double x, w, v, u, delta, delta2, fu, fv, fw, fx, mid, fract1, fract2;
    x = w = v = max;
    delta2 = delta = 0;
    // the job index above the iteration count: one register in the loop
    static_assert(B <= (1 << 16), "job index field");
    int count = (j << 8) | 60;
    bool go = true;
    {
        // the opening: lane k at point k, then the siblings' points and values to the group's first lane
        const int lane = (int)__lane_id(), k = lane & (L - 1), g0 = lane & ~(L - 1);  // (L = 1: point 0)
        u = gs_brent_point(z1, k);
        fu = fe(u);
        double sz1 = 0.0, sf1 = 0.0, sz2 = 0.0, sf2 = 0.0, sz3 = 0.0, sf3 = 0.0;
        if (L >= 2) {
            sz1 = __shfl(u, g0 + 1);
            sf1 = __shfl(fu, g0 + 1);
        }
        if (L == 4) {
            sz2 = __shfl(u, g0 + 2);
            sf2 = __shfl(fu, g0 + 2);
            sz3 = __shfl(u, g0 + 3);
            sf3 = __shfl(fu, g0 + 3);
        }
        if (k != 0) return;
        fw = fv = fx = fu;  // x = w = v = z1 = u
        // the peeled iterations. A miss puts delta and delta2 back and leaves: the loop below then forms the same u
        // from the same state and evaluates it
        if (L >= 2) do {
            GSB_NEXT_POINT(go);  // iteration 1: u1
            if (!go) break;
            if (__double_as_longlong(u) != __double_as_longlong(sz1)) {
                delta2 = delta = 0;
                break;
            }
            fu = sf1;
            GSB_TAKE();
            --count;
            if (L == 4) {
                const double d = delta, d2 = delta2;
                GSB_NEXT_POINT(go);  // iteration 2: u2a or u2b
                if (!go) break;
                if (__double_as_longlong(u) == __double_as_longlong(sz2)) fu = sf2;
                else if (__double_as_longlong(u) == __double_as_longlong(sz3)) fu = sf3;
                else {
                    delta = d;
                    delta2 = d2;
                    break;
                }
                GSB_TAKE();
                --count;
            }
        } while (0);
    }
    if (go) do {  // gs_corr_lwc_lean's loop
        GSB_NEXT_POINT(go);
        if (!go) break;
        // a2 + 1 and the policy eps are formed again in each trip (the same values) instead of being held across
        // the loop: the two registers that otherwise make the allocator spill one of f's constants to scratch and
        // reload it in every trip
        double a2o = fe.a2;
        asm volatile("" : "+v"(a2o));
        gsb_f fl = fe;
        fl.ap1 = a2o + 1.0;
        fl.eps = detmath::gamma_snow_policy_eps(a2o);
        fu = fl(u);
        GSB_TAKE();
    } while (--count & 0xff);
    jq[GSQ_RES * B + (count >> 8)] = x;
}
#undef GSB_NEXT_POINT
#undef GSB_TAKE

}  // namespace shyft_dev
