// The incomplete gamma of gamma_snow (boost gamma_p with the digits10<5>/<10> policy, gamma_snow.h:189-201, as
// detmath::gamma_pq restates it) in fewer instructions, for the fast domain -- shape a > 0, x positive normal,
// |a log x - x - lgamma(a)| <= 708 -- where it is bit-identical to detmath::gamma_pq<dev_math>:
//  - exp and log are inline (detmath's |x| <= 708 / positive-normal fast paths), their polynomial constants read
//    once from a constant table into SGPRs and used as SGPR operands of v_fma_f64 (gs_fma_s), no call;
//  - the series and the continued fraction run without their 2^-200 rescale test: with a > 0 the series'
//    E = (a+1)...(a+n) only grows, so a final E <= 2^200/... proves no term rescaled; the fraction's largest |P| is
//    kept with a max (no per-term branch) and checked after the loop. An evaluation that would have rescaled, or
//    that leaves the fast domain, is redone by the general detmath evaluation.
// Used by the Brent job of device/gs_brent.h (its f), by calc_snow_state (device/ptgsk_dev.h) and by Skaugen's
// sca_rel_red (device/ptssk_dev.h); exp_fast / log_fast are the kernels' inline exp / log (device/pt_dev.h kmath).
#pragma once
#include <hip/hip_runtime.h>

#include "special.h"

namespace shyft_dev {

// dexp / dlog bit for bit: the fast paths of device/fastmath.h inline, the out-of-line general function beyond them
__device__ __forceinline__ double exp_fast(double x, const gsb_k& k) {
    double r = gsb_exp(x, k);
    if (!(__builtin_fabs(x) <= 708.0)) r = dexp(x);
    return r;
}
__device__ __forceinline__ double log_fast(double x, const gsb_k& k) {
    double r = gsb_log(x, k);
    if (!(x >= 2.2250738585072014e-308 && x <= 1.7976931348623157e308)) r = dlog(x);
    return r;
}

// SHYFT_GAMMA_LOOPS: how the two term loops below are controlled. 0: the C++ loops, as the compiler lowers a loop
// that lanes leave at different terms (a per-lane down-counter for the 2,000-term cap and five or more scalar
// instructions per term that gather the lanes that have left; the fraction unrolled by five into nested exec regions).
// Bit 0 (the series) and bit 1 (the fraction): the same terms -- the same floating-point instructions on the same
// operands in the same order -- in a hand-written loop of two terms per trip: the term's compare writes the exec
// mask itself (v_cmpx), so a lane that has met its own tolerance simply stops executing and keeps the values of the
// term it left at, and one branch per term leaves when no lane is left. The 2,000-term cap is wave-uniform: a scalar
// counter of trips in the series (999 down to the borrow: 1,000 trips), one compare of the fraction's own term
// count per trip (every lane still in the loop has the same count). exec is saved on entry and restored on exit.
// Nothing inside the statements needs a wait state: no instruction reads vcc or an SGPR that a VALU instruction has
// just written, and the branches read exec, which needs none (DESIGN.md 3.1 has the per-term counts).
#ifndef SHYFT_GAMMA_LOOPS
#define SHYFT_GAMMA_LOOPS 3
#endif

#if SHYFT_GAMMA_LOOPS
// one series term: ap += 1, xn *= x, E *= ap, B = fma(B, ap, xn), then continue while !(xn < eps (E + B))
#define GSB_SERIES_TERM                                 \
    "v_add_f64 %[ap], %[ap], 1.0\n\t"                   \
    "v_mul_f64 %[xn], %[x], %[xn]\n\t"                  \
    "v_mul_f64 %[E], %[E], %[ap]\n\t"                   \
    "v_fma_f64 %[B], %[B], %[ap], %[xn]\n\t"            \
    "v_add_f64 %[s], %[E], %[B]\n\t"                    \
    "v_mul_f64 %[t], %[eps], %[s]\n\t"                  \
    "v_cmpx_nlt_f64_e32 vcc, %[xn], %[t]\n\t"

// detmath::gamma_series_sums without the rescale test, from n = 1: E = (a+1)...(a+n), B = sum of x^k (a+k+1)...(a+n),
// and the last term's E + B
__device__ __forceinline__ void gsb_series_loop(double a, double x, double eps, double& E_, double& B_, double& S_) {
    double ap = a, E = 1.0, B = 0.0, xn = 1.0, s, t;
    unsigned long long live;
    unsigned pairs;
    asm volatile(
        "s_mov_b64 %[live], exec\n\t"
        "s_movk_i32 %[pairs], 999\n"
        ".Lgsb_series_%=:\n\t"
        GSB_SERIES_TERM
        "s_cbranch_execz .Lgsb_series_done_%=\n\t"
        GSB_SERIES_TERM
        "s_sub_u32 %[pairs], %[pairs], 1\n\t"
        "s_cbranch_scc1 .Lgsb_series_done_%=\n\t"  // the 2,000-term cap
        "s_cbranch_execnz .Lgsb_series_%=\n"
        ".Lgsb_series_done_%=:\n\t"
        "s_mov_b64 exec, %[live]"
        : [ap] "+v"(ap), [xn] "+v"(xn), [E] "+v"(E), [B] "+v"(B), [s] "=&v"(s), [t] "=&v"(t),
          [live] "=&s"(live), [pairs] "=&s"(pairs)
        : [x] "v"(x), [eps] "v"(eps)
        : "vcc", "scc");
    E_ = E;
    B_ = B;
    S_ = s;
}

// one continued-fraction term. PM / P and QM / QD are the previous and the current convergent's numerator and
// denominator; the new ones are written over the previous ones, so the next term takes the roles swapped and no
// register moves. Continue while !(|Pn Qd - P Qn| <= eps |Pn Qd|); the largest |P| takes the new P only in the
// lanes that continue (exec is already theirs).
#define GSB_CF_TERM(PM, P, QM, QD)                                  \
    "v_add_f64 %[di], %[di], 1.0\n\t"                               \
    "v_add_f64 %[t], %[di], -%[a]\n\t"                              \
    "v_mul_f64 %[t], %[t], -%[di]\n\t"                              \
    "v_add_f64 %[bcf], %[bcf], 2.0\n\t"                             \
    "v_mul_f64 %[" PM "], %[t], %[" PM "]\n\t"                      \
    "v_mul_f64 %[" QM "], %[" QM "], %[t]\n\t"                      \
    "v_fma_f64 %[" PM "], %[bcf], %[" P "], %[" PM "]\n\t"          \
    "v_fma_f64 %[" QM "], %[bcf], %[" QD "], %[" QM "]\n\t"         \
    "v_mul_f64 %[t], %[" QD "], %[" PM "]\n\t"                      \
    "v_mul_f64 %[u], %[" P "], %[" QM "]\n\t"                       \
    "v_add_f64 %[u], %[t], -%[u]\n\t"                               \
    "v_mul_f64 %[t], %[eps], |%[t]|\n\t"                            \
    "v_cmpx_nle_f64_e64 vcc, |%[u]|, %[t]\n\t"

// detmath::gamma_cf_terms with the rescale test folded into the largest |P| (bigP), from i = 1 with bcf = x + 1 - a
__device__ __forceinline__ void gsb_cf_loop(double a, double eps, double bcf, double& P_, double& Qd_, double& bigP_) {
    double pa = 1.0, pb = bcf, qa = 0.0, qb = 1.0, di = 0.0, bigP = 0.0, t, u;
    unsigned long long live;
    asm volatile(
        "s_mov_b64 %[live], exec\n"
        ".Lgsb_cf_%=:\n\t"
        GSB_CF_TERM("pa", "pb", "qa", "qb")  // odd terms: the new P, Qd in pa, qa
        "s_cbranch_execz .Lgsb_cf_done_%=\n\t"
        "v_max_f64 %[big], %[big], |%[pa]|\n\t"
        GSB_CF_TERM("pb", "pa", "qb", "qa")  // even terms: in pb, qb
        "v_max_f64 %[big], %[big], |%[pb]|\n\t"
        "v_cmpx_gt_f64_e32 vcc, 2000.0, %[di]\n\t"  // the 2,000-term cap (di is the same in every lane still here)
        "s_cbranch_execnz .Lgsb_cf_%=\n"
        ".Lgsb_cf_done_%=:\n\t"
        "s_mov_b64 exec, %[live]"
        : [pa] "+v"(pa), [pb] "+v"(pb), [qa] "+v"(qa), [qb] "+v"(qb), [di] "+v"(di), [bcf] "+v"(bcf),
          [big] "+v"(bigP), [t] "=&v"(t), [u] "=&v"(u), [live] "=&s"(live)
        : [a] "v"(a), [eps] "v"(eps)
        : "vcc");
    // di is the lane's own term count (it stopped with the lane): odd, the lane left at an odd term
    const bool odd = ((int)di & 1) != 0;
    P_ = odd ? pa : pb;
    Qd_ = odd ? qa : qb;
    bigP_ = bigP;
}
#undef GSB_SERIES_TERM
#undef GSB_CF_TERM
#endif

// P(a, x), P(a+1, x) and the prefix by detmath::gamma_pq's series / continued fraction for the fast domain;
// ok = false: the caller takes the general evaluation (the value returned is then meaningless)
__device__ __forceinline__ gamma_p_result gsb_gamma_pq(double a, double x, double lga, double eps, double ap1,
                                                       const gsb_k& k, bool& ok) {
    const double lx = gsb_log(x, k);
    const double arg = a * lx - x - lga;
    ok = a > 0.0 && x >= 2.2250738585072014e-308 && x <= 1.7976931348623157e308 && __builtin_fabs(arg) <= 708.0;
    const double prefix = gsb_exp(arg, k);
    gamma_p_result r;
    r.prefix = prefix;
    r.p = r.p1 = 0.0;
    if (!ok) return r;  // (x = inf or NaN would not converge: no loop for a lane outside the domain)
    if (x < ap1) {
        // series (detmath::gamma_series_sums without the rescale test)
#if SHYFT_GAMMA_LOOPS & 1
        double E, B, S;
        gsb_series_loop(a, x, eps, E, B, S);
#else
        double ap = a, E = 1.0, B = 0.0, xn = 1.0;
        for (int n = 1; n <= 2000; ++n) {
            ap = ap + 1.0;
            xn = xn * x;
            E = E * ap;
            B = __builtin_fma(B, ap, xn);
            if (xn < eps * (B + E)) break;
        }
#endif
        ok = ok && E <= detmath::GPQ_SCALE_HI;
        const double aE = a * E;
#if SHYFT_GAMMA_LOOPS & 1
        const double pp = prefix * (S / aE);  // S = E + B of the lane's last term (the loop's own sum: the same bits)
#else
        const double pp = prefix * ((B + E) / aE);
#endif
        const double pp1 = prefix * (B / aE);
        r.p = pp < 1.0 ? pp : 1.0;
        r.p1 = pp1 < 1.0 ? pp1 : 1.0;
    } else {
        // continued fraction (detmath::gamma_cf_terms; the rescale test folded into the largest |P|)
#if SHYFT_GAMMA_LOOPS & 2
        double P, Qd, bigP;
        gsb_cf_loop(a, eps, x + 1.0 - a, P, Qd, bigP);
#else
        double bcf = x + 1.0 - a;
        double Pm = 1.0, Qm = 0.0, P = bcf, Qd = 1.0, di = 0.0, bigP = 0.0;
        for (int i = 1; i <= 2000; ++i) {
            di = di + 1.0;
            const double an = -di * (di - a);
            bcf = bcf + 2.0;
            const double Pn = __builtin_fma(bcf, P, an * Pm);
            const double Qn = __builtin_fma(bcf, Qd, an * Qm);
            const double cross = Pn * Qd;
            const double diff = cross - P * Qn;
            Pm = P; Qm = Qd;
            P = Pn; Qd = Qn;
            if (__builtin_fabs(diff) <= eps * __builtin_fabs(cross)) break;
            bigP = __builtin_fmax(bigP, __builtin_fabs(P));  // NaN P: no rescale there either
        }
#endif
        ok = ok && !(bigP > detmath::GPQ_SCALE_HI);
        const double q = prefix * (Qd / P);
        const double q1 = q + prefix / a;
        const double pp = 1.0 - q;
        const double pp1 = 1.0 - q1;
        r.p = pp > 0.0 ? pp : 0.0;
        r.p1 = pp1 > 0.0 ? pp1 : 0.0;
    }
    return r;
}

// the general evaluation (detmath::gamma_pq with the out-of-line exp / log), out of line
__device__ __noinline__ gamma_p_result gs_gamma_pq_general(double a, double x, double lga) {
    return gamma_p_prefix(a, x, lga, detmath::gamma_snow_policy_eps(a));
}

}  // namespace shyft_dev
