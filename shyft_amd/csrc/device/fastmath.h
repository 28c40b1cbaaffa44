// The |x| <= 708 exp and the positive-normal log of detmath (detmath/detmath.h: exp_poly + one ldexp; log_dd's hi
// part without its subnormal branch) with their polynomial constants read from a constant table into SGPRs and
// used as SGPR operands of v_fma_f64 (gs_fma_s): no v_mov_b32 pair per 64-bit constant per evaluation. The same
// bits as detmath::exp / detmath::log on those domains (tests: every kernel's parity suite; tools/mb/mb_brent).
// Included by device/special.h; the inline users are device/gamma_lean.h and the kernels' kmath<true>.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../detmath/detmath.h"

namespace shyft_dev {

// exp: INV_LN2 SHIFT LN2_HI LN2_LO and detmath::exp_poly's q coefficients; log: LN2_HI LN2_LO and
// detmath::log_core's Lg1 .. Lg7
static __constant__ double gsb_const[32] = {
    1.4426950408889634, 6755399441055744.0, 6.93147180369123816490e-01, 1.90821492927058770002e-10,
    detmath::EXP_Q[0], detmath::EXP_Q[1], detmath::EXP_Q[2], detmath::EXP_Q[3], detmath::EXP_Q[4], detmath::EXP_Q[5],
    detmath::EXP_Q[6], detmath::EXP_Q[7], detmath::EXP_Q[8], detmath::EXP_Q[9], detmath::EXP_Q[10],
    detmath::LOG_LG1, detmath::LOG_LG2, detmath::LOG_LG3, detmath::LOG_LG4, detmath::LOG_LG5, detmath::LOG_LG6,
    detmath::LOG_LG7, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

typedef __attribute__((address_space(4))) const double gsb_cdouble;

// a * b + c with c an SGPR pair (wave-uniform constant): one v_fma_f64, no v_mov of the constant
__device__ __forceinline__ double gs_fma_s(double a, double b, double c) {
    double d;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
    return d;
}

struct gsb_k {
    double c[22];
};

__device__ __forceinline__ gsb_k gsb_load() {
    gsb_k k;
    const gsb_cdouble* __restrict__ p = (const gsb_cdouble*)gsb_const;
    asm volatile("" : "+s"(p));  // keep the table opaque: scalar loads into SGPRs, not folded literals
#pragma unroll
    for (int i = 0; i < 22; ++i) k.c[i] = p[i];
    return k;
}

// detmath::exp for |x| <= 708 (exp_poly + one ldexp)
__device__ __forceinline__ double gsb_exp(double x, const gsb_k& k) {
    const double t = gs_fma_s(x, k.c[0], k.c[1]);
    const double kf = t - k.c[1];
    double r = __builtin_fma(-kf, k.c[2], x);
    r = __builtin_fma(-kf, k.c[3], r);
    double q = gs_fma_s(r, k.c[4], k.c[5]);
#pragma unroll
    for (int i = 6; i <= 14; ++i) q = gs_fma_s(q, r, k.c[i]);
    return __builtin_ldexp(__builtin_fma(r, q, 1.0), (int)kf);
}

// two values of one elementary function (dexp2 of device/special.h, kmath's exp2 / log2p of device/pt_dev.h)
struct dexp_pair {
    double a, b;
};

// gsb_exp of two independent arguments, step by step side by side: one basic block, so each chain's fma latency
// is hidden behind the other's -- the same instructions and the same bits as gsb_exp(x), gsb_exp(y)
__device__ __forceinline__ dexp_pair gsb_exp2(double x, double y, const gsb_k& k) {
    const double tx = gs_fma_s(x, k.c[0], k.c[1]), ty = gs_fma_s(y, k.c[0], k.c[1]);
    const double kx = tx - k.c[1], ky = ty - k.c[1];
    double rx = __builtin_fma(-kx, k.c[2], x), ry = __builtin_fma(-ky, k.c[2], y);
    rx = __builtin_fma(-kx, k.c[3], rx);
    ry = __builtin_fma(-ky, k.c[3], ry);
    double qx = gs_fma_s(rx, k.c[4], k.c[5]), qy = gs_fma_s(ry, k.c[4], k.c[5]);
#pragma unroll
    for (int i = 6; i <= 14; ++i) {
        qx = gs_fma_s(qx, rx, k.c[i]);
        qy = gs_fma_s(qy, ry, k.c[i]);
    }
    dexp_pair r;
    r.a = __builtin_ldexp(__builtin_fma(rx, qx, 1.0), (int)kx);
    r.b = __builtin_ldexp(__builtin_fma(ry, qy, 1.0), (int)ky);
    return r;
}

// detmath::log for positive normal finite x (detmath::log_core with k_adj = 0, step by step)
__device__ __forceinline__ double gsb_log(double x, const gsb_k& k) {
    uint64_t u = (uint64_t)__double_as_longlong(x);
    int e = (int)((u >> 52) & 0x7ff) - 1023;
    const uint32_t hx = (uint32_t)(u >> 32) & 0x000fffffu;
    const uint32_t i = (hx + 0x95f64u) & 0x100000u;
    u = (u & 0x000fffffffffffffull) | ((uint64_t)(i ^ 0x3ff00000u) << 32);
    e += (int)(i >> 20);
    const double f = __longlong_as_double((long long)u) - 1.0;
    const double s = f / (2.0 + f);
    const double dk = (double)e;
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * gs_fma_s(w, gs_fma_s(w, k.c[20], k.c[18]), k.c[16]);
    const double t2 = z * gs_fma_s(w, gs_fma_s(w, gs_fma_s(w, k.c[21], k.c[19]), k.c[17]), k.c[15]);
    const double R = t2 + t1;
    if (((int32_t)(hx - 0x6147au) | (int32_t)(0x6b851u - hx)) > 0) {
        const double hfsq = 0.5 * f * f;
        return dk * k.c[2] - ((hfsq - __builtin_fma(s, hfsq + R, dk * k.c[3])) - f);
    }
    return dk * k.c[2] - (__builtin_fma(s, f - R, -(dk * k.c[3])) - f);
}

// gsb_log of two independent arguments, step by step side by side as gsb_exp2 -- the same instructions and the
// same bits as gsb_log(x), gsb_log(y)
__device__ __forceinline__ dexp_pair gsb_log2(double x, double y, const gsb_k& k) {
    uint64_t ux = (uint64_t)__double_as_longlong(x), uy = (uint64_t)__double_as_longlong(y);
    int ex = (int)((ux >> 52) & 0x7ff) - 1023, ey = (int)((uy >> 52) & 0x7ff) - 1023;
    const uint32_t hx = (uint32_t)(ux >> 32) & 0x000fffffu, hy = (uint32_t)(uy >> 32) & 0x000fffffu;
    const uint32_t ix = (hx + 0x95f64u) & 0x100000u, iy = (hy + 0x95f64u) & 0x100000u;
    ux = (ux & 0x000fffffffffffffull) | ((uint64_t)(ix ^ 0x3ff00000u) << 32);
    uy = (uy & 0x000fffffffffffffull) | ((uint64_t)(iy ^ 0x3ff00000u) << 32);
    ex += (int)(ix >> 20);
    ey += (int)(iy >> 20);
    const double fx = __longlong_as_double((long long)ux) - 1.0, fy = __longlong_as_double((long long)uy) - 1.0;
    const double sx = fx / (2.0 + fx), sy = fy / (2.0 + fy);
    const double dkx = (double)ex, dky = (double)ey;
    const double zx = sx * sx, zy = sy * sy;
    const double wx = zx * zx, wy = zy * zy;
    double ax = gs_fma_s(wx, k.c[20], k.c[18]), ay = gs_fma_s(wy, k.c[20], k.c[18]);
    double bx = gs_fma_s(wx, k.c[21], k.c[19]), by = gs_fma_s(wy, k.c[21], k.c[19]);
    ax = gs_fma_s(wx, ax, k.c[16]);
    ay = gs_fma_s(wy, ay, k.c[16]);
    bx = gs_fma_s(wx, bx, k.c[17]);
    by = gs_fma_s(wy, by, k.c[17]);
    bx = gs_fma_s(wx, bx, k.c[15]);
    by = gs_fma_s(wy, by, k.c[15]);
    const double Rx = zx * bx + wx * ax, Ry = zy * by + wy * ay;
    dexp_pair r;
    if (((int32_t)(hx - 0x6147au) | (int32_t)(0x6b851u - hx)) > 0) {
        const double hfsq = 0.5 * fx * fx;
        r.a = dkx * k.c[2] - ((hfsq - __builtin_fma(sx, hfsq + Rx, dkx * k.c[3])) - fx);
    } else {
        r.a = dkx * k.c[2] - (__builtin_fma(sx, fx - Rx, -(dkx * k.c[3])) - fx);
    }
    if (((int32_t)(hy - 0x6147au) | (int32_t)(0x6b851u - hy)) > 0) {
        const double hfsq = 0.5 * fy * fy;
        r.b = dky * k.c[2] - ((hfsq - __builtin_fma(sy, hfsq + Ry, dky * k.c[3])) - fy);
    } else {
        r.b = dky * k.c[2] - (__builtin_fma(sy, fy - Ry, -(dky * k.c[3])) - fy);
    }
    return r;
}

}  // namespace shyft_dev
