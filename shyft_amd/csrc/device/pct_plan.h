// What a percentile entry reads of a sorted sample set. Shared by kernels/percentiles.hip (the cells of a region),
// kernels/ts_percentiles.hip (a vector of series) and, for the plan alone, host/ts_percentiles.hpp; there is one copy.
// The order-preserving key of an fp64 sample is device-only and lives in device/workgroup.h.
//
// The plan is plain C++ and compiles for the host and the device; pct_value is device code and exists only under
// hipcc. Its multiply and add are rounded separately (-ffp-contract=off on every file that includes this).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PCT_HD __host__ __device__
#else
#define PCT_HD
#endif

enum { PCT_NAN = 0, PCT_SINGLE = 1, PCT_LERP = 2, PCT_AVG = 3 };
struct pct_plan {
    int kind;
    uint32_t lo, hi;
    double delta;
};

// What percentile p of ns sorted samples reads (time_series_statistics.h:119-157; R7 with the eps rules), and the
// extremes on the model's own axis (nan_min / nan_max of one value per series, :25-39, :77-90, :221-226).
PCT_HD inline pct_plan pct_make_plan(int64_t p, int ns) {
    pct_plan r{PCT_NAN, 0u, 0u, 0.0};
    if (ns <= 0) return r;
    if (p == -1) {
        r.kind = PCT_AVG;
    } else if (p == -1000) {
        r.kind = PCT_SINGLE;
    } else if (p == 1000) {
        r.kind = PCT_SINGLE;
        r.lo = uint32_t(ns - 1);
    } else if (p >= 0 && p <= 100) {
        const double eps = 1e-30;
        double nd = 1.0 + (ns - 1) * double(p) / 100.0;
        int n = int(nd);
        double delta = nd - n;
        --n;
        r.kind = PCT_SINGLE;
        if (n <= 0 && delta <= eps) {
            r.lo = 0u;
        } else if (n >= ns) {
            r.lo = uint32_t(ns - 1);
        } else if (delta < eps) {
            r.lo = uint32_t(n);
        } else {
            r.kind = PCT_LERP;
            r.lo = uint32_t(n);
            r.hi = uint32_t(n < ns - 1 ? n + 1 : n);
            r.delta = delta;
        }
    }
    return r;
}

#ifdef __HIPCC__
__device__ inline double pct_value(const pct_plan& pl, double lower, double upper) {
    if (pl.kind == PCT_SINGLE) return lower;
    return lower + pl.delta * (upper - lower);  // separately rounded multiply and add (-ffp-contract=off)
}
#endif
