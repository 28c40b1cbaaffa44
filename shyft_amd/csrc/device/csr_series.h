// The series of a flat point of a CSR batch, shared by kernels/tsprep.hip and kernels/tsfilter.hip; there is one copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the series of flat point k < row[S]: the s with row[s] <= k < row[s+1] (empty series are stepped over). Reads
// row[1 .. S] only.
__device__ inline int64_t csr_series_of(const int64_t* __restrict__ row, int64_t S, int64_t k) {
    int64_t lo = 0, hi = S;  // upper_bound of k in row[1 .. S]
    while (lo < hi) {
        const int64_t m = lo + ((hi - lo) >> 1);
        if (row[m + 1] <= k) lo = m + 1;
        else hi = m;
    }
    return lo;
}
