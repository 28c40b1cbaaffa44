// The series of a flat point of a CSR batch, shared by kernels/tsprep.hip, kernels/tsfilter.hip and kernels/ts_expr.hip
// (the expression of a wavefront); there is one copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "workgroup.h"

// the series of flat point k < row[S]: the s with row[s] <= k < row[s+1] (empty series are stepped over). Reads
// row[1 .. S] only. I is the type of a series index, int32 or int64.
template <class I>
__device__ inline I csr_series_of(const int64_t* __restrict__ row, I S, int64_t k) {
    return first_false(I(0), S, [&](I m) { return row[m + 1] <= k; });  // upper_bound of k in row[1 .. S]
}
