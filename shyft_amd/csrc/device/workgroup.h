// The wavefront and workgroup building blocks that the reduction, selection and series kernels share (gfx950,
// 64-lane wavefronts); device-only, and there is one copy of each. The fp64 key functions live here, not in
// device/pct_plan.h, which keeps the host+device plan. Each block carries a bit-exactness promise, argued here once:
//   - a reduction adds in one fixed order, so an fp64 sum has the same bits on every run;
//   - order statistics go through integer keys, so a selection equals a full sort;
//   - every barrier sits where all lanes of the workgroup meet it;
//   - a wavefront-local LDS sort is fenced, so no LDS access moves across a stage.
// Every function says who must call it and what it reads. None of them reads global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- quiet NaN, finite, order-preserving key ------------------------------------------------------------------------
constexpr uint64_t RS_SIGN = 0x8000000000000000ull;
constexpr uint64_t RS_EXPO = 0x7ff0000000000000ull;

__device__ inline double rs_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
// isfinite by the exponent bits
__device__ inline bool rs_finite(double x) { return ((uint64_t)__double_as_longlong(x) & RS_EXPO) != RS_EXPO; }

// The order-preserving 64-bit key of an fp64 value: a < b as doubles implies key(a) < key(b) as integers; +0.0 and
// -0.0 are different keys. Returns false for NaN and +-inf. Every finite key is below the all-ones sentinel.
__device__ inline bool key_of(double v, uint64_t& key) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    key = (u & RS_SIGN) ? ~u : (u | RS_SIGN);
    return (u & RS_EXPO) != RS_EXPO;  // rs_finite(v)
}
__device__ inline double value_of(uint64_t key) {
    const uint64_t u = (key & RS_SIGN) ? (key ^ RS_SIGN) : ~key;
    return __longlong_as_double((long long)u);
}

// ---- binary search ---------------------------------------------------------------------------------------------------
// The first index in [lo, hi) for which pred(index) is false, hi when there is none; pred must be true on a prefix of
// the range and false on the rest. Any lane may call it. pred is asked about indexes m with lo <= m < hi only.
template <class I, class Pred>
__device__ inline I first_false(I lo, I hi, Pred pred) {
    while (lo < hi) {
        const I m = lo + ((hi - lo) >> 1);
        if (pred(m)) lo = m + 1;
        else hi = m;
    }
    return lo;
}

// ---- wavefront reduction ---------------------------------------------------------------------------------------------
struct op_add {
    template <class T>
    __device__ T operator()(T a, T b) const { return a + b; }
};
struct op_min {
    template <class T>
    __device__ T operator()(T a, T b) const { return a < b ? a : b; }
};
struct op_max {
    template <class T>
    __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// Fixed xor butterfly over the 64 lanes: offsets 32, 16, .., 1, v = op(v, partner's v). All 64 lanes of the wavefront
// call it, in wavefront-uniform control flow; every lane returns the same bits (op is commutative), the same on every
// run. Reads registers only.
template <class T, class Op>
__device__ inline T wave_reduce(T v, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- workgroup sum ---------------------------------------------------------------------------------------------------
// Sum over a workgroup of WG lanes: the butterfly per wavefront, lane 0 of each wavefront stores, one barrier, thread 0
// adds part[0] + part[1] + .. in wavefront order. All WG lanes call it, in workgroup-uniform control flow. Thread 0
// returns the sum, every other lane T(). Each (WG, T) has its own LDS slots; a second call with the same WG and T needs
// a barrier in between (thread 0 may still be reading them).
template <int WG, class T>
__device__ inline T block_sum(T v) {
    __shared__ T part[WG / 64];
    v = wave_reduce(v, op_add());
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) part[wid] = v;
    __syncthreads();
    T r = T();
    if (threadIdx.x == 0) {
        r = part[0];
        for (int w = 1; w < WG / 64; ++w) r += part[w];
    }
    return r;
}

// ---- workgroup scan --------------------------------------------------------------------------------------------------
constexpr int SCAN_BLOCK = 256;  // the workgroup of block_scan: 4 wavefronts

// Inclusive scan of one value per lane over the SCAN_BLOCK lanes of the workgroup in thread order: a __shfl_up scan in
// each wavefront, lane 63 stores its wavefront's total to part[wavefront], and every lane combines the totals of the
// wavefronts before its own. `total` is the result over all lanes. All SCAN_BLOCK lanes call it, in workgroup-uniform
// control flow (two barriers; the first keeps the previous call's readers of part ahead of this call's writers).
// part is SCAN_BLOCK / 64 slots of LDS that the caller owns; on return part[w] is wavefront w's total and stays so
// until the next call, so "the result over the lanes before this one" is __shfl_up(result, 1), and for lane 0 of a
// wavefront the fold of part[0 .. wavefront): no second scan. op must be associative; identity is its neutral value.
template <class T, class Op>
__device__ inline T block_scan(T v, Op op, T identity, T* part, T& total) {
    const int lane = int(threadIdx.x & 63), wave = int(threadIdx.x >> 6);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= d) v = op(v, o);
    }
    __syncthreads();
    if (lane == 63) part[wave] = v;
    __syncthreads();
    T before = identity;
    total = identity;
#pragma unroll
    for (int w = 0; w < SCAN_BLOCK / 64; ++w) {
        const T y = part[w];
        if (w < wave) before = op(before, y);
        total = op(total, y);
    }
    return op(v, before);
}

// ---- bitonic sorts of 64-bit keys ------------------------------------------------------------------------------------
// What separates two stages of an LDS sort. WAVE: the lanes are one wavefront, whose LDS operations complete in order;
// the fences keep the compiler from moving or caching LDS accesses across the point, and no workgroup barrier is met,
// so other wavefronts of the workgroup may be elsewhere. Otherwise a workgroup barrier, which every lane of the
// workgroup must meet.
template <bool WAVE>
__device__ inline void lds_sync() {
    if (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        __syncthreads();
    }
}

// Pads keys[nf .. Q) (and idx, with PAYLOAD) with the all-ones sentinel, which sorts after every finite key; returns Q,
// the power of two >= nf. The nt lanes tid = 0 .. nt - 1 call it; the caller synchronises before the sort. Writes
// slots < Q only, so the arrays need as many slots as the power of two >= the largest nf.
template <bool PAYLOAD>
__device__ inline int lds_sort_pad(uint64_t* keys, uint32_t* idx, int nf, int tid, int nt) {
    int Q = 1;
    while (Q < nf) Q <<= 1;
    for (int i = nf + tid; i < Q; i += nt) {
        keys[i] = ~0ull;
        if (PAYLOAD) idx[i] = ~0u;
    }
    return Q;
}

// Bitonic sort of the Q (a power of two) keys in LDS, ascending. With PAYLOAD, (key, idx) pairs sorted
// lexicographically: the payload breaks every tie, so the order is total and the network's instability cannot show;
// without it idx is not read and may be null. The nt lanes
// tid = 0 .. nt - 1 call it with the same Q, in control flow uniform over them: WAVE with nt == 64 lanes of one
// wavefront, otherwise all lanes of the workgroup. The arrays must be visible to the lanes on entry (lds_sync after
// the last write) and are on return. Touches slots i and i ^ j, both < Q.
template <bool WAVE, bool PAYLOAD>
__device__ inline void lds_bitonic_sort(uint64_t* keys, uint32_t* idx, int Q, int tid, int nt) {
    for (int k = 2; k <= Q; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < Q; i += nt) {
                const int x = i ^ j;
                if (x > i) {
                    const uint64_t a = keys[i], d = keys[x];
                    const uint32_t ia = PAYLOAD ? idx[i] : 0u, id = PAYLOAD ? idx[x] : 0u;
                    const bool up = (i & k) == 0;
                    const bool gt = a > d || (a == d && ia > id);
                    if (gt == up) {
                        keys[i] = d;
                        keys[x] = a;
                        if (PAYLOAD) {
                            idx[i] = id;
                            idx[x] = ia;
                        }
                    }
                }
            }
            lds_sync<WAVE>();
        }
    }
}

// The cross-lane form: bitonic sort of one key per lane, ascending by lane; no LDS and no barrier. All 64 lanes of the
// wavefront call it, in wavefront-uniform control flow.
__device__ inline uint64_t wave_bitonic_sort(uint64_t key, int lane) {
    for (int k = 2; k <= 64; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const uint64_t o = __shfl_xor(key, j, 64);
            const bool up = (lane & k) == 0, low = (lane & j) == 0;
            const uint64_t mn = key < o ? key : o, mx = key < o ? o : key;
            key = low == up ? mn : mx;
        }
    return key;
}
