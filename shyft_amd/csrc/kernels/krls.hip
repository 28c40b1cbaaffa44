// Batched KRLS training and prediction for gfx950: prediction::krls_rbf_predictor (core/predictions.h:30-343) over
// dlib::krls, restated in host/krls.hpp, which is the definition of correct. The device is bit-identical to it in the
// dictionary, the weights, Kinv, P, the mse and every predicted value. Parity with dlib's last bit is not pinned.
//
// krls_train_k  One workgroup of KRLS_BLOCK lanes per series of a CSR batch; the point loop and the iteration loop run
//   inside the kernel, every series with its own dt, gamma, tolerance, offset, count, stride, iterations, mse_tol and
//   an optional starting state. The recursion is sequential in the points; the O(m^2) work of one point is spread over
//   the lanes.
//   Lane mapping. Lane l owns the rows l, l + KRLS_BLOCK, ... of Kinv and P: it forms the elements of Kinv k, P a and
//   Kinv q for those rows, one accumulator each, adding the terms in index order as the host does, and it updates
//   those rows. For a' P the same lane owns the COLUMNS l, l + KRLS_BLOCK, ... and walks down them. The four scalar
//   products (k.a, k.alpha, a.Pa, and the f(x) of the running mse) are krls_dot of host/krls.hpp: every wavefront
//   forms the same 64 strided partial sums and folds them with six xor exchanges (wave_reduce, device/workgroup.h), so all lanes of the workgroup hold
//   the same bits and the grow/update decision delta > tolerance is uniform without a broadcast.
//   Layout. k, a, Pa, r, q, alpha and d live in LDS, `cap` doubles each. The matrices are row-major with the leading
//   dimension ld = cap | 1, an odd count of doubles. ds_read_b64 serves 32 lanes per cycle from 64 four-byte banks,
//   bank (address / 4) mod 64: in a per-row product 32 neighbouring lanes read one column of 32 neighbouring rows,
//   2 * ld dwords apart, which for odd ld are 32 different even banks; in the per-column product they read 32
//   neighbouring doubles of one row. So neither direction has a systematic conflict, and an even ld (96, say) would
//   put the 32 rows on two banks.
//   Storage. The kernel is written once over two matrix pointers and ld and instantiated twice. IN_LDS: both matrices
//   in dynamic LDS, for a capacity of KRLS_LDS_CAP = 99 entries, the largest c with (7 c + 2 c (c | 1)) * 8 bytes
//   within the CU's 160 KiB, and before it for KRLS_LDS_SMALL_CAP = 31 entries (17 KB): a workgroup with the whole
//   LDS has its CU to itself, which a batch of more series than CUs with short dictionaries pays for (measured: 1,000
//   series with 23 entries took 13.6 ms at capacity 99 and 7.3 ms in the workspace), so such series are served eight
//   workgroups to a CU. Workspace: the matrices in a slab of device memory per series, for capacities up to
//   KRLS_MAX_DICT = 1024; the vectors stay in LDS. There the per-row products read with a stride of ld doubles
//   between lanes (uncoalesced, served by the caches) and the per-column product and the row updates are coalesced
//   over j only across lanes of different rows; DESIGN.md 3.15 has the measured cost.
//   The kernel never removes a dictionary entry. It ends a series with status 1 when the dictionary wants to grow past
//   the storage capacity and with status 2 when it wants to grow at max_dict_size; the entry retrains such a series
//   from its original state on the next path (LDS -> workspace -> host), and returns the path per series.
//   Control flow. Every __syncthreads and every cross-lane exchange sits in workgroup-uniform control flow: the loop
//   bounds, the NaN test of a point's value, m, delta and the status come from values that all lanes computed from
//   the same memory with the same instructions. Lanes beyond m skip the arithmetic and stay in the loop.
//
// krls_predict_k  One lane per (predictor, output time): a workgroup takes a tile of KRLS_BLOCK output times of one
//   predictor and stages the dictionary and the weights through LDS in tiles of KRLS_BLOCK; each lane adds
//   alpha_i * k(x, d_i) to its one accumulator in index order. With values given the output is the residual
//   v - f(x) (NaN where v is NaN), which predictor_mse and mse_ts sum on the host in the reference's order.
//
// Index safety. The host checks row and s_row (non-decreasing from 0) before any launch, so a job's points r0 + i,
// i < dim <= n, lie inside the uploaded t and v, and its starting state inside the uploaded s_* arrays. m starts at
// m0 <= cap (the entry sends a larger state to the next path) and grows only after the test m < cap, so the row and
// the column m that a growth step writes exist: rows < cap, columns < cap <= ld. Vector indexes are < m <= cap or
// == m < cap. A slab holds 2 cap + 2 cap ld doubles per job and job b uses [b * slab_stride, (b + 1) * slab_stride).
// krls_pack_k copies m <= cap entries of a finished job to offsets the host computed from the downloaded m.
// krls_predict_k reads d and alpha at d_row[s] + j, j < m_s, q_t and q_v at q_row[s] + i, i < n_s, and LDS slots
// < KRLS_BLOCK.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/shyft_hip.h"
#include "../device/workgroup.h"
#include "../host/krls.hpp"
#include "../include_internal/device_call.h"
#include "../include_internal/series_args.h"

using namespace shyft_hip_impl;
namespace h = shyft_hip::host;

namespace {

constexpr int KRLS_BLOCK = 256;  // 4 wavefronts
constexpr int KRLS_VECTORS = 7;  // k, a, Pa, r, q, alpha, d
constexpr int KRLS_MAX_DICT = SHYFT_HIP_KRLS_MAX_DICT;
constexpr size_t KRLS_LDS_BYTES = 160 * 1024;  // per CU on gfx950, and the most one workgroup can have

constexpr int krls_ld(int cap) { return cap | 1; }
constexpr size_t krls_lds_bytes(int cap, bool in_lds) {
    return (size_t(KRLS_VECTORS) * cap + (in_lds ? 2 * size_t(cap) * krls_ld(cap) : 0)) * sizeof(double);
}
constexpr int krls_lds_cap() {
    int c = 1;
    while (krls_lds_bytes(c + 1, true) <= KRLS_LDS_BYTES) ++c;
    return c;
}
constexpr int KRLS_LDS_CAP = krls_lds_cap();
static_assert(KRLS_LDS_CAP == SHYFT_HIP_KRLS_LDS_CAPACITY, "include/shyft_hip.h states the LDS capacity");
// the small LDS storage: eight workgroups of it (32 wavefronts, all a CU runs) fit the CU's LDS
constexpr int KRLS_LDS_SMALL_CAP = SHYFT_HIP_KRLS_LDS_SMALL_CAPACITY;
static_assert(8 * krls_lds_bytes(KRLS_LDS_SMALL_CAP, true) <= KRLS_LDS_BYTES && KRLS_LDS_SMALL_CAP < KRLS_LDS_CAP, "");
static_assert(krls_lds_bytes(KRLS_MAX_DICT, false) <= 64 * 1024, "the vectors of the workspace path fit a small LDS share");

struct krls_job {  // one series of a launch
    int64_t r0;    // its first point in t and v
    int64_t offset, dim, stride, iterations, max_dict;
    double scaling_f, gamma, tolerance, mse_tol;
    int64_t m0, s_vec, s_mat;  // the starting state: entries, offset into s_d / s_alpha, offset into s_Kinv / s_P
};

struct krls_train_args {
    const krls_job* jobs;
    const int64_t* t;
    const double* v;
    const double* s_d;
    const double* s_alpha;
    const double* s_Kinv;
    const double* s_P;
    double* slab;  // per job: d [cap], alpha [cap], Kinv [cap][ld], P [cap][ld]
    int64_t slab_stride;
    int cap, ld;
    int64_t* m_out;
    int32_t* status;
    double* mse;
};

// krls_dot of host/krls.hpp on one wavefront; every lane returns the sum
__device__ inline double krls_wave_dot(const double* u, const double* v, int m, int lane) {
    double acc = 0.0;
    for (int i = lane; i < m; i += 64) acc = acc + u[i] * v[i];
    return wave_reduce(acc, op_add());
}

template <bool IN_LDS>
__global__ __launch_bounds__(KRLS_BLOCK) void krls_train_k(const krls_train_args A) {
    extern __shared__ __attribute__((aligned(16))) double krls_sm[];
    const int tid = int(threadIdx.x), lane = tid & 63;
    const krls_job J = A.jobs[blockIdx.x];
    const int cap = A.cap, ld = A.ld;
    double* const k = krls_sm;
    double* const a = k + cap;
    double* const Pa = a + cap;
    double* const r = Pa + cap;
    double* const q = r + cap;
    double* const alpha = q + cap;
    double* const d = alpha + cap;
    double* const slab = A.slab + int64_t(blockIdx.x) * A.slab_stride;
    double* Kinv;
    if constexpr (IN_LDS) Kinv = d + cap;
    else Kinv = slab + 2 * int64_t(cap);
    double* const P = Kinv + int64_t(cap) * ld;

    int m = int(J.m0);
    for (int idx = tid; idx < m * m; idx += KRLS_BLOCK) {
        const int i = idx / m, j = idx - i * m;
        Kinv[i * ld + j] = A.s_Kinv[J.s_mat + idx];
        P[i * ld + j] = A.s_P[J.s_mat + idx];
    }
    for (int i = tid; i < m; i += KRLS_BLOCK) {
        d[i] = A.s_d[J.s_vec + i];
        alpha[i] = A.s_alpha[J.s_vec + i];
    }
    __syncthreads();

    const double gamma = J.gamma, tolerance = J.tolerance;
    double mse = 0.0;
    int status = 0;
    for (int64_t iter = 0; iter < J.iterations && status == 0; ++iter) {
        mse = 0.0;
        int64_t nan_count = 0;
        for (int64_t p = J.offset; p < J.dim; p += J.stride) {
            const double y = A.v[J.r0 + p];
            if (y != y) {
                nan_count += 1;
                continue;
            }
            const double x = h::krls_position(A.t[J.r0 + p], J.scaling_f);
            if (m == 0) {  // the first sample
                if (tid == 0) {
                    d[0] = x;
                    alpha[0] = y / 1.0;
                    Kinv[0] = 1.0 / 1.0;
                    P[0] = 1.0;
                    k[0] = h::krls_kernel(gamma, x, x);
                }
                m = 1;
            } else {
                for (int i = tid; i < m; i += KRLS_BLOCK) k[i] = h::krls_kernel(gamma, x, d[i]);
                __syncthreads();
                for (int i = tid; i < m; i += KRLS_BLOCK) {
                    const double* row = Kinv + i * ld;
                    double acc = 0.0;
                    for (int j = 0; j < m; ++j) acc = acc + row[j] * k[j];
                    a[i] = acc;
                }
                __syncthreads();
                const double delta = 1.0 - krls_wave_dot(k, a, m, lane);
                const double e = y - krls_wave_dot(k, alpha, m, lane);
                __syncthreads();  // every wavefront has read alpha before a row owner changes it
                if (delta > tolerance) {
                    if (int64_t(m) >= J.max_dict) status = 2;
                    else if (m >= cap) status = 1;
                    if (status != 0) break;
                    const double ka = e / delta;
                    for (int i = tid; i < m; i += KRLS_BLOCK) {
                        double* row = Kinv + i * ld;
                        const double ai = a[i];
                        for (int j = 0; j < m; ++j) row[j] = row[j] + (ai * a[j]) / delta;
                        row[m] = -ai / delta;
                        P[i * ld + m] = 0.0;
                        alpha[i] = alpha[i] - ai * ka;
                    }
                    for (int j = tid; j < m; j += KRLS_BLOCK) {  // the new row, its columns spread over the lanes
                        Kinv[m * ld + j] = -a[j] / delta;
                        P[m * ld + j] = 0.0;
                    }
                    if (tid == 0) {
                        Kinv[m * ld + m] = 1.0 / delta;
                        P[m * ld + m] = 1.0;
                        alpha[m] = ka;
                        d[m] = x;
                        k[m] = h::krls_kernel(gamma, x, x);
                    }
                    m += 1;
                } else {
                    for (int i = tid; i < m; i += KRLS_BLOCK) {
                        const double* row = P + i * ld;
                        double acc = 0.0;
                        for (int j = 0; j < m; ++j) acc = acc + row[j] * a[j];
                        Pa[i] = acc;
                    }
                    __syncthreads();
                    const double s = 1.0 + krls_wave_dot(a, Pa, m, lane);
                    for (int i = tid; i < m; i += KRLS_BLOCK) q[i] = Pa[i] / s;
                    for (int j = tid; j < m; j += KRLS_BLOCK) {  // a' P: this lane walks down column j
                        double acc = 0.0;
                        for (int i = 0; i < m; ++i) acc = acc + a[i] * P[i * ld + j];
                        r[j] = acc;
                    }
                    __syncthreads();
                    for (int i = tid; i < m; i += KRLS_BLOCK) {
                        double* prow = P + i * ld;
                        const double* krow = Kinv + i * ld;
                        const double qi = q[i];
                        double acc = 0.0;
                        for (int j = 0; j < m; ++j) {
                            prow[j] = prow[j] - qi * r[j];
                            acc = acc + krow[j] * q[j];
                        }
                        alpha[i] = alpha[i] + acc * e;
                    }
                }
            }
            __syncthreads();
            const double diff_v = y - krls_wave_dot(alpha, k, m, lane);
            mse = mse + diff_v * diff_v;
            __syncthreads();  // k and alpha have been read before the next point rewrites them
        }
        if (status != 0) break;
        const double cnt = double(J.dim - nan_count);
        mse = mse / (cnt > 1.0 ? cnt : 1.0);
        if (mse < J.mse_tol) break;
    }

    __syncthreads();
    if (tid == 0) {
        A.m_out[blockIdx.x] = m;
        A.status[blockIdx.x] = status;
        A.mse[blockIdx.x] = mse;
    }
    for (int i = tid; i < m; i += KRLS_BLOCK) {
        slab[i] = d[i];
        slab[cap + i] = alpha[i];
    }
    if constexpr (IN_LDS) {
        double* const gK = slab + 2 * int64_t(cap);
        double* const gP = gK + int64_t(cap) * ld;
        for (int idx = tid; idx < m * m; idx += KRLS_BLOCK) {
            const int i = idx / m, j = idx - i * m;
            gK[i * ld + j] = Kinv[i * ld + j];
            gP[i * ld + j] = P[i * ld + j];
        }
    }
}

struct krls_pack_args {
    const double* slab;
    int64_t slab_stride;
    int cap, ld;
    const int64_t* m;       // [jobs] the entries to copy, 0 for a job that did not finish
    const int64_t* v_off;   // [jobs] into d / alpha
    const int64_t* m_off;   // [jobs] into Kinv / P, dense m x m
    double* d;
    double* alpha;
    double* Kinv;
    double* P;
};

__global__ __launch_bounds__(KRLS_BLOCK) void krls_pack_k(const krls_pack_args A) {
    const int tid = int(threadIdx.x);
    const int m = int(A.m[blockIdx.x]);
    const double* const slab = A.slab + int64_t(blockIdx.x) * A.slab_stride;
    const double* const gK = slab + 2 * int64_t(A.cap);
    const double* const gP = gK + int64_t(A.cap) * A.ld;
    const int64_t vo = A.v_off[blockIdx.x], mo = A.m_off[blockIdx.x];
    for (int i = tid; i < m; i += KRLS_BLOCK) {
        A.d[vo + i] = slab[i];
        A.alpha[vo + i] = slab[A.cap + i];
    }
    for (int idx = tid; idx < m * m; idx += KRLS_BLOCK) {
        const int i = idx / m, j = idx - i * m;
        A.Kinv[mo + idx] = gK[i * A.ld + j];
        A.P[mo + idx] = gP[i * A.ld + j];
    }
}

struct krls_predict_args {
    int64_t ntiles;
    const int64_t* tile_s;   // [ntiles] the predictor of a tile
    const int64_t* tile_i0;  // [ntiles] its first output time inside the predictor's queries
    const int64_t* d_row;
    const double* d;
    const double* alpha;
    const double* scaling_f;
    const double* gamma;
    const int64_t* q_row;
    const int64_t* q_t;
    const double* q_v;  // null: predictions; given: residuals
    double* out;
};

__global__ __launch_bounds__(KRLS_BLOCK) void krls_predict_k(const krls_predict_args A) {
    __shared__ double ds[KRLS_BLOCK];
    __shared__ double as[KRLS_BLOCK];
    const int l = int(threadIdx.x);
    for (int64_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {  // uniform over the workgroup
        const int64_t s = A.tile_s[tile];
        const int64_t q0 = A.q_row[s], n = A.q_row[s + 1] - q0;
        const int64_t d0 = A.d_row[s], m = A.d_row[s + 1] - d0;
        const int64_t i = A.tile_i0[tile] + l;
        const bool valid = i < n;
        const double gamma = A.gamma[s];
        const double x = valid ? h::krls_position(A.q_t[q0 + i], A.scaling_f[s]) : 0.0;
        double acc = 0.0;
        for (int64_t j0 = 0; j0 < m; j0 += KRLS_BLOCK) {  // uniform
            const int cnt = int(m - j0 < KRLS_BLOCK ? m - j0 : KRLS_BLOCK);
            __syncthreads();  // the previous tile of the dictionary has been read
            if (l < cnt) {
                ds[l] = A.d[d0 + j0 + l];
                as[l] = A.alpha[d0 + j0 + l];
            }
            __syncthreads();
            if (valid)
                for (int jj = 0; jj < cnt; ++jj) acc = acc + as[jj] * h::krls_kernel(gamma, x, ds[jj]);
        }
        if (valid) {
            double o = acc;
            if (A.q_v) {
                const double v = A.q_v[q0 + i];
                o = v != v ? v : v - acc;
            }
            A.out[q0 + i] = o;
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct krls_in {  // the arguments of a train entry, checked
    size_t S;
    const int64_t* row;
    const int64_t* t;
    const double* v;
    const int64_t* dt;
    const double* gamma;
    const double* tolerance;
    const int64_t* max_dict;
    const int64_t* offset;
    const int64_t* count;
    const int64_t* stride;
    const int64_t* iterations;
    const double* mse_tol;
    const int64_t* s_row;  // null: every predictor starts empty
    const double* s_d;
    const double* s_alpha;
    const double* s_Kinv;
    const double* s_P;
    std::vector<int64_t> s_mat;  // [S+1] offsets of the dense starting matrices
    int64_t m0(size_t s) const { return s_row ? s_row[s + 1] - s_row[s] : 0; }
    size_t n(size_t s) const { return size_t(row[s + 1] - row[s]); }
    size_t dim(size_t s) const { return h::krls_dim(size_t(offset[s]), count[s], size_t(stride[s]), n(s)); }
};

}  // namespace

struct shyft_hip_krls_result {
    size_t S = 0;
    std::vector<std::vector<double>> d, alpha, Kinv, P;
    std::vector<double> mse;
    std::vector<int32_t> path;
    explicit shyft_hip_krls_result(size_t S_) : S(S_), d(S_), alpha(S_), Kinv(S_), P(S_), mse(S_, 0.0), path(S_, 0) {}
};

namespace {

krls_in krls_prepare(const char* who, size_t S, const int64_t* row, const int64_t* t, const double* v, const int64_t* t_end,
                     const int32_t* fx, const int64_t* dt, const double* gamma, const double* tolerance,
                     const int64_t* max_dict, const int64_t* offset, const int64_t* count, const int64_t* stride,
                     const int64_t* iterations, const double* mse_tol, const int64_t* s_row, const double* s_d,
                     const double* s_alpha, const double* s_Kinv, const double* s_P, shyft_hip_krls_result** result) {
    if (!result) throw std::runtime_error(std::string(who) + ": null argument");
    *result = nullptr;
    krls_in in{S, row, t, v, dt, gamma, tolerance, max_dict, offset, count, stride, iterations, mse_tol,
               s_row, s_d, s_alpha, s_Kinv, s_P, std::vector<int64_t>(S + 1, 0)};
    if (S == 0) return in;
    check_point_series(who, "krls", S, row, t, v, t_end, fx);
    if (!dt || !gamma || !tolerance || !max_dict || !offset || !count || !stride || !iterations || !mse_tol)
        throw std::runtime_error(std::string(who) + ": null argument");
    for (size_t s = 0; s < S; ++s) {
        h::krls_rbf_predictor::check_parameters(dt[s], gamma[s], tolerance[s], max_dict[s]);
        if (offset[s] < 0) throw std::runtime_error("krls: offset must not be negative");
        if (stride[s] < 1) throw std::runtime_error("krls: stride must be greater than 0");
        if (iterations[s] < 0) throw std::runtime_error("krls: iterations must not be negative");
    }
    if (s_row) {
        check_csr_rows("krls starting state", S, s_row);
        if (s_row[S] > 0 && (!s_d || !s_alpha || !s_Kinv || !s_P)) throw std::runtime_error(std::string(who) + ": null argument");
        for (size_t s = 0; s < S; ++s) {
            const int64_t m0 = s_row[s + 1] - s_row[s];
            if (m0 > (int64_t(1) << 20)) throw std::runtime_error("krls: a starting dictionary above 2^20 entries is not supported");
            in.s_mat[s + 1] = in.s_mat[s] + m0 * m0;
        }
    }
    return in;
}

void krls_train_on_host(const krls_in& in, size_t s, shyft_hip_krls_result& R) {
    h::krls_rbf_predictor p(in.dt[s], in.gamma[s], in.tolerance[s], size_t(in.max_dict[s]));
    const size_t m0 = size_t(in.m0(s));
    if (m0)
        p.set_state(m0, in.s_d + in.s_row[s], in.s_alpha + in.s_row[s], in.s_Kinv + in.s_mat[s], in.s_P + in.s_mat[s]);
    R.mse[s] = p.train(in.t + in.row[s], in.v + in.row[s], in.n(s), size_t(in.offset[s]), in.count[s],
                       size_t(in.stride[s]), size_t(in.iterations[s]), in.mse_tol[s]);
    const size_t m = p.dictionary_size();
    R.d[s].resize(m);
    R.alpha[s].resize(m);
    R.Kinv[s].resize(m * m);
    R.P[s].resize(m * m);
    p.get_state(R.d[s].data(), R.alpha[s].data(), R.Kinv[s].data(), R.P[s].data());
    R.path[s] = SHYFT_HIP_KRLS_PATH_HOST;
}

call_record g_krls;
std::atomic<int> g_krls_path{0};  // shyft_hip_krls_set_path
constexpr const char* KRLS_UPLOAD = "krls upload";
constexpr const char* KRLS_DOWNLOAD = "krls download";

struct krls_device_inputs {  // uploaded once, shared by the two rounds
    dbuf<int64_t> t;
    dbuf<double> v, s_d, s_alpha, s_Kinv, s_P;
};

// One launch of krls_train_k over `series` with the capacity `cap`, and of krls_pack_k over what finished. Fills R for
// the series that finished and returns the status of every series of the round. Adds the kernels' milliseconds to ms.
std::vector<int32_t> krls_device_round(device_call& c, const krls_in& in, const krls_device_inputs& D, bool in_lds, int cap,
                                       const std::vector<size_t>& series, shyft_hip_krls_result& R, double& ms) {
    const size_t nj = series.size();
    const int ld = krls_ld(cap);
    const size_t slab_stride = 2 * size_t(cap) + 2 * size_t(cap) * ld;
    if (nj > size_t(std::numeric_limits<int>::max())) throw std::runtime_error("krls: too many series for one launch");
    const size_t lds = krls_lds_bytes(cap, in_lds);
    int lds_limit = 0;
    hip_check(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, c.dev), "hipDeviceGetAttribute");
    if (lds > size_t(lds_limit))
        throw std::runtime_error("krls: the device gives a workgroup " + std::to_string(lds_limit) + " bytes of LDS, the kernel needs " +
                                 std::to_string(lds));
    size_t free_b = 0, total_b = 0;
    hip_check(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
    if (slab_stride * sizeof(double) > free_b / nj)
        throw std::runtime_error("krls: " + std::to_string(nj) + " series with a dictionary capacity of " + std::to_string(cap) +
                                 " need " + std::to_string(nj * slab_stride * sizeof(double)) + " bytes of device memory, " +
                                 std::to_string(free_b) + " are free; train fewer series in one call");
    std::vector<krls_job> jobs(nj);
    for (size_t b = 0; b < nj; ++b) {
        const size_t s = series[b];
        krls_job& j = jobs[b];
        j.r0 = in.row[s];
        j.offset = in.offset[s];
        j.dim = int64_t(in.dim(s));
        j.stride = in.stride[s];
        j.iterations = in.iterations[s];
        j.max_dict = in.max_dict[s];
        j.scaling_f = h::krls_scaling(in.dt[s]);
        j.gamma = in.gamma[s];
        j.tolerance = in.tolerance[s];
        j.mse_tol = in.mse_tol[s];
        j.m0 = in.m0(s);
        j.s_vec = in.s_row ? in.s_row[s] : 0;
        j.s_mat = in.s_mat[s];
    }
    dbuf<krls_job> d_jobs;
    dbuf<double> d_slab, d_mse;
    dbuf<int64_t> d_m;
    dbuf<int32_t> d_status;
    c.upload(d_jobs, jobs.data(), nj, KRLS_UPLOAD);
    d_slab.alloc(nj * slab_stride);
    d_m.alloc(nj);
    d_status.alloc(nj);
    d_mse.alloc(nj);
    krls_train_args a{d_jobs.p, D.t.p, D.v.p, D.s_d.p, D.s_alpha.p, D.s_Kinv.p, D.s_P.p, d_slab.p, int64_t(slab_stride),
                      cap, ld, d_m.p, d_status.p, d_mse.p};
    if (in_lds)
        hip_check(hipFuncSetAttribute(reinterpret_cast<const void*>(&krls_train_k<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)), "hipFuncSetAttribute");
    c.begin();
    if (in_lds) hipLaunchKernelGGL(krls_train_k<true>, dim3(unsigned(nj)), dim3(KRLS_BLOCK), lds, c.s, a);
    else hipLaunchKernelGGL(krls_train_k<false>, dim3(unsigned(nj)), dim3(KRLS_BLOCK), lds, c.s, a);
    hip_check(hipGetLastError(), "krls_train");
    c.end();
    std::vector<int64_t> m(nj), v_off(nj + 1, 0), m_off(nj + 1, 0);
    std::vector<int32_t> status(nj);
    std::vector<double> mse(nj);
    c.download(m.data(), d_m.p, nj, KRLS_DOWNLOAD);
    c.download(status.data(), d_status.p, nj, KRLS_DOWNLOAD);
    c.download(mse.data(), d_mse.p, nj, KRLS_DOWNLOAD);
    ms += c.finish("krls_train");
    for (size_t b = 0; b < nj; ++b) {
        if (status[b] != 0) m[b] = 0;
        if (m[b] < 0 || m[b] > cap) throw std::runtime_error("krls: the device returned a dictionary size outside its capacity");
        v_off[b + 1] = v_off[b] + m[b];
        m_off[b + 1] = m_off[b] + m[b] * m[b];
    }
    const size_t nv = size_t(v_off[nj]), nm = size_t(m_off[nj]);
    std::vector<double> pd(nv), pa(nv), pK(nm), pP(nm);
    if (v_off[nj] > 0) {
        dbuf<int64_t> d_pm, d_voff, d_moff;
        dbuf<double> d_pd, d_pa, d_pK, d_pP;
        c.upload(d_pm, m.data(), nj, KRLS_UPLOAD);
        c.upload(d_voff, v_off.data(), nj, KRLS_UPLOAD);
        c.upload(d_moff, m_off.data(), nj, KRLS_UPLOAD);
        d_pd.alloc(pd.size());
        d_pa.alloc(pa.size());
        d_pK.alloc(pK.size());
        d_pP.alloc(pP.size());
        krls_pack_args pk{d_slab.p, int64_t(slab_stride), cap, ld, d_pm.p, d_voff.p, d_moff.p, d_pd.p, d_pa.p, d_pK.p, d_pP.p};
        c.begin();
        hipLaunchKernelGGL(krls_pack_k, dim3(unsigned(nj)), dim3(KRLS_BLOCK), 0, c.s, pk);
        hip_check(hipGetLastError(), "krls_pack");
        c.end();
        c.download(pd.data(), d_pd.p, pd.size(), KRLS_DOWNLOAD);
        c.download(pa.data(), d_pa.p, pa.size(), KRLS_DOWNLOAD);
        c.download(pK.data(), d_pK.p, pK.size(), KRLS_DOWNLOAD);
        c.download(pP.data(), d_pP.p, pP.size(), KRLS_DOWNLOAD);
        ms += c.finish("krls_pack");
    }
    for (size_t b = 0; b < nj; ++b) {
        if (status[b] != 0) continue;
        const size_t s = series[b];
        R.d[s].assign(pd.begin() + v_off[b], pd.begin() + v_off[b + 1]);
        R.alpha[s].assign(pa.begin() + v_off[b], pa.begin() + v_off[b + 1]);
        R.Kinv[s].assign(pK.begin() + m_off[b], pK.begin() + m_off[b + 1]);
        R.P[s].assign(pP.begin() + m_off[b], pP.begin() + m_off[b + 1]);
        R.mse[s] = mse[b];
        R.path[s] = in_lds ? SHYFT_HIP_KRLS_PATH_LDS : SHYFT_HIP_KRLS_PATH_WORKSPACE;
    }
    return status;
}

// the predictors as the predict entries take them, checked; true when there is nothing to do
bool krls_predict_prepare(const char* who, size_t S, const int64_t* d_row, const double* d, const double* alpha,
                          const int64_t* dt, const double* gamma, const int64_t* q_row, const int64_t* q_t, const double* out) {
    if (S == 0) return true;
    if (!d_row || !dt || !gamma || !q_row) throw std::runtime_error(std::string(who) + ": null argument");
    check_csr_rows("krls dictionary", S, d_row);
    check_csr_rows("krls output times", S, q_row);
    if (d_row[S] > 0 && (!d || !alpha)) throw std::runtime_error(std::string(who) + ": null argument");
    for (size_t s = 0; s < S; ++s) h::krls_rbf_predictor::check_parameters(dt[s], gamma[s], 0.0, 1);
    if (q_row[S] == 0) return true;
    if (!q_t || !out) throw std::runtime_error(std::string(who) + ": null argument");
    return false;
}

}  // namespace

extern "C" {

int shyft_hip_krls_train_csr(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, const int64_t* dt, const double* gamma,
                             const double* tolerance, const int64_t* max_dict, const int64_t* offset, const int64_t* count,
                             const int64_t* stride, const int64_t* iterations, const double* mse_tol, const int64_t* s_row,
                             const double* s_d, const double* s_alpha, const double* s_Kinv, const double* s_P,
                             shyft_hip_krls_result** result) {
    try {
        const krls_in in = krls_prepare("shyft_hip_krls_train_csr", S, row, t, v, t_end, fx, dt, gamma, tolerance, max_dict,
                                        offset, count, stride, iterations, mse_tol, s_row, s_d, s_alpha, s_Kinv, s_P, result);
        std::unique_ptr<shyft_hip_krls_result> R(new shyft_hip_krls_result(S));
        if (S == 0) {
            *result = R.release();
            return 0;
        }
        // bound[s]: what the dictionary of series s can reach by counting, its start plus every training sample
        std::vector<int64_t> bound(S);
        for (size_t s = 0; s < S; ++s) {
            int64_t valid = 0;
            const size_t dim = in.dim(s);
            for (size_t i = size_t(offset[s]); i < dim; i += size_t(stride[s])) valid += !(v[row[s] + i] != v[row[s] + i]);
            const int64_t room = std::numeric_limits<int64_t>::max() / 2;
            bound[s] = (iterations[s] > 0 && valid > room / iterations[s]) ? room : in.m0(s) + valid * iterations[s];
        }
        // The storages, smallest first: LDS for KRLS_LDS_SMALL_CAP entries (17 KB, so that eight workgroups share a CU
        // when a batch of short dictionaries is larger than the CU count), LDS for KRLS_LDS_CAP entries (the whole
        // CU), then the workspace. A series starts in the first storage that holds its starting dictionary. One whose
        // bound fits a storage cannot overflow there; any other is tried there all the same, a short dictionary being
        // cheapest there and the steps up to a small capacity cheap, and moves on when the kernel reports that it
        // wanted to pass the capacity.
        const bool use_lds = g_krls_path.load() != SHYFT_HIP_KRLS_PATH_WORKSPACE;
        std::vector<size_t> pending(S), host_round;
        for (size_t s = 0; s < S; ++s) pending[s] = s;
        double ms = 0.0;
        {
            device_call c(device);
            krls_device_inputs D;
            const size_t np = size_t(row[S]);
            c.upload(D.t, t, np, KRLS_UPLOAD);
            c.upload(D.v, v, np, KRLS_UPLOAD);
            if (s_row) {
                c.upload(D.s_d, s_d, size_t(s_row[S]), KRLS_UPLOAD);
                c.upload(D.s_alpha, s_alpha, size_t(s_row[S]), KRLS_UPLOAD);
                c.upload(D.s_Kinv, s_Kinv, size_t(in.s_mat[S]), KRLS_UPLOAD);
                c.upload(D.s_P, s_P, size_t(in.s_mat[S]), KRLS_UPLOAD);
            }
            for (int storage = use_lds ? 0 : 2; storage < 3; ++storage) {
                const bool in_lds = storage < 2;
                int64_t cap = storage == 0 ? KRLS_LDS_SMALL_CAP : KRLS_LDS_CAP;
                if (!in_lds) {  // the workspace is as large as the longest dictionary left can become
                    cap = 1;
                    for (size_t s : pending) cap = std::max(cap, std::max(in.m0(s), std::min(bound[s], max_dict[s])));
                    cap = std::min<int64_t>(cap, KRLS_MAX_DICT);
                }
                std::vector<size_t> round, later;
                for (size_t s : pending) (in.m0(s) <= cap ? round : later).push_back(s);
                if (!round.empty()) {
                    const std::vector<int32_t> st = krls_device_round(c, in, D, in_lds, int(cap), round, *R, ms);
                    for (size_t b = 0; b < round.size(); ++b) {
                        if (st[b] == 1) later.push_back(round[b]);
                        if (st[b] == 2) host_round.push_back(round[b]);
                    }
                }
                pending.swap(later);
            }
            g_krls.record(c.dev, ms);
        }
        host_round.insert(host_round.end(), pending.begin(), pending.end());  // beyond KRLS_MAX_DICT
        for (size_t s : host_round) krls_train_on_host(in, s, *R);
        *result = R.release();
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_krls_train_csr_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                  const int64_t* t_end, const int32_t* fx, const int64_t* dt, const double* gamma,
                                  const double* tolerance, const int64_t* max_dict, const int64_t* offset,
                                  const int64_t* count, const int64_t* stride, const int64_t* iterations,
                                  const double* mse_tol, const int64_t* s_row, const double* s_d, const double* s_alpha,
                                  const double* s_Kinv, const double* s_P, shyft_hip_krls_result** result) {
    (void)device;
    try {
        const krls_in in = krls_prepare("shyft_hip_krls_train_csr_host", S, row, t, v, t_end, fx, dt, gamma, tolerance,
                                        max_dict, offset, count, stride, iterations, mse_tol, s_row, s_d, s_alpha, s_Kinv, s_P,
                                        result);
        std::unique_ptr<shyft_hip_krls_result> R(new shyft_hip_krls_result(S));
        for (size_t s = 0; s < S; ++s) krls_train_on_host(in, s, *R);
        *result = R.release();
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_krls_result_sizes(const shyft_hip_krls_result* result, size_t S, int64_t* d_row) {
    if (!result || !d_row || result->S != S) return fail(nullptr, "shyft_hip_krls_result_sizes: bad argument");
    d_row[0] = 0;
    for (size_t s = 0; s < S; ++s) d_row[s + 1] = d_row[s] + int64_t(result->d[s].size());
    return 0;
}

int shyft_hip_krls_result_fetch(const shyft_hip_krls_result* result, size_t S, double* d, double* alpha, double* Kinv,
                                double* P, double* mse, int32_t* path) {
    if (!result || result->S != S || (S && (!mse || !path))) return fail(nullptr, "shyft_hip_krls_result_fetch: bad argument");
    size_t vo = 0, mo = 0;
    for (size_t s = 0; s < S; ++s) {
        const size_t m = result->d[s].size();
        if (m && (!d || !alpha || !Kinv || !P)) return fail(nullptr, "shyft_hip_krls_result_fetch: null argument");
        std::copy(result->d[s].begin(), result->d[s].end(), d + vo);
        std::copy(result->alpha[s].begin(), result->alpha[s].end(), alpha + vo);
        std::copy(result->Kinv[s].begin(), result->Kinv[s].end(), Kinv + mo);
        std::copy(result->P[s].begin(), result->P[s].end(), P + mo);
        mse[s] = result->mse[s];
        path[s] = result->path[s];
        vo += m;
        mo += m * m;
    }
    return 0;
}

void shyft_hip_krls_result_free(shyft_hip_krls_result* result) { delete result; }

int shyft_hip_krls_predict(int device, size_t S, const int64_t* d_row, const double* d, const double* alpha,
                           const int64_t* dt, const double* gamma, const int64_t* q_row, const int64_t* q_t,
                           const double* q_v, double* out) {
    try {
        if (krls_predict_prepare("shyft_hip_krls_predict", S, d_row, d, alpha, dt, gamma, q_row, q_t, out)) return 0;
        std::vector<int64_t> tile_s, tile_i0;
        std::vector<double> scaling(S);
        for (size_t s = 0; s < S; ++s) {
            scaling[s] = h::krls_scaling(dt[s]);
            for (int64_t i0 = 0; i0 < q_row[s + 1] - q_row[s]; i0 += KRLS_BLOCK) {
                tile_s.push_back(int64_t(s));
                tile_i0.push_back(i0);
            }
        }
        const size_t nq = size_t(q_row[S]), ntiles = tile_s.size();
        device_call c(device);
        dbuf<int64_t> d_tile_s, d_tile_i0, d_drow, d_qrow, d_qt;
        dbuf<double> d_d, d_alpha, d_scaling, d_gamma, d_qv, d_out;
        c.upload(d_tile_s, tile_s.data(), ntiles, KRLS_UPLOAD);
        c.upload(d_tile_i0, tile_i0.data(), ntiles, KRLS_UPLOAD);
        c.upload(d_drow, d_row, S + 1, KRLS_UPLOAD);
        c.upload(d_d, d, size_t(d_row[S]), KRLS_UPLOAD);
        c.upload(d_alpha, alpha, size_t(d_row[S]), KRLS_UPLOAD);
        c.upload(d_scaling, scaling.data(), S, KRLS_UPLOAD);
        c.upload(d_gamma, gamma, S, KRLS_UPLOAD);
        c.upload(d_qrow, q_row, S + 1, KRLS_UPLOAD);
        c.upload(d_qt, q_t, nq, KRLS_UPLOAD);
        if (q_v) c.upload(d_qv, q_v, nq, KRLS_UPLOAD);
        d_out.alloc(nq);
        krls_predict_args a{int64_t(ntiles), d_tile_s.p, d_tile_i0.p, d_drow.p, d_d.p, d_alpha.p, d_scaling.p, d_gamma.p,
                            d_qrow.p, d_qt.p, q_v ? d_qv.p : nullptr, d_out.p};
        c.begin();
        hipLaunchKernelGGL(krls_predict_k, dim3(launch_blocks(ntiles)), dim3(KRLS_BLOCK), 0, c.s, a);  // the tile loop takes the rest
        hip_check(hipGetLastError(), "krls_predict");
        c.end();
        c.download(out, d_out.p, nq, KRLS_DOWNLOAD);
        g_krls.record(c.dev, c.finish("krls_predict"));
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_krls_predict_host(int device, size_t S, const int64_t* d_row, const double* d, const double* alpha,
                                const int64_t* dt, const double* gamma, const int64_t* q_row, const int64_t* q_t,
                                const double* q_v, double* out) {
    (void)device;
    try {
        if (krls_predict_prepare("shyft_hip_krls_predict_host", S, d_row, d, alpha, dt, gamma, q_row, q_t, out)) return 0;
        for (size_t s = 0; s < S; ++s) {
            const double scaling_f = h::krls_scaling(dt[s]);
            const size_t m = size_t(d_row[s + 1] - d_row[s]);
            for (int64_t i = q_row[s]; i < q_row[s + 1]; ++i) {
                const double f = h::krls_f(gamma[s], d + d_row[s], alpha + d_row[s], m, h::krls_position(q_t[i], scaling_f));
                const double v = q_v ? q_v[i] : 0.0;
                out[i] = q_v ? (v != v ? v : v - f) : f;
            }
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

double shyft_hip_krls_last_ms(int device) { return g_krls.last_ms.load(device, 0.0); }

int shyft_hip_krls_set_path(int path) {
    if (path != 0 && path != SHYFT_HIP_KRLS_PATH_WORKSPACE) return fail(nullptr, "krls: path must be 0 or SHYFT_HIP_KRLS_PATH_WORKSPACE");
    g_krls_path.store(path);
    return 0;
}

}  // extern "C"
