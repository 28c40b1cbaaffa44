// Host restatement of the reference's KRLS predictor with a radial-basis kernel: prediction::krls_rbf_predictor
// (core/predictions.h:30-343) over dlib::krls, and so krls_interpolation_ts (core/time_series_dd.h:1368-1442). C++17; the
// few functions marked KRLS_FN are also compiled for the device by kernels/krls.hip, which is bit-identical to this file
// in the dictionary, the weights, both matrices, the mse and every predicted value. The _host entries of the C ABI run
// this file on one thread.
//
// dlib is not a dependency. Its krls::train is restated from the published recursion (Engel, Mannor, Meir 2004, "The
// kernel recursive least-squares algorithm", eqs. 3.12-3.16), in the form dlib implements it. Last-bit parity with dlib
// is NOT pinned; the reference's two Python tests are.
//
// State of a predictor: dictionary d[0..m) of sample positions, weights alpha[0..m), the full m x m matrices Kinv and P
// (P is not kept symmetric by the update, so both are stored and read in full), and K, the kernel matrix of the
// dictionary, which only the removal of a dictionary entry reads (host only).
//
//  kernel      k(a, b) = exp(-gamma * ((a - b) * (a - b))), exp = detmath::exp
//  position    x = to_seconds(t) * (1.0 / to_seconds(dt)) in train, predict(ta), predictor_mse, mse_ts
//              (predictions.h:152,165,198,202); the scalar predict(t) divides, to_seconds(t) / to_seconds(dt) (:235)
//  train(x, y) first sample: d = [x], alpha = [y / 1.0], Kinv = [[1 / 1.0]], P = [[1]]. Later samples:
//              k_i = k(x, d_i); a = Kinv k; delta = 1.0 - k.a; e = y - k.alpha
//              delta > tolerance, grow (after the removal of entry 0 and a recomputation of k, a, delta, e when
//              m == max_dict_size):
//                Kinv <- [[Kinv_ij + (a_i * a_j) / delta, -a_i / delta], [-a_j / delta, 1.0 / delta]]
//                P <- [[P, 0], [0, 1]]; ka = e / delta; alpha_i <- alpha_i - a_i * ka; alpha <- [alpha, ka]; d <- [d, x]
//              otherwise, update:
//                Pa = P a; q = Pa / (1.0 + a.Pa); r_j = sum_i a_i * P_ij; P_ij <- P_ij - q_i * r_j
//                alpha_i <- alpha_i + (sum_j Kinv_ij * q_j) * e
//  removal     Kinv' = removerc(Kinv, 0, 0) - (col0 / Kinv_00) row0; alpha' = Kinv' ((K without row 0) alpha), the inner
//              product first; row and column 0 of P and K dropped
//  f(x)        sum_i alpha_i * k(x, d_i), one accumulator in index order (predict, predictor_mse, mse_ts)
//
// Arithmetic rules. No FMA (-ffp-contract=off). Every element of a matrix-vector product is one accumulator that adds
// its terms in index order. The four scalar products inside train -- k.a, k.alpha, a.Pa and the f(x) of the running
// mse -- use krls_dot: 64 accumulators, accumulator l adding the terms i = l, l + 64, ... in that order, then the
// fixed tree p[l] += p[l + o] for o = 32, 16, .. 1. That is what one wavefront computes with a strided loop and six
// cross-lane exchanges, so the device reproduces it exactly. The running mse itself adds diff * diff point by point.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../detmath/detmath.h"
#include "time_series.hpp"

#if defined(__HIPCC__)
#define KRLS_FN __host__ __device__ inline
#else
#define KRLS_FN inline
#endif

namespace shyft_hip::host {

KRLS_FN double krls_kernel(double gamma, double a, double b) {
    const double d = a - b;
    return detmath::exp(-gamma * (d * d));
}

// the sample position of a time (predictions.h:152,165): a multiplication by the reciprocal
KRLS_FN double krls_scaling(int64_t dt) { return 1.0 / (double(dt) / 1e6); }
KRLS_FN double krls_position(int64_t t, double scaling_f) { return (double(t) / 1e6) * scaling_f; }

// krls::operator(): f(x) = sum_i alpha_i * k(x, d_i), one accumulator in index order
KRLS_FN double krls_f(double gamma, const double* d, const double* alpha, size_t m, double x) {
    double acc = 0.0;
    for (size_t i = 0; i < m; ++i) acc = acc + alpha[i] * krls_kernel(gamma, x, d[i]);
    return acc;
}

// dim of train and predictor_mse (predictions.h:150,262): min(offset + count * stride, size). The reference's unsigned
// product wraps; here it saturates, so that its default count (the largest size_t) means "to the end" at any offset.
// A negative count is that default.
inline size_t krls_dim(size_t offset, int64_t count, size_t stride, size_t size) {
    if (count < 0) return size;
    if (stride != 0 && size_t(count) > (size - std::min(size, offset)) / stride) return size;
    return std::min(offset + size_t(count) * stride, size);
}

// the association of the scalar products inside train, see the file header
inline double krls_dot(const double* u, const double* v, size_t m) {
    double p[64];
    for (int l = 0; l < 64; ++l) p[l] = 0.0;
    for (size_t i = 0; i < m; ++i) p[i & 63] = p[i & 63] + u[i] * v[i];
    for (int o = 32; o >= 1; o /= 2)
        for (int l = 0; l < o; ++l) p[l] = p[l] + p[l + o];
    return p[0];
}

class krls_rbf_predictor {
  public:
    utctimespan dt = 0;
    double gamma = 0.0, tolerance = 0.0;
    size_t max_dict_size = 0;
    ts_point_fx predicted_point_fx = POINT_AVERAGE_VALUE;

    krls_rbf_predictor() = default;
    // the conditions of dlib::krls's and the kernel's constructors, and a dt that can be divided by
    krls_rbf_predictor(utctimespan dt_, double gamma_, double tolerance_, size_t size = 1000000u,
                       ts_point_fx fx = POINT_AVERAGE_VALUE)
        : dt(dt_), gamma(gamma_), tolerance(tolerance_), max_dict_size(size), predicted_point_fx(fx) {
        check_parameters(dt_, gamma_, tolerance_, int64_t(std::min(size, size_t(std::numeric_limits<int64_t>::max()))));
    }
    static void check_parameters(int64_t dt, double gamma, double tolerance, int64_t size) {
        if (!(dt > 0)) throw std::runtime_error("krls: dt must be greater than 0");
        if (!(gamma >= 0.0)) throw std::runtime_error("krls: gamma must not be negative");
        if (!(tolerance >= 0.0)) throw std::runtime_error("krls: tolerance must not be negative");
        if (size <= 0) throw std::runtime_error("krls: the dictionary size must be greater than 0");
    }

    size_t dictionary_size() const { return m; }
    void clear() {  // krls::clear_dictionary
        m = 0;
        d.clear();
        alpha.clear();
    }

    // the state as dense m x m matrices, row-major
    void get_state(double* d_out, double* alpha_out, double* Kinv_out, double* P_out) const {
        for (size_t i = 0; i < m; ++i) {
            d_out[i] = d[i];
            alpha_out[i] = alpha[i];
            for (size_t j = 0; j < m; ++j) {
                Kinv_out[i * m + j] = Kinv[i * ld + j];
                P_out[i * m + j] = P[i * ld + j];
            }
        }
    }
    // K is rebuilt from the dictionary: K_ij = k(d_i, d_j) is what train stored when the later of the two joined
    void set_state(size_t m_in, const double* d_in, const double* alpha_in, const double* Kinv_in, const double* P_in) {
        clear();
        reserve(m_in);
        m = m_in;
        d.assign(d_in, d_in + m);
        alpha.assign(alpha_in, alpha_in + m);
        for (size_t i = 0; i < m; ++i)
            for (size_t j = 0; j < m; ++j) {
                Kinv[i * ld + j] = Kinv_in[i * m + j];
                P[i * ld + j] = P_in[i * m + j];
                K[i * ld + j] = i >= j ? krls_kernel(gamma, d[i], d[j]) : krls_kernel(gamma, d[j], d[i]);
            }
    }

    // krls::train(x, y), the caller skips a NaN y. Returns f(x) of the updated state in krls_dot's association.
    double train(double x, double y) {
        if (m == 0) {
            reserve(1);
            d.assign(1, x);
            alpha.assign(1, y / 1.0);
            Kinv[0] = 1.0 / 1.0;
            P[0] = 1.0;
            K[0] = krls_kernel(gamma, x, x);
            m = 1;
            k[0] = K[0];
            return krls_dot(alpha.data(), k.data(), m);
        }
        double delta, e;
        project(x, y, delta, e);
        if (delta > tolerance) {
            if (m >= max_dict_size) {
                remove_first();
                if (m == 0) return train(x, y);  // max_dict_size == 1: the new sample is the whole dictionary
                project(x, y, delta, e);
            }
            reserve(m + 1);
            for (size_t i = 0; i < m; ++i) {
                for (size_t j = 0; j < m; ++j) Kinv[i * ld + j] = Kinv[i * ld + j] + (a[i] * a[j]) / delta;
                Kinv[i * ld + m] = -a[i] / delta;
                Kinv[m * ld + i] = -a[i] / delta;
                P[i * ld + m] = 0.0;
                P[m * ld + i] = 0.0;
                K[i * ld + m] = k[i];
                K[m * ld + i] = k[i];
            }
            Kinv[m * ld + m] = 1.0 / delta;
            P[m * ld + m] = 1.0;
            k[m] = krls_kernel(gamma, x, x);
            K[m * ld + m] = k[m];
            const double ka = e / delta;
            for (size_t i = 0; i < m; ++i) alpha[i] = alpha[i] - a[i] * ka;
            alpha.push_back(ka);
            d.push_back(x);
            ++m;
        } else {
            for (size_t i = 0; i < m; ++i) Pa[i] = row_dot(P, i, a);
            const double s = 1.0 + krls_dot(a.data(), Pa.data(), m);
            for (size_t i = 0; i < m; ++i) q[i] = Pa[i] / s;
            for (size_t j = 0; j < m; ++j) {  // a' P: down column j
                double acc = 0.0;
                for (size_t i = 0; i < m; ++i) acc = acc + a[i] * P[i * ld + j];
                r[j] = acc;
            }
            for (size_t i = 0; i < m; ++i)
                for (size_t j = 0; j < m; ++j) P[i * ld + j] = P[i * ld + j] - q[i] * r[j];
            for (size_t i = 0; i < m; ++i) alpha[i] = alpha[i] + row_dot(Kinv, i, q) * e;
        }
        return krls_dot(alpha.data(), k.data(), m);
    }

    // krls_rbf_predictor::train (predictions.h:139-181) on the points t[0..n), v[0..n)
    double train(const utctime* t, const double* v, size_t n, size_t offset = 0, int64_t count = -1, size_t stride = 1,
                 size_t iterations = 1, double mse_tol = 0.001) {
        if (stride == 0) throw std::runtime_error("krls: stride must be greater than 0");
        double mse = 0.0;
        const size_t dim = krls_dim(offset, count, stride, n);
        const double scaling_f = krls_scaling(dt);
        size_t iter_count = 0;
        while (iter_count++ < iterations) {
            mse = 0.0;
            size_t nan_count = 0;
            for (size_t i = offset; i < dim; i += stride) {
                const double pv = v[i];
                if (!(pv != pv)) {
                    const double diff_v = pv - train(krls_position(t[i], scaling_f), pv);
                    mse = mse + diff_v * diff_v;
                } else {
                    nan_count += 1;
                }
            }
            mse = mse / std::max(double(dim - nan_count), 1.);  // as the reference writes it: the stride is ignored
            if (mse < mse_tol) return mse;
        }
        return mse;
    }
    double train(const point_ts& ts, size_t offset = 0, int64_t count = -1, size_t stride = 1, size_t iterations = 1,
                 double mse_tol = 0.001) {
        return train(ts.t.data(), ts.v.data(), ts.size(), offset, count, stride, iterations, mse_tol);
    }

    double f(double x) const { return krls_f(gamma, d.data(), alpha.data(), m, x); }
    // predict_vec (predictions.h:193-207)
    std::vector<double> predict_vec(const utctime* t, size_t n) const {
        std::vector<double> out(n);
        const double scaling_f = krls_scaling(dt);
        for (size_t i = 0; i < n; ++i) out[i] = f(krls_position(t[i], scaling_f));
        return out;
    }
    point_ts predict(const point_ts& axis) const {
        point_ts out = axis;
        out.v = predict_vec(axis.t.data(), axis.size());
        out.fx = predicted_point_fx;
        return out;
    }
    // the scalar predict (predictions.h:232-237): a division
    double predict(utctime t) const { return f(to_seconds(t) / to_seconds(dt)); }

    // predictor_mse (predictions.h:253-282). As the reference writes it, the loop steps by one and the stride only
    // enters dim.
    double predictor_mse(const point_ts& ts, size_t offset = 0, int64_t count = -1, size_t stride = 1) const {
        size_t nan_count = 0;
        double mse = 0.0;
        const size_t dim = krls_dim(offset, count, stride, ts.size());
        const double scaling_f = krls_scaling(dt);
        for (size_t i = offset; i < dim; ++i) {
            const double pv = ts.v[i];
            if (!(pv != pv)) {
                const double diff_v = pv - f(krls_position(ts.t[i], scaling_f));
                mse = mse + diff_v * diff_v;
            } else {
                nan_count += 1;
            }
        }
        return mse / std::max(double(dim - nan_count), 1.);
    }
    // mse_ts (predictions.h:300-334): the mean squared residual of the points i - points .. i + points
    point_ts mse_ts(const point_ts& ts, size_t points) const {
        point_ts out = ts;
        const double scaling_f = krls_scaling(dt);
        const size_t dim = ts.size();
        for (size_t i = 0; i < dim; ++i) {
            size_t count = 0;
            double acc = 0.0;
            const size_t j_low = i < points ? 0u : i - points;
            const size_t j_high = (points >= dim || i + points + 1u > dim) ? dim : i + points + 1u;
            for (size_t j = j_low; j < j_high; ++j) {
                const double ts_v = ts.v[j];
                if (!(ts_v != ts_v)) {
                    count += 1;
                    const double diff_v = ts_v - f(krls_position(ts.t[j], scaling_f));
                    acc = acc + diff_v * diff_v;
                }
            }
            out.v[i] = count != 0 ? acc / double(count) : std::numeric_limits<double>::quiet_NaN();
        }
        return out;
    }

  private:
    size_t m = 0, ld = 0;  // ld: the allocated rows and columns of the matrices
    std::vector<double> d, alpha, Kinv, P, K;
    std::vector<double> k, a, Pa, r, q;  // scratch of train

    double row_dot(const std::vector<double>& M, size_t i, const std::vector<double>& x) const {
        double acc = 0.0;
        for (size_t j = 0; j < m; ++j) acc = acc + M[i * ld + j] * x[j];
        return acc;
    }
    // k, a, delta and e of a sample against the current dictionary
    void project(double x, double y, double& delta, double& e) {
        for (size_t i = 0; i < m; ++i) k[i] = krls_kernel(gamma, x, d[i]);
        for (size_t i = 0; i < m; ++i) a[i] = row_dot(Kinv, i, k);
        delta = 1.0 - krls_dot(k.data(), a.data(), m);
        e = y - krls_dot(k.data(), alpha.data(), m);
    }
    void reserve(size_t rows) {
        if (rows <= ld) return;
        const size_t nld = std::max(rows, std::max<size_t>(8, 2 * ld));
        for (std::vector<double>* M : {&Kinv, &P, &K}) {
            std::vector<double> n(nld * nld, 0.0);
            for (size_t i = 0; i < m; ++i)
                for (size_t j = 0; j < m; ++j) n[i * nld + j] = (*M)[i * ld + j];
            M->swap(n);
        }
        ld = nld;
        for (std::vector<double>* s : {&k, &a, &Pa, &r, &q}) s->resize(ld, 0.0);
    }
    // krls::remove_dictionary_vector(0)
    void remove_first() {
        const size_t n = m - 1;
        std::vector<double> Kn(n * n), tmp(n), an(n);
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < n; ++j)
                Kn[i * n + j] = Kinv[(i + 1) * ld + (j + 1)] - (Kinv[(i + 1) * ld] / Kinv[0]) * Kinv[j + 1];
        for (size_t i = 0; i < n; ++i) {  // (K without row 0) alpha
            double acc = 0.0;
            for (size_t j = 0; j < m; ++j) acc = acc + K[(i + 1) * ld + j] * alpha[j];
            tmp[i] = acc;
        }
        for (size_t i = 0; i < n; ++i) {
            double acc = 0.0;
            for (size_t j = 0; j < n; ++j) acc = acc + Kn[i * n + j] * tmp[j];
            an[i] = acc;
        }
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < n; ++j) {
                Kinv[i * ld + j] = Kn[i * n + j];
                P[i * ld + j] = P[(i + 1) * ld + (j + 1)];
                K[i * ld + j] = K[(i + 1) * ld + (j + 1)];
            }
        alpha = an;
        d.erase(d.begin());
        m = n;
    }
};

}  // namespace shyft_hip::host
