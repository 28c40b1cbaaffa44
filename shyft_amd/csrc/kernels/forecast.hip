// Forecast skill by lead time for gfx950: the Nash-Sutcliffe score of P problems in one launch, each problem a set of
// forecasts against one observation over n slices that start a lead time into every forecast
// (core/time_series_merge.h:123-144 over average_accessor, core/time_series.h:2033-2072, and
// nash_sutcliffe_goal_function, :2316-2344; core/time_series_dd.cpp:1137-1165).
//
// The S series are one pool in the CSR form of kernels/resample.hip (row, t, v, t_end, fx); forecasts and observations
// sit together. Problem p names its forecasts fc_ix[fc_row[p] .. fc_row[p+1]) and its observation obs_ix[p] (-1: none)
// by index into the pool, and carries its own t0_offset, dt and n. Job (p, k, i) is slice i of forecast k of problem
// p and lies at job_row[p] + k * n_p + i; its period is [t[row[f]] + t0_offset + i * dt, + dt) with f the forecast.
// sim and obs [J] hold the slice averages of the forecast and of the observation by the AVERAGE rule of resample.hip
// (NaN when the period starts at or after the series' end, else area / to_seconds(tsum), NaN without covered time),
// ns [P] the score 1 - err2 / var2 over the jobs of a problem where both are finite. host/forecast.hpp holds the same
// statements in plain C++ and is the definition of correct; shyft_hip_forecast_skill_host runs those, not this file's.
//
// Every operation is evaluated as written: int64 tick arithmetic, to_seconds(x) = double(x) / 1e6 as a division, no
// FMA (-ffp-contract=off), isfinite by the exponent bits, every division a division. No atomics, no inline assembly.
//
// Launch shape. One wavefront takes one problem and loops grid-stride over the problems with 64-bit indexes; the
// problem index is the same in all 64 lanes, so every loop count below is uniform over the wavefront. The jobs of a
// problem go by in chunks of 64 consecutive jobs, lane l taking job c + l: two rs_area walks (device/ts_area.h),
// forecast and observation; a lane past the last job holds NaN for both. The reference forms its sums sequentially in
// job order, and so does every lane here: after a chunk's walks the 64 (sim, obs) pairs are read lane by lane in
// lane order (readlane with a constant lane, a register broadcast: no LDS, no barrier, and the lanes that only hold
// NaN add nothing, as a non-finite pair adds nothing in the reference) and every lane carries the same err2, mean and
// count. Pass 2 needs the mean of the whole problem, so each lane stores its two averages to sim and obs (device
// buffers of J doubles, allocated always, downloaded when asked for) and rereads them chunk by chunk with the same
// lane <-> job mapping: a lane reads only what it stored itself, so no visibility between lanes is assumed. Lane 0
// stores the score. There is no tree reduction anywhere: ns, sim and obs are bit-identical to the host twin.
//
// Index safety. The host checks before the launch: the series as in resample.hip (row a CSR inside the uploaded
// points, times strictly increasing, t_end after the last); fc_row a CSR inside the uploaded fc_ix; every fc_ix in
// [0, S) and naming a series with at least one point, so t[row[f]] exists; every obs_ix in [-1, S); dt > 0,
// t0_offset >= 0, n >= 0 and every slice axis inside a quarter of the int64 range, so no tick sum overflows.
// job_row is built on the host as the running sum of F_p * n_p, so job_row[p] + j with j < F_p * n_p lies inside the
// J doubles of sim and obs, and k = j / n_p < F_p. A problem with F_p * n_p == 0 runs no job (n_p is never a divisor
// then) and stores NaN. rs_area reads point k only with k < the series' point count (its own argument, ts_area.h); an
// observation without points is never read; the one place where the reference reads past a one-point series is
// refused by the host check (a one-point observation inside a period of any forecast's axis; a forecast's own first
// point can never lie inside a period that starts before it, since t0_offset >= 0). ns is written at p < P only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../device/ts_area.h"
#include "../host/forecast.hpp"
#include "../include_internal/device_call.h"
#include "../include_internal/series_args.h"

using namespace shyft_hip_impl;

namespace {

constexpr int FS_BLOCK = 256;  // 4 wavefronts, each with a problem of its own
constexpr int FS_WAVES = FS_BLOCK / 64;

struct fs_args {
    size_t P;
    const int64_t* row;
    const int64_t* t;
    const double* v;
    const int64_t* t_end;
    const int32_t* fx;
    const int64_t* fc_row;
    const int64_t* fc_ix;
    const int64_t* obs_ix;
    const int64_t* t0_offset;
    const int64_t* dt;
    const int64_t* n;
    const int64_t* job_row;
    double* ns;
    double* sim;
    double* obs;
};

// average_accessor::value of the period [ps, pe) over the np > 0 points of one series (rs_job of resample.hip, AVERAGE)
__device__ inline double fs_average(const int64_t* __restrict__ t, const double* __restrict__ v, int64_t np, int64_t t_end,
                                    bool linear, int64_t ps, int64_t pe) {
    if (ps >= t_end) return rs_nan();
    int64_t tsum = 0;
    const double area = rs_area(t, v, np, t_end, ps, pe, linear, tsum);
    return tsum > 0 ? area / rs_seconds(tsum) : rs_nan();
}

// the value that `lane` holds, in every lane; `lane` is a constant
__device__ inline double fs_lane_value(double x, int lane) {
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(FS_BLOCK) void forecast_skill_kernel(fs_args a) {
    const int lane = int(threadIdx.x & 63);
    const size_t wave = size_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    const size_t stride = size_t(gridDim.x) * FS_WAVES;
    for (size_t p = size_t(blockIdx.x) * FS_WAVES + wave; p < a.P; p += stride) {  // uniform over the wavefront
        const int64_t f0 = a.fc_row[p];
        const uint64_t F = uint64_t(a.fc_row[p + 1] - f0), n = uint64_t(a.n[p]);
        const uint64_t jobs = F * n;
        const int64_t j0 = a.job_row[p], off = a.t0_offset[p], dt = a.dt[p];
        const int64_t oi = a.obs_ix[p];
        int64_t o_r0 = 0, o_np = 0, o_end = 0;
        bool o_linear = false;
        if (oi >= 0) {
            o_r0 = a.row[oi];
            o_np = a.row[oi + 1] - o_r0;
            o_end = a.t_end[oi];
            o_linear = a.fx[oi] == int32_t(shyft_hip::host::POINT_INSTANT_VALUE);
        }
        // pass 1 (core/time_series.h:2320-2333): err2 += (o - m)^2, mean += o, ++count, in job order
        double err2 = 0.0, mean = 0.0;
        uint64_t count = 0;
        for (uint64_t c = 0; c < jobs; c += 64) {
            const uint64_t j = c + uint64_t(lane);
            double s = rs_nan(), o = rs_nan();
            if (j < jobs) {
                const uint64_t k = j / n, i = j % n;
                const int64_t f = a.fc_ix[f0 + int64_t(k)];
                const int64_t r0 = a.row[f], np = a.row[f + 1] - r0;
                const int64_t ps = a.t[r0] + off + int64_t(i) * dt, pe = ps + dt;
                s = fs_average(a.t + r0, a.v + r0, np, a.t_end[f],
                               a.fx[f] == int32_t(shyft_hip::host::POINT_INSTANT_VALUE), ps, pe);
                if (o_np > 0) o = fs_average(a.t + o_r0, a.v + o_r0, o_np, o_end, o_linear, ps, pe);
                a.sim[j0 + int64_t(j)] = s;
                a.obs[j0 + int64_t(j)] = o;
            }
#pragma unroll
            for (int l = 0; l < 64; ++l) {
                const double sl = fs_lane_value(s, l), ol = fs_lane_value(o, l);
                if (rs_finite(ol) && rs_finite(sl)) {
                    const double d = ol - sl;
                    err2 += d * d;
                    mean += ol;
                    ++count;
                }
            }
        }
        mean /= double(count);
        // pass 2 (:2334-2342): var2 += (o - mean)^2 over the same pairs, in job order; each lane rereads its own stores
        double var2 = 0.0;
        for (uint64_t c = 0; c < jobs; c += 64) {
            const uint64_t j = c + uint64_t(lane);
            double s = rs_nan(), o = rs_nan();
            if (j < jobs) {
                s = a.sim[j0 + int64_t(j)];
                o = a.obs[j0 + int64_t(j)];
            }
#pragma unroll
            for (int l = 0; l < 64; ++l) {
                const double sl = fs_lane_value(s, l), ol = fs_lane_value(o, l);
                if (rs_finite(ol) && rs_finite(sl)) {
                    const double d = ol - mean;
                    var2 += d * d;
                }
            }
        }
        if (lane == 0) a.ns[p] = jobs ? 1.0 - err2 / var2 : rs_nan();
    }
}

// Argument checks shared by the device and the host entry, with the same texts; fills job_row [P+1] and returns J.
size_t fs_prepare(const char* who, size_t S, const int64_t* row, const int64_t* t, const double* v, const int64_t* t_end,
                  const int32_t* fx, size_t P, const int64_t* fc_row, const int64_t* fc_ix, const int64_t* obs_ix,
                  const int64_t* t0_offset, const int64_t* dt, const int64_t* n, std::vector<int64_t>& job_row) {
    const int64_t i64max = std::numeric_limits<int64_t>::max();
    job_row.assign(P + 1, 0);
    if (S > 0 || P > 0) check_point_series(who, "forecast_skill", S, row, t, v, t_end, fx);
    if (P == 0) return 0;
    if (!fc_row || !obs_ix || !t0_offset || !dt || !n) throw std::runtime_error(std::string(who) + ": null argument");
    check_csr_rows("forecast_skill", P, fc_row);
    if (fc_row[P] > 0 && !fc_ix) throw std::runtime_error(std::string(who) + ": null argument");
    const size_t max_jobs = std::numeric_limits<size_t>::max() / sizeof(double) / 4;
    for (size_t p = 0; p < P; ++p) {
        // the argument texts of ats_vector::nash_sutcliffe / average_slice (core/time_series_dd.cpp:1138-1143)
        if (n[p] < 0) throw std::runtime_error("n, number of intervals, must be specified as > 0");
        if (dt[p] <= 0) throw std::runtime_error("dt, average interval, must be specified as > 0 s");
        if (t0_offset[p] < 0) throw std::runtime_error("lead_time,t0_offset,must be specified  >= 0 s");
        const int64_t oi = obs_ix[p];
        if (oi < -1 || oi >= int64_t(S))
            throw std::runtime_error("forecast_skill: an observation index lies outside the series");
        const bool one_point_obs = oi >= 0 && row[oi + 1] - row[oi] == 1;
        // the sums to_seconds(px.start + px.end) and p.end - p.start stay inside int64
        const bool wide = n[p] > 0 && (t0_offset[p] > i64max / 4 || n[p] > i64max / 4 / dt[p]);
        for (int64_t e = fc_row[p]; e < fc_row[p + 1]; ++e) {
            const int64_t f = fc_ix[e];
            if (f < 0 || f >= int64_t(S)) throw std::runtime_error("forecast_skill: a forecast index lies outside the series");
            // the reference asks an empty axis for time(0)
            if (row[f + 1] == row[f]) throw std::runtime_error("forecast_skill: a forecast has no points");
            if (n[p] == 0) continue;
            const int64_t ta_t0 = wide ? 0 : t[row[f]] + t0_offset[p];
            if (wide || ta_t0 > i64max / 4 - n[p] * dt[p])
                throw std::runtime_error("forecast_skill: times beyond a quarter of the 64-bit range are not supported");
            if (one_point_obs) {
                // accumulate_value reads point 1 of a one-point series when the point lies inside a period that starts
                // before it; the reference throws out of point_dt::time (core/time_axis.h:317-322)
                const int64_t tb = t[row[oi]], ta_end = ta_t0 + n[p] * dt[p];
                if (tb > ta_t0 && tb < ta_end && (tb - ta_t0) % dt[p] != 0)
                    throw std::runtime_error("point_dt.time(i): a one-point series cannot be integrated over a period "
                                             "that starts before its point and holds it");
            }
        }
        const uint64_t F = uint64_t(fc_row[p + 1] - fc_row[p]);
        if (F > 0 && n[p] > 0 && (uint64_t(n[p]) > max_jobs / F || F * uint64_t(n[p]) > max_jobs - uint64_t(job_row[p])))
            throw std::runtime_error("forecast_skill: the batch is too large");
        job_row[p + 1] = job_row[p] + int64_t(F * uint64_t(n[p]));
    }
    return size_t(job_row[P]);
}

void fs_fill_nan(double* x, size_t count) {
    if (x) std::fill(x, x + count, std::numeric_limits<double>::quiet_NaN());
}

call_record g_fs;
constexpr const char* FS_UPLOAD = "forecast_skill upload";

}  // namespace

extern "C" {

int shyft_hip_forecast_skill(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                             const int64_t* t_end, const int32_t* fx, size_t P, const int64_t* fc_row,
                             const int64_t* fc_ix, const int64_t* obs_ix, const int64_t* t0_offset, const int64_t* dt,
                             const int64_t* n, double* ns, double* sim, double* obs) {
    try {
        std::vector<int64_t> job_row;
        const size_t J = fs_prepare("shyft_hip_forecast_skill", S, row, t, v, t_end, fx, P, fc_row, fc_ix, obs_ix,
                                    t0_offset, dt, n, job_row);
        if (P == 0 || J == 0) {
            fs_fill_nan(ns, P);
            return 0;
        }
        device_call c(device);
        const size_t np = size_t(row[S]);
        dbuf<int64_t> d_row, d_t, d_tend, d_fc_row, d_fc_ix, d_obs_ix, d_off, d_dt, d_n, d_job_row;
        dbuf<double> d_v, d_ns, d_sim, d_obs;
        dbuf<int32_t> d_fx;
        c.upload(d_row, row, S + 1, FS_UPLOAD);
        c.upload(d_t, t, np, FS_UPLOAD);
        c.upload(d_v, v, np, FS_UPLOAD);
        c.upload(d_tend, t_end, S, FS_UPLOAD);
        c.upload(d_fx, fx, S, FS_UPLOAD);
        c.upload(d_fc_row, fc_row, P + 1, FS_UPLOAD);
        c.upload(d_fc_ix, fc_ix, size_t(fc_row[P]), FS_UPLOAD);
        c.upload(d_obs_ix, obs_ix, P, FS_UPLOAD);
        c.upload(d_off, t0_offset, P, FS_UPLOAD);
        c.upload(d_dt, dt, P, FS_UPLOAD);
        c.upload(d_n, n, P, FS_UPLOAD);
        c.upload(d_job_row, job_row.data(), P + 1, FS_UPLOAD);
        d_ns.alloc(P);
        d_sim.alloc(J);
        d_obs.alloc(J);
        fs_args a{};
        a.P = P;
        a.row = d_row.p;
        a.t = d_t.p;
        a.v = d_v.p;
        a.t_end = d_tend.p;
        a.fx = d_fx.p;
        a.fc_row = d_fc_row.p;
        a.fc_ix = d_fc_ix.p;
        a.obs_ix = d_obs_ix.p;
        a.t0_offset = d_off.p;
        a.dt = d_dt.p;
        a.n = d_n.p;
        a.job_row = d_job_row.p;
        a.ns = d_ns.p;
        a.sim = d_sim.p;
        a.obs = d_obs.p;
        c.begin();
        hipLaunchKernelGGL(forecast_skill_kernel, dim3(launch_blocks((P + FS_WAVES - 1) / FS_WAVES)), dim3(FS_BLOCK), 0, c.s, a);
        hip_check(hipGetLastError(), "forecast_skill");
        c.end();
        if (ns) c.download(ns, d_ns.p, P, "forecast_skill download");
        if (sim) c.download(sim, d_sim.p, J, "forecast_skill download");
        if (obs) c.download(obs, d_obs.p, J, "forecast_skill download");
        g_fs.record(c.dev, c.finish("forecast_skill"));
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

int shyft_hip_forecast_skill_host(int device, size_t S, const int64_t* row, const int64_t* t, const double* v,
                                  const int64_t* t_end, const int32_t* fx, size_t P, const int64_t* fc_row,
                                  const int64_t* fc_ix, const int64_t* obs_ix, const int64_t* t0_offset,
                                  const int64_t* dt, const int64_t* n, double* ns, double* sim, double* obs) {
    namespace h = shyft_hip::host;
    (void)device;
    try {
        std::vector<int64_t> job_row;
        const size_t J = fs_prepare("shyft_hip_forecast_skill_host", S, row, t, v, t_end, fx, P, fc_row, fc_ix, obs_ix,
                                    t0_offset, dt, n, job_row);
        if (P == 0 || J == 0) {
            fs_fill_nan(ns, P);
            return 0;
        }
        std::vector<h::point_ts> series;  // every series once, however many problems name it
        series.reserve(S);
        for (size_t s = 0; s < S; ++s) series.push_back(point_series(s, row, t, v, t_end, fx));
        std::vector<const h::point_ts*> tsv;
        std::vector<double> vs, vo;
        for (size_t p = 0; p < P; ++p) {
            tsv.clear();
            vs.clear();
            vo.clear();
            for (int64_t e = fc_row[p]; e < fc_row[p + 1]; ++e) tsv.push_back(&series[size_t(fc_ix[e])]);
            h::forecast_slices(tsv, obs_ix[p] >= 0 ? &series[size_t(obs_ix[p])] : nullptr, t0_offset[p], dt[p],
                               size_t(n[p]), vs, vo);
            if (ns) ns[p] = vs.empty() ? std::numeric_limits<double>::quiet_NaN() : 1.0 - h::nash_sutcliffe_goal(vo, vs);
            if (sim) std::copy(vs.begin(), vs.end(), sim + job_row[p]);
            if (obs) std::copy(vo.begin(), vo.end(), obs + job_row[p]);
        }
        return 0;
    } catch (const std::exception& e) {
        return fail(nullptr, e.what());
    }
}

double shyft_hip_forecast_skill_last_ms(int device) { return g_fs.last_ms.load(device, 0.0); }

uint64_t shyft_hip_forecast_skill_calls(int device) { return g_fs.calls.load(device, 0); }

}  // extern "C"
