"""Shared by the quantile-mapping tests: a literal pure-Python restatement of the reference's stateful loops
(core/time_series_qm.h: the `while` walks of compute_weighted_quantiles :80-100 and
compute_interp_weighted_quantiles :139-170, wvo_accessor :187-210, quantile_index :34-52 and the per-step body of
quantile_mapping :325-347), not the closed form the library evaluates, and the case generators.

Python floats are IEEE doubles and every operation below is one rounded operation in the reference's order, so the
library's host entry must reproduce these numbers exactly."""
import math

import numpy as np

NAN, INF = float("nan"), float("inf")
PRIOR, QM, QM_BLEND = 0, 1, 2


# ---- the reference, literally ----------------------------------------------------------------------------------------
def quantile_index(row):
    """:40-50 for one step: the indexes of the finite values, ascending by `<`; std::sort's open order of equal values
    fixed as the library fixes it, by ascending index (list.sort is stable, and -0.0 < 0.0 is false)."""
    pi = [i for i, v in enumerate(row) if math.isfinite(v)]
    pi.sort(key=lambda i: row[i])
    return pi


class WvoAccessor:
    """:187-210 at one step"""

    def __init__(self, ordered_ix, w, row):
        self.ix, self.w, self.row = ordered_ix, w, row
        s = 0.0
        for i in ordered_ix:
            s += w[i]
        self.w_sum = s

    def size(self):
        return len(self.ix)

    def weight(self, i):
        return self.w[self.ix[i]] / self.w_sum

    def value(self, i):
        return self.row[self.ix[i]]


def _q_step(n_q):
    return 1.0 / (n_q - 1) if n_q != 1 else INF  # 1.0 / 0 in C++


def compute_weighted_quantiles(n_q, wv):
    """:80-100"""
    q_step = _q_step(n_q)
    q = []
    j = 0
    q_j = 0.0
    w_j = wv.weight(j)
    v_j = wv.value(j)
    for i in range(n_q):
        q_i = q_step * i
        while q_j + w_j < q_i:
            q_j += w_j
            if j + 1 < wv.size():
                j += 1
                w_j = wv.weight(j)
                v_j = wv.value(j)
        q.append(v_j)
    return q


def compute_interp_weighted_quantiles(n_q, wv):
    """:139-170. With one quantile q_i is NaN, the reference never enters its loop and reads value(size_t(-1)); the
    library defines value(0) there."""
    if n_q == 1:
        return [wv.value(0)]
    q_step = _q_step(n_q)
    q = []
    j = -1
    q_j = 0.0
    w_j = 0.0
    width = 0.0
    for i in range(n_q):
        q_i = q_step * i
        while q_j <= q_i and j + 1 != wv.size():
            width = 0.5 * w_j
            j += 1
            w_j = wv.weight(j)
            width += 0.5 * w_j
            q_j += width
        if j == 0 or (j + 1 == wv.size() and q_i >= q_j):
            v_j = wv.value(j)
        else:
            interp_start = wv.value(j - 1)
            interp_end = wv.value(j)
            inclination = (interp_end - interp_start) / width
            offset = q_j - width
            v_j = interp_start + inclination * (q_i - offset)
        q.append(v_j)
    return q


def quantile_mapping_step(fc_row, w, pri_row, mode, interp_weight, interpolated):
    """:325-347 for one step; `mode` is what :328 and :335-336 decide from the times"""
    fc_row, pri_row, w = [float(x) for x in fc_row], [float(x) for x in pri_row], [float(x) for x in w]
    fc_ix = quantile_index(fc_row)
    if mode == PRIOR or not fc_ix:
        return list(pri_row)
    pri_ix = quantile_index(pri_row)
    out = [NAN] * len(pri_row)
    if not pri_ix:
        return out
    wvo = WvoAccessor(fc_ix, w, fc_row)
    fn = compute_interp_weighted_quantiles if interpolated else compute_weighted_quantiles
    quantile_vals = fn(len(pri_ix), wvo)
    for i, k in enumerate(pri_ix):
        if mode == QM_BLEND:
            out[k] = (1.0 - interp_weight) * quantile_vals[i] + interp_weight * pri_row[k]
        else:
            out[k] = quantile_vals[i]
    return out


def quantile_mapping(fc, w, pri, mode, interp_weight, interpolated):
    """every (problem, step) of fc [B][T][F], pri [B][T][P]"""
    out = np.empty(pri.shape)
    for b in range(pri.shape[0]):
        for t in range(pri.shape[1]):
            out[b, t] = quantile_mapping_step(fc[b, t], w, pri[b, t], int(mode[t]), float(interp_weight[t]), interpolated)
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------
def _values(rng, shape):
    """continuous values, about a third drawn from five multiples of 1.5 (value ties, 0.0 among them), some -0.0,
    about 20 % NaN and a few +-inf"""
    v = rng.normal(0.0, 10.0, shape)
    ties = rng.random(shape) < 0.35
    v[ties] = (rng.integers(-2, 3, shape) * 1.5)[ties]
    v[rng.random(shape) < 0.05] = -0.0
    v[rng.random(shape) < 0.2] = NAN
    r = rng.random(shape)
    v[r < 0.02] = INF
    v[(r >= 0.02) & (r < 0.04)] = -INF
    return v


def make_case(B, T, F, P, seed):
    """fc [B][T][F], w [F], pri [B][T][P], mode [T], interp_weight [T]. Modes cycle QM, QM_BLEND, PRIOR along T. Where T
    allows: step 0 (QM) has no finite forecast, step 1 (QM_BLEND) one finite scenario, step 3 (QM) none, step 4
    (QM_BLEND) a forecast tie with unequal weights, step 6 (QM) +0.0 and -0.0 in both sets, step 7 (QM_BLEND) an
    infinity and a NaN in both sets; with P > 2 one scenario is NaN at every step."""
    rng = np.random.default_rng(seed)
    fc, pri = _values(rng, (B, T, F)), _values(rng, (B, T, P))
    w = rng.integers(1, 8, F) + rng.integers(0, 4, F) * 0.25
    if F >= 2:
        w[0], w[F - 1] = 5.0, 2.0
    mode = np.array([(QM, QM_BLEND, PRIOR)[t % 3] for t in range(T)], dtype=np.int32)
    iw = np.where(mode == QM_BLEND, rng.random(T), 0.0)
    if P > 2:
        pri[:, :, P - 2] = NAN
    if T >= 2:
        fc[:, 0, :] = NAN
        pri[:, 1, :] = NAN
        pri[:, 1, P - 1] = 3.25
        fc[:, 1, 0] = 1.5
    if T >= 5:
        pri[:, 3, :] = NAN
        fc[:, 3, 0] = -4.0
        fc[:, 4, 0] = fc[:, 4, F - 1] = 2.5
    if T >= 7:
        fc[:, 6, 0], fc[:, 6, F - 1] = 0.0, -0.0
        pri[:, 6, 0], pri[:, 6, P - 1] = -0.0, 0.0
    if T >= 8 and F >= 3:
        fc[:, 7, 1], fc[:, 7, 2] = INF, NAN
    if T >= 8 and P >= 3:
        pri[:, 7, 0], pri[:, 7, 1] = NAN, -INF
    return fc, w.astype(np.float64), pri, mode, iw


def branches(fc, pri, mode):
    """which branches of the per-step body the case reaches, over all (problem, step)"""
    nf = np.isfinite(fc).sum(axis=2)
    npri = np.isfinite(pri).sum(axis=2)
    got = set()
    for t, m in enumerate(mode):
        for b in range(fc.shape[0]):
            if m == PRIOR:
                got.add("prior")
            elif nf[b, t] == 0:
                got.add("no_forecast")
            elif npri[b, t] == 0:
                got.add("no_scenario")
            else:
                got.add("qm" if m == QM else "qm_blend")
                if npri[b, t] == 1:
                    got.add("one_scenario")
    return got


def qm_main_inputs(api, rng):
    """the arrangement of qm_test.cpp:385-435 (qm_main): three weighted forecast sets on a 4-step daily axis, 56
    scenarios of uniform random values on the 6-step axis"""
    fx = api.POINT_AVERAGE_VALUE
    t0 = api.Calendar().time(2017, 1, 1)
    ta = api.TimeAxis(t0, api.deltahours(24), 4)
    tah = api.TimeAxis(t0, api.deltahours(24), 6)
    sets = api.TsVectorSet()
    for values in ([[13.4, 15.6, 17.1, 19.1], [34.1, 2.4, 43.9, 10.2]],
                   [[83.1, -42.2, 0.4, 23.4], [15.1, 6.5, 4.2, 2.9], [53.1, 87.9, 23.8, 5.6]],
                   [[1.5, -1.9, -17.2, -10.0], [4.7, 18.2, 15.3, 8.9], [-45.2, -2.3, 80.2, 71.0],
                    [45.1, -92.0, 34.4, 65.8]]):
        tsv = api.TsVector()
        for v in values:
            tsv.append(api.TimeSeries(ta, api.DoubleVector(v), fx))
        sets.append(tsv)
    weights = api.DoubleVector([5.0, 9.0, 3.0])
    hist = rng.random((56, 6)) * 50.0
    historical = api.TsVector()
    for row in hist:
        historical.append(api.TimeSeries(tah, api.DoubleVector.from_numpy(row), fx))
    return sets, weights, historical, tah, hist


# the rank breaks of qm_test.cpp:448-488: per step, (first rank past the value, value)
QM_MAIN_BREAKS = (
    ((4, -45.2), (7, 1.5), (11, 4.7), (16, 13.4), (26, 15.1), (32, 34.1), (35, 45.1), (45, 53.1), (56, 83.1)),
    ((4, -92.0), (14, -42.2), (17, -2.3), (21, -1.9), (26, 2.4), (36, 6.5), (42, 15.6), (45, 18.2), (56, 87.9)),
    ((4, -17.2), (14, 0.4), (24, 4.2), (27, 15.3), (33, 17.1), (43, 23.8), (47, 34.4), (52, 43.9), (56, 80.2)),
    ((4, -10.0), (14, 2.9), (24, 5.6), (27, 8.9), (33, 10.2), (39, 19.1), (49, 23.4), (52, 65.8), (56, 71.0)),
)


def check_qm_main(result, hist):
    """the assertions of qm_test.cpp:448-504 on a result of quantile_map_forecast(..., tah, time(4), time(4), False)"""
    for t, breaks in enumerate(QM_MAIN_BREAKS):
        order = np.argsort(hist[:, t], kind="stable")
        for i, k in enumerate(order):
            want = next(v for end, v in breaks if i < end)
            assert result[int(k)].value(t) == want, (t, i)
    check_historical_tail(result, hist)


def check_historical_tail(result, hist):
    """qm_test.cpp:490-503 with its bound: the tail is the scenarios' true average (v * dt) / dt, not a copy"""
    for t in range(4, 6):
        for i in range(hist.shape[0]):
            assert not abs(result[i].value(t) - hist[i, t]) > 0.0001, (t, i)
