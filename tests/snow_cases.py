"""Shared by the snow-step tests (test_snow_steps_host.py, test_snow_steps_gpu.py): single-step jobs for the three
stacks that keep their snow pack in quantile bins (hbv_stack, pt_hs_k: hbv_snow; pt_hps_k: hbv_physical_snow), the
branch labels each job takes, and a second reference.

The second reference is a plain Python restatement of one hbv_snow step (core/hbv_snow.h:139-272 with
distribute_snow and integrate of core/hbv_snow_common.h:14-66) and of one hbv_physical_snow step
(core/hbv_physical_snow.h:227-553), in the manner of tests/qm_cases.py: Python floats are IEEE doubles and every
operation below is one rounded double operation in the reference's order. hbv_snow uses no elementary function, so its
restatement equals the oracle bit for bit; hbv_physical_snow takes exp, log, pow, pow4 and pow8 from the oracle's
entries. Both return the set of branch labels the job took.

A job is a flat state row, one step of forcing and the parameter set it belongs to: one cell of a region with T = 1.
Start states come from seeded random walks on the oracle's single-step entries (states a run reaches) and from
hand-made rows that put a value on, and one double to either side of, each comparison that decides a branch."""
import functools
import math

import numpy as np

from tests import edge_sets, oracle_lib

NAN, INF = float("nan"), float("inf")
HOUR = 3600_000_000
DTS = {"1h": HOUR, "3h": 3 * HOUR, "24h": 24 * HOUR}
MB = oracle_lib.HBV_MAX_BINS
STACKS = ("hbv_stack", "pt_hs_k", "pt_hps_k")
QUOTA = 12        # clean jobs kept per label (the coverage rule asks for 8)
N_WALKS = 900     # random walks per (snow routine, dt)
HPS_TOL = 1.0e-10

# ---- labels ----------------------------------------------------------------------------------------------------------
DISTRIBUTE_LABELS = ("dist_skip", "dist_reset", "dist_corr", "dist_nocorr")
INTEGRATE_LABELS = ("swe_zero", "int_full", "int_end_first", "int_end_middle", "int_end_last")
BIN_LABELS = ("rf_empty", "rf_partial", "rf_partial_cap", "rf_all", "us_melt", "us_min_cap", "us_gone", "us_empty")
BALANCE_LABELS = ("balance_ok", "clamp")
HS_LABELS = DISTRIBUTE_LABELS + (
    "snow", "rain", "reset", "rescale_skip", "rescale_idx0", "rescale_idxk", "scan_top", "scan_past_zero", "scan_none",
    "refreeze", "melt", "potmelt_zero", "melt_idx0", "melt_idx_nb", "melt_front_pos", "melt_front_zero",
) + BIN_LABELS + INTEGRATE_LABELS + BALANCE_LABELS
HPS_LABELS = DISTRIBUTE_LABELS + (
    "snow", "rain", "reset", "rescale_skip", "rescale_idx0", "rescale_idxk", "scan_top", "scan_past_zero", "scan_none",
    "sca_gt_1", "alb_slow", "alb_fast", "alb_at_max", "alb_at_min", "alb_inside", "rain_heat", "snow_heat", "iso",
    "vp_cold", "sst_zero", "sst_neg", "delta_sh_pos", "delta_sh_nonpos", "no_melt", "melt_idx0", "melt_idx_nb",
    "melt_front_pos", "melt_front_zero", "mixed_melt_refreeze",
) + BIN_LABELS + INTEGRATE_LABELS + BALANCE_LABELS
# the rest of an hbv_stack step (hbv_actual_evapotranspiration, hbv_soil, hbv_tank)
HBV_TAIL_LABELS = ("sm_lt_lp", "sm_ge_lp", "beta2", "beta_pow", "soil_clamp", "soil_noclamp", "sm_clamped0", "sm_pos",
                   "q12_zero", "q12_pos", "tank_below_uz1", "tank_above_uz1")
RAISE = "raise"


# ---- parameter sets --------------------------------------------------------------------------------------------------
def _dist(s, intervals):
    return [float(v) for v in oracle_lib.hbv_normalize(s, intervals)], [float(v) for v in intervals]


_DISTS = (
    ("flat5", [1.0] * 5, [0.0, 0.25, 0.5, 0.75, 1.0]),
    ("skew5", [1.5, 1.3, 1.0, 0.8, 0.5], [0.0, 0.2, 0.5, 0.8, 1.0]),      # uneven intervals
    ("zero5", [1.5, 1.0, 1.2, 0.0, 0.6], [0.0, 0.25, 0.5, 0.75, 1.0]),    # an interior factor of exactly 0
    ("three", [1.4, 1.0, 0.7], [0.0, 0.4, 1.0]),
    ("two", [1.2, 0.8], [0.0, 1.0]),
    ("eight", [1.6, 1.4, 1.1, 1.0, 0.9, 0.7, 0.8, 1.5], [0.0, 0.1, 0.25, 0.4, 0.5, 0.65, 0.8, 1.0]),
)
# hbv_snow: tx cx ts lw cfr
_HS_PAR = ((0.0, 1.0, 0.0, 0.1, 0.5), (0.5, 2.5, -0.25, 0.07, 0.3), (-0.5, 4.0, 0.25, 0.2, 0.8),
           (1.0, 1.5, 0.5, 0.05, 0.1), (0.25, 3.0, 0.0, 0.15, 0.6), (-1.0, 2.0, -0.5, 0.12, 0.4))
# hbv_stack: fc beta lp uz1 (one set with beta != 2, a small fc for the soil clamp, a small lp for sm clamped at 0)
_HBV_PAR = ((300.0, 2.0, 150.0, 25.0), (250.0, 1.7, 120.0, 30.0), (1.5, 2.0, 150.0, 25.0), (300.0, 2.0, 0.02, 10.0),
            (40.0, 2.5, 60.0, 25.0), (300.0, 2.0, 150.0, 5.0))
# hbv_physical_snow: tx lw cfr wind_scale wind_const surface_magnitude max_albedo min_albedo fast slow reset_depth iso
_HPS_PAR = ((0.0, 0.1, 0.5, 2.0, 1.0, 30.0, 0.9, 0.6, 5.0, 5.0, 5.0, 0.0),
            (0.5, 0.07, 0.3, 1.0, 0.5, 20.0, 0.85, 0.55, 3.0, 7.0, 4.0, 1.0),
            (-0.5, 0.2, 0.8, 3.0, 1.0, 30.0, 0.9, 0.6, 5.0, 5.0, 0.05, 0.0),   # albedo reaches max_albedo in one fall
            (1.0, 0.05, 0.1, 2.0, 2.0, 40.0, 0.8, 0.5, 2.0, 4.0, 5.0, 1.0),
            (0.25, 0.15, 0.6, 0.5, 1.0, 10.0, 0.9, 0.6, 5.0, 5.0, 2.0, 0.0),
            (-1.0, 0.12, 0.4, 2.0, 1.0, 30.0, 0.95, 0.4, 1.0, 2.0, 5.0, 1.0))


@functools.lru_cache(maxsize=None)
def hs_sets():
    """the hbv_snow parameter sets: dicts name, s, I (normalised), tx, cx, ts, lw, cfr"""
    out = []
    for (name, s, iv), (tx, cx, ts, lw, cfr) in zip(_DISTS, _HS_PAR):
        sn, ivn = _dist(s, iv)
        out.append(dict(name=name, s=sn, I=ivn, tx=tx, cx=cx, ts=ts, lw=lw, cfr=cfr))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hps_sets():
    keys = ("tx", "lw", "cfr", "wind_scale", "wind_const", "surface_magnitude", "max_albedo", "min_albedo", "fast",
            "slow", "reset_depth", "iso")
    out = []
    for (name, s, iv), row in zip(_DISTS, _HPS_PAR):
        sn, ivn = _dist(s, iv)
        d = dict(zip(keys, row))
        d.update(name=name, s=sn, I=ivn, p12=list(row))
        out.append(d)
    return tuple(out)


def set_names():
    return [d[0] for d in _DISTS]


def dist_rows():
    """[n_sets][17] n_bins, s[8], intervals[8] of the normalised distributions"""
    return np.stack([oracle_lib.hbv_dist_row(p["s"], p["I"]) for p in hs_sets()])


def stack_params(stack):
    """the parameter rows [n_sets][reference width] of a stack, in set order (without the distribution)"""
    from shyft_amd import synthetic
    rows = []
    for k in range(len(_DISTS)):
        if stack == "hbv_stack":
            p = synthetic.default_hbv_parameters()
            p[[0, 1, 2, 3]] = _HBV_PAR[k]
            tx, cx, ts, lw, cfr = _HS_PAR[k]
            p[8:13] = [lw, tx, cx, ts, cfr]
            p[20] = (0.0, 0.4)[k % 2]                 # gm.direct_response
        elif stack == "pt_hs_k":
            p = synthetic.default_pthsk_parameters()
            tx, cx, ts, lw, cfr = _HS_PAR[k]
            p[4:9] = [lw, tx, cx, ts, cfr]
            p[16] = (0.0, 0.4)[k % 2]
        else:
            p = synthetic.default_pthpsk_parameters()
            tx, lw, cfr = _HPS_PAR[k][:3]
            p[4:7] = [lw, tx, cfr]                    # the row's order (pt_hps_k.h:64-90)
            p[7:16] = _HPS_PAR[k][3:]
        rows.append(p)
    return np.stack(rows)


HPS_GM_DIRECT = (0.0, 0.4, 0.0, 0.4, 0.0, 0.4)


# ---- the reference, literally ----------------------------------------------------------------------------------------
def _div(a, b):
    """a / b as IEEE does it (Python raises on a zero divisor)"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def integrate0(f, x, n, b, f_b_is_zero):
    """hbv_snow_common::integrate (:14-44) from a = 0; returns (area, index of the interval the walk ended inside or
    None when it ran to the last knot)"""
    a = 0.0
    left = 0
    area = 0.0
    x_l = a
    while a > x[left]:
        left += 1
    if abs(a - x[left]) > 1.0e-8 and left > 0:
        left -= 1
        f_l = _div(f[left + 1] - f[left], x[left + 1] - x[left]) * (a - x[left]) + f[left]
    else:
        f_l = f[left]
    ended = None
    while left < n - 1:
        if b >= x[left + 1]:
            area += 0.5 * (f_l + f[left + 1]) * (x[left + 1] - x_l)
            x_l = x[left + 1]
            f_l = f[left + 1]
            left += 1
        else:
            if not f_b_is_zero:
                area += (f_l + _div(0.5 * (f[left + 1] - f_l), x[left + 1] - x_l) * (b - x_l)) * (b - x_l)
            else:
                area += 0.5 * f_l * (b - x_l)
            ended = left
            break
    return area, ended


def _integrate_label(ended, n, L):
    if ended is None:
        L.add("int_full")
    elif ended == 0:
        L.add("int_end_first")
    elif ended == n - 2:
        L.add("int_end_last")
    else:
        L.add("int_end_middle")


def distribute(s, iv, lw, st, L):
    """state::distribute(p, false) (hbv_snow.h:95-99) -> distribute_snow (hbv_snow_common.h:47-66) on
    st = dict(swe, sca, sp, sw): only when the state's bin count differs from the set's"""
    n = len(iv)
    if len(st["sp"]) == n:
        L.add("dist_skip")
        return
    st["sp"] = [0.0] * n
    st["sw"] = [0.0] * n
    swe, sca = st["swe"], st["sca"]
    if swe <= 1.0e-3 or sca <= 1.0e-3:
        st["swe"] = st["sca"] = 0.0
        L.add("dist_reset")
        return
    sp = st["sp"]
    for i in range(n):
        sp[i] = 0.0 if sca < iv[i] else s[i] * swe
    temp_swe, _ = integrate0(sp, iv, n, sca, True)
    if temp_swe < swe:
        corr1 = _div(swe, temp_swe) * lw
        corr2 = _div(swe, temp_swe) * (1.0 - lw)
        for i in range(n):
            st["sw"][i] = corr1 * sp[i]
            sp[i] *= corr2
        L.add("dist_corr")
    else:
        L.add("dist_nocorr")


def _refreeze(sp, sw, i, rain, potmelt, lw, L):
    if sp[i] > 0.0:
        if sw[i] + rain > -potmelt:
            sp[i] -= potmelt
            sw[i] += potmelt + rain
            if sw[i] > sp[i] * lw:
                sw[i] = sp[i] * lw
                L.add("rf_partial_cap")
            L.add("rf_partial")
        else:
            sp[i] += sw[i] + rain
            sw[i] = 0.0
            L.add("rf_all")
    else:
        L.add("rf_empty")


def _update_state(sp, sw, i, rain, potmelt, lw, L):
    if sp[i] > potmelt:
        sw[i] += potmelt + rain
        sp[i] -= potmelt
        cap = sp[i] * lw
        if cap < sw[i]:          # std::min(sw, sp * lw)
            sw[i] = cap
            L.add("us_min_cap")
        L.add("us_melt")
    elif sp[i] > 0.0:
        sp[i] = sw[i] = 0.0
        L.add("us_gone")
    else:
        L.add("us_empty")


def _sca_index(iv, sca):
    for i in range(len(iv) - 1):
        if sca >= iv[i] and sca < iv[i + 1]:
            return i
    return len(iv) - 1


def _rescale(iv, sp, sw, sca, L):
    """the bin rescale before snowfall (hbv_snow.h:226-236, hbv_physical_snow.h:393-405)"""
    idx = _sca_index(iv, sca)
    if sca > 1.0e-5 and sca < 1.0 - 1.0e-5:
        if idx == 0:
            sp[0] *= _div(sca, iv[1] - iv[0])
            sw[0] *= _div(sca, iv[1] - iv[0])
            L.add("rescale_idx0")
        else:
            f = _div(1.0 + _div(sca - iv[idx], iv[idx] - iv[idx - 1]),
                     1.0 + _div(iv[idx + 1] - iv[idx], iv[idx] - iv[idx - 1]))
            sp[idx] *= f
            sw[idx] *= f
            L.add("rescale_idxk")
    else:
        L.add("rescale_skip")


class NegativeOutflow(RuntimeError):
    pass


def hs_step(p, st, dt_us, prec_mm_h, temp):
    """distribute(p, false) and one hbv_snow::calculator::step on st = dict(swe, sca, sp, sw) (updated in place).
    Returns (outflow mm/h, labels); raises NegativeOutflow (with .labels) where the reference throws."""
    L = set()
    s, iv = p["s"], p["I"]
    n = len(iv)
    distribute(s, iv, p["lw"], st, L)
    sp, sw = st["sp"], st["sw"]
    swe = st["swe"]
    sca = st["sca"]
    step_in_days = (dt_us / 1e6) / 86400.0
    dt_hours = (dt_us / 1e6) / 3600.0
    prec = prec_mm_h * dt_hours
    total_water = prec + swe
    if temp < p["tx"]:
        snow, rain = prec, 0.0
        L.add("snow")
    else:
        snow, rain = 0.0, prec
        L.add("rain")
    swe += snow + sca * rain
    if swe < 0.1:
        for i in range(n):
            sp[i] = sw[i] = 0.0
        st["swe"] = 0.0
        st["sca"] = 0.0
        L.add("reset")
        return total_water / dt_hours, L
    if snow > 0.0:
        _rescale(iv, sp, sw, sca, L)
        for i in range(n):
            sp[i] += snow * s[i]
        sca = iv[1]
        label = "scan_none"
        for i in range(n - 2, 0, -1):
            if s[i] > 0.0:
                sca = iv[i + 1]
                label = "scan_top" if i == n - 2 else "scan_past_zero"
                break
        L.add(label)
    potmelt = p["cx"] * step_in_days * (temp - p["ts"])
    lw = p["lw"]
    if potmelt < 0.0:
        potmelt *= p["cfr"]
        L.add("refreeze")
        for i in range(n):
            _refreeze(sp, sw, i, rain, potmelt, lw, L)
    else:
        L.add("melt")
        if potmelt == 0.0:
            L.add("potmelt_zero")
        idx = n
        for i in range(n):
            if sp[i] < potmelt:
                idx = i
                break
        if idx == 0:
            sca = 0.0
            L.add("melt_idx0")
        elif idx == n:
            sca = 1.0
            L.add("melt_idx_nb")
        elif sp[idx] > 0.0:
            sca = iv[idx] - _div((iv[idx] - iv[idx - 1]) * (potmelt - sp[idx]), sp[idx - 1] - sp[idx])
            L.add("melt_front_pos")
        else:
            sca = (1.0 - _div(potmelt, sp[idx - 1])) * (sca - iv[idx - 1]) + iv[idx - 1]
            L.add("melt_front_zero")
        for i in range(n):
            _update_state(sp, sw, i, rain, potmelt, lw, L)
    if sca < 1.0e-6:
        swe = 0.0
        L.add("swe_zero")
    else:
        f_is_zero = not sca >= 1.0
        swe, ended = integrate0(sp, iv, n, sca, f_is_zero)
        swe += integrate0(sw, iv, n, sca, f_is_zero)[0]
        _integrate_label(ended, n, L)
    if total_water < swe:
        if total_water - swe < -1.0e-6:
            e = NegativeOutflow("Negative outflow")
            e.labels = L | {RAISE}
            raise e
        swe = total_water
        L.add("clamp")
    else:
        L.add("balance_ok")
    st["swe"] = swe
    st["sca"] = sca
    return (total_water - swe) / dt_hours, L


def _math():
    L = oracle_lib.load("detmath")
    return L.oracle_exp, L.oracle_log, L.oracle_pow, L.oracle_pow4, L.oracle_pow8


def hps_step(p, st, dt_us, T, rad, prec_mm_h, wind_speed, rel_hum):
    """distribute(p, false) and one hbv_physical_snow::calculator::step on st = dict(swe, sca, surface_heat, sp, sw,
    albedo, iso) (updated in place). Returns ((outflow, sca, storage), labels); raises NegativeOutflow."""
    oexp, olog, opow, opow4, opow8 = _math()
    L = set()
    s, iv = p["s"], p["I"]
    n = len(iv)
    distribute(s, iv, p["lw"], st, L)
    if len(st["sp"]) != len(st["albedo"]):
        st["albedo"] = [0.4] * n
        st["iso"] = [0.0] * n
    sp, sw = st["sp"], st["sw"]
    melt_heat, water_heat, ice_heat, sigma = 333660.0, 4180.0, 2050.0, 5.670373e-8
    BB0 = 0.98 * sigma * opow(273.15, 4.0)
    dts = float(dt_us) / 1e6
    prec = prec_mm_h * float(dt_us) / 3600000000.0
    total_water = prec + st["swe"]
    if T < p["tx"]:
        snow, rain = prec, 0.0
        L.add("snow")
    else:
        snow, rain = 0.0, prec
        L.add("rain")
    st["swe"] += snow + st["sca"] * rain
    if st["swe"] < HPS_TOL:
        for i in range(n):
            sp[i] = sw[i] = 0.0
            st["albedo"][i] = p["max_albedo"]
            st["iso"][i] = 0.0
        st["swe"] = 0.0
        st["sca"] = 0.0
        st["surface_heat"] = 0.0
        L.add("reset")
        return (total_water, 0.0, 0.0), L
    albedo = list(st["albedo"])
    surface_heat = st["surface_heat"]
    min_albedo, max_albedo = p["min_albedo"], p["max_albedo"]
    albedo_range = max_albedo - min_albedo
    dt_in_days = dts / 86400.0
    slow_decay = (0.5 * albedo_range * dt_in_days / p["slow"])
    fast_decay = opow(2.0, -dt_in_days / p["fast"])
    T_k = T + 273.15
    turb = p["wind_scale"] * wind_speed + p["wind_const"]
    vapour_pressure = (33.864 * (opow8(7.38e-3 * T + 0.8072) - 1.9e-5 * abs(1.8 * T + 48.0) + 1.316e-3) * rel_hum)
    if T < 0.0:
        vapour_pressure *= 1.0 + 9.72e-3 * T + 4.2e-5 * T * T
        L.add("vp_cold")
    if snow > HPS_TOL:
        _rescale(iv, sp, sw, st["sca"], L)
        for i in range(n):
            currsnow = snow * s[i]
            sp[i] += currsnow
            albedo[i] += (currsnow * albedo_range / p["reset_depth"])
        label = "scan_none"
        for i in range(n - 2, 0, -1):
            if s[i] > 0.0:
                st["sca"] = s[i + 1]          # the reference reads the factors, not the quantiles
                label = "scan_top" if i == n - 2 else "scan_past_zero"
                break
            st["sca"] = s[1]
        L.add(label)
        if st["sca"] > 1.0:
            L.add("sca_gt_1")
    else:
        if T < 0.0:
            for i in range(n):
                albedo[i] -= slow_decay
            L.add("alb_slow")
        else:
            for i in range(n):
                albedo[i] = (min_albedo + fast_decay * (albedo[i] - min_albedo))
            L.add("alb_fast")
    for i in range(n):
        a = albedo[i]
        if max_albedo < a:       # std::min(alb, max_albedo)
            a = max_albedo
            L.add("alb_at_max")
        if a < min_albedo:       # std::max(., min_albedo)
            a = min_albedo
            L.add("alb_at_min")
        if a == albedo[i]:
            L.add("alb_inside")
        albedo[i] = a
    effect = [rad * (1.0 - a) for a in albedo]
    lw_in = (0.98 * sigma * oexp(6.87e-2 * olog(vapour_pressure / T_k)) * opow4(T_k))
    for i in range(n):
        effect[i] += lw_in
    if T > 0.0 and snow < HPS_TOL:
        for i in range(n):
            effect[i] += rain * T * water_heat / dts
        L.add("rain_heat")
    if T <= 0.0 and rain < HPS_TOL:
        for i in range(n):
            effect[i] += snow * s[i] * T * ice_heat / dts
        L.add("snow_heat")
    if p["iso"] != 0.0:
        for i in range(n):
            iso_effect = (effect[i] - BB0 + turb * (T + 1.7 * (vapour_pressure - 6.12)))
            st["iso"][i] += (iso_effect * dts / melt_heat)
        L.add("iso")
    sst = min(0.0, 1.16 * T - 2.09)
    if sst > -HPS_TOL:
        term = turb * (T + 1.7 * (vapour_pressure - 6.12)) - BB0
        L.add("sst_zero")
    else:
        term = (turb * (T - sst + 1.7 * (vapour_pressure - 6.132 * oexp(0.103 * T - 0.186))) -
                0.98 * sigma * opow4(sst + 273.15))
        L.add("sst_neg")
    for i in range(n):
        effect[i] += term
    delta_sh = -surface_heat
    surface_heat = p["surface_magnitude"] * ice_heat * sst * 0.5
    delta_sh += surface_heat
    energy = [e * dts for e in effect]
    if delta_sh > 0.0:
        for i in range(n):
            energy[i] -= delta_sh
        L.add("delta_sh_pos")
    else:
        L.add("delta_sh_nonpos")
    pm = [e / melt_heat for e in energy]
    lw = p["lw"]
    idx = n
    any_melt = False
    for i in range(n):
        if pm[i] >= HPS_TOL:
            any_melt = True
            if sp[i] < pm[i]:
                idx = i
                break
    if any_melt:
        if idx == 0:
            st["sca"] = 0.0
            L.add("melt_idx0")
        elif idx == n:
            st["sca"] = 1.0
            L.add("melt_idx_nb")
        elif sp[idx] > 0.0:
            sp[idx - 1] = sp[idx]             # the reference's assignment inside the denominator (:511-513)
            st["sca"] = (iv[idx] - (iv[idx] - iv[idx - 1]) * (pm[idx] - sp[idx]) / sp[idx - 1])
            L.add("melt_front_pos")
        else:
            st["sca"] = (1.0 - _div(pm[idx], sp[idx - 1])) * (st["sca"] - iv[idx - 1]) + iv[idx - 1]
            L.add("melt_front_zero")
    else:
        L.add("no_melt")
    n_rf = 0
    for i in range(n):
        if pm[i] < HPS_TOL:
            _refreeze(sp, sw, i, rain, p["cfr"] * pm[i], lw, L)
            n_rf += 1
        else:
            _update_state(sp, sw, i, rain, pm[i], lw, L)
    if 0 < n_rf < n:
        L.add("mixed_melt_refreeze")
    if st["sca"] < HPS_TOL:
        st["swe"] = 0.0
        L.add("swe_zero")
    else:
        f_is_zero = not st["sca"] >= 1.0
        st["swe"], ended = integrate0(sp, iv, n, st["sca"], f_is_zero)
        st["swe"] += integrate0(sw, iv, n, st["sca"], f_is_zero)[0]
        _integrate_label(ended, n, L)
    if total_water < st["swe"]:
        if total_water - st["swe"] < -HPS_TOL:
            e = NegativeOutflow("Negative outflow")
            e.labels = L | {RAISE}
            raise e
        st["swe"] = total_water
        L.add("clamp")
    else:
        L.add("balance_ok")
    return (total_water - st["swe"], st["sca"], st["swe"]), L


# ---- snow rows <-> the restatements' states --------------------------------------------------------------------------
# hbv_snow row (19): swe sca n_bins sp[8] sw[8]; hbv_physical_snow row (36): swe sca surface_heat n_bins sp sw albedo iso
HS_ROW, HPS_ROW = 3 + 2 * MB, 4 + 4 * MB


def hs_unpack(row):
    nb = int(row[2])
    return dict(swe=float(row[0]), sca=float(row[1]), sp=[float(v) for v in row[3:3 + nb]],
                sw=[float(v) for v in row[3 + MB:3 + MB + nb]])


def hs_pack(st):
    row = np.zeros(HS_ROW)
    nb = len(st["sp"])
    row[0], row[1], row[2] = st["swe"], st["sca"], nb
    row[3:3 + nb] = st["sp"]
    row[3 + MB:3 + MB + nb] = st["sw"]
    return row


def hps_unpack(row):
    nb = int(row[3])
    g = lambda k: [float(v) for v in row[4 + k * MB:4 + k * MB + nb]]  # noqa: E731
    return dict(swe=float(row[0]), sca=float(row[1]), surface_heat=float(row[2]), sp=g(0), sw=g(1), albedo=g(2), iso=g(3))


def hps_pack(st):
    row = np.zeros(HPS_ROW)
    nb = len(st["sp"])
    row[0], row[1], row[2], row[3] = st["swe"], st["sca"], st["surface_heat"], nb
    for k, key in enumerate(("sp", "sw", "albedo", "iso")):
        row[4 + k * MB:4 + k * MB + nb] = st[key]
    return row


def oracle_hs_step(k, row, dt_us, prec, temp):
    """the oracle's single-step entry on a snow row: (new row, outflow); raises RuntimeError where it throws"""
    p = hs_sets()[k]
    flat = np.zeros(oracle_lib.HBV_FLAT)
    flat[0:2] = row[0:2]
    flat[5:] = row[2:]
    st, out = oracle_lib.hbv_snow_step(flat, prec, temp, 0, dt_us, s=p["s"], intervals=p["I"], tx=p["tx"], cx=p["cx"],
                                       ts=p["ts"], lw=p["lw"], cfr=p["cfr"], distribute=2)
    new = np.zeros(HS_ROW)
    new[0:2] = st[0:2]
    new[2:] = st[5:]
    return new, out


def oracle_hps_step(k, row, dt_us, T, rad, prec, wind, rh):
    p = hps_sets()[k]
    st = np.array(row, dtype=np.float64)
    r = oracle_lib.hps_step(st, p["p12"], oracle_lib.hbv_dist_row(p["s"], p["I"]), 2, dt_us, T, rad, prec, wind, rh)
    return st, r


def python_hs_step(k, row, dt_us, prec, temp):
    """(new row, outflow, labels) by the restatement; a raise comes back as (None, None, labels with 'raise')"""
    st = hs_unpack(row)
    try:
        out, L = hs_step(hs_sets()[k], st, dt_us, prec, temp)
    except NegativeOutflow as e:
        return None, None, frozenset(e.labels)
    return hs_pack(st), out, frozenset(L)


def python_hps_step(k, row, dt_us, T, rad, prec, wind, rh):
    st = hps_unpack(row)
    try:
        r, L = hps_step(hps_sets()[k], st, dt_us, T, rad, prec, wind, rh)
    except NegativeOutflow as e:
        return None, None, frozenset(e.labels)
    return hps_pack(st), r, frozenset(L)


# ---- jobs ------------------------------------------------------------------------------------------------------------
# a snow job: (set, row, forcing) with forcing = (temp, prec, wind_speed, rel_hum, radiation) in the region's order
def _run_python(kind, k, row, dt_us, f):
    f = [float(v) for v in f]
    if kind == "hs":
        return python_hs_step(k, row, dt_us, f[1], f[0])
    return python_hps_step(k, row, dt_us, f[0], f[4], f[1], f[2], f[3])


def _run_oracle(kind, k, row, dt_us, f):
    if kind == "hs":
        return oracle_hs_step(k, row, dt_us, f[1], f[0])
    return oracle_hps_step(k, row, dt_us, f[0], f[4], f[1], f[2], f[3])


def _random_forcing(rng, kind, p, dt_us):
    h = dt_us / HOUR
    u = rng.random()
    temp = p["tx"] + (rng.normal(0.0, 1.0) if u < 0.3 else rng.normal(0.0, 8.0))
    if kind == "hs" and rng.random() < 0.3:   # melt large enough to take some bins and leave others
        temp = p["ts"] + rng.uniform(0.0, 30.0) * (24.0 / h) ** rng.uniform(0.0, 1.0)
    prec = 0.0 if rng.random() < 0.4 else float(np.exp(rng.uniform(np.log(0.01), np.log(20.0)))) / h ** rng.uniform(0, 1)
    wind = 0.0 if rng.random() < 0.1 else rng.uniform(0.0, 10.0)
    rh = rng.uniform(0.3, 1.0)
    rad = 0.0 if rng.random() < 0.2 else rng.uniform(0.0, 800.0)
    return (float(temp), float(prec), float(wind), float(rh), float(rad))


def _walk_pool(kind, dt_name):
    """every step of N_WALKS seeded random walks of 1 to 6 steps on the oracle's single-step entry, started from an
    undistributed pack: (set, row before the step, forcing, 'walk')"""
    dt_us = DTS[dt_name]
    sets = hs_sets() if kind == "hs" else hps_sets()
    rng = np.random.default_rng({"hs": 11, "hps": 12}[kind] * 100 + list(DTS).index(dt_name))
    width = HS_ROW if kind == "hs" else HPS_ROW
    pool = []
    for w in range(N_WALKS):
        k = int(rng.integers(len(sets)))
        row = np.zeros(width)
        if rng.random() > 0.15:
            row[0] = float(np.exp(rng.uniform(np.log(0.05), np.log(200.0))))
            row[1] = float(rng.choice([rng.uniform(0.0, 1.0), 1.0, rng.uniform(0.0, 0.3)]))
        if kind == "hps":
            row[2] = float(rng.choice([30000.0, 0.0, -rng.uniform(0.0, 60000.0)]))
        for _ in range(int(rng.integers(1, 7))):
            f = _random_forcing(rng, kind, sets[k], dt_us)
            pool.append((k, row.copy(), f, "walk"))
            try:
                row = _run_oracle(kind, k, row, dt_us, f)[0]
            except RuntimeError:
                break
    return pool


def _nb(x):
    return edge_sets.neighbours(x, 1)


def _base_rows(kind, pool):
    """per set: a distributed row at partial cover with every bin filled where the walks reach one, else any
    distributed row with snow"""
    sets = hs_sets() if kind == "hs" else hps_sets()
    nbc = 2 if kind == "hs" else 3
    best = {}
    for k, row, _, _ in pool:
        n = len(sets[k]["I"])
        if int(row[nbc]) != n or row[0] <= 1.0:
            continue
        sp = row[nbc + 1:nbc + 1 + n]
        score = (0.0 < row[1] < 1.0) + 2 * bool((sp > 0.0).all()) + bool((row[nbc + 1 + MB:nbc + 1 + MB + n] > 0.0).any())
        if k not in best or score > best[k][0]:
            best[k] = (score, row.copy())
    return {k: v[1] for k, v in best.items()}


def _hand_made(kind, pool, dt_name):
    """rows that put a value on, and one double to either side of, each comparison (module docstring)"""
    dt_us = DTS[dt_name]
    h = dt_us / HOUR
    sid = (dt_us / 1e6) / 86400.0
    sets = hs_sets() if kind == "hs" else hps_sets()
    base = _base_rows(kind, pool)
    nbc = 2 if kind == "hs" else 3          # column of n_bins
    o_sp, o_sw = nbc + 1, nbc + 1 + MB
    width = HS_ROW if kind == "hs" else HPS_ROW
    jobs = []

    def add(tag, k, row, temp, prec, wind=2.0, rh=0.7, rad=100.0):
        jobs.append((k, np.array(row, dtype=np.float64), (float(temp), float(prec), float(wind), float(rh), float(rad)),
                     tag))

    def undistributed(swe, sca, nb=0.0):
        row = np.zeros(width)
        row[0], row[1], row[nbc] = swe, sca, nb
        if kind == "hps":
            row[2] = 30000.0
        return row

    for k, p in enumerate(sets):
        n = len(p["I"])
        iv = p["I"]
        tx = p["tx"]
        b = base.get(k)
        # temp == tx exactly and its neighbours, with precipitation
        for t in _nb(tx):
            if b is not None:
                add("temp_at_tx", k, b, t, 2.0 / h)
            add("temp_at_tx", k, undistributed(20.0, 0.6), t, 2.0 / h)
        # swe + snow on either side of the reset threshold (no precipitation: swe itself)
        for v in _nb(0.1 if kind == "hs" else HPS_TOL):
            add("reset_threshold", k, undistributed(v, 0.5), tx + 1.0, 0.0)
            if b is not None:
                r = b.copy()
                r[0] = v
                add("reset_threshold", k, r, tx - 1.0, 0.0)
        # run-start distribute: a bin count of 0, of the set's, of another set's; swe and sca about 1e-3; stale slots
        for other in (0.0, float(n), 8.0 if n != 8 else 5.0, 5.0 if n != 5 else 3.0):
            for swe in _nb(1.0e-3) + [30.0]:
                for sca in _nb(1.0e-3) + [0.45, 1.0]:
                    if swe < 1.0 and sca < 0.4 and (swe != 1.0e-3 and sca != 1.0e-3):
                        continue
                    r = undistributed(swe, sca, other)
                    if other > 0.0:
                        r[o_sp:o_sp + MB] = 1.5 + 0.25 * np.arange(MB)   # stale beyond the count, live below it
                        r[o_sw:o_sw + MB] = 0.125
                        if kind == "hps":
                            r[o_sw + MB:o_sw + 2 * MB] = 0.7
                            r[o_sw + 2 * MB:o_sw + 3 * MB] = 3.0
                    add("bin_count", k, r, tx - 2.0, 1.0 / h)
                    if swe > 1.0:                       # without snowfall the tiny packs only reset
                        add("bin_count", k, r, tx + 3.0, 0.0)
        if b is None:
            continue
        # sca at the rescale's bounds, at an interval edge and at 1, before snowfall
        for c in [1.0e-5, 1.0 - 1.0e-5, 1.0] + list(iv[1:-1]):
            for sca in _nb(c):
                r = b.copy()
                r[1] = sca
                add("sca_edge", k, r, tx - 1.0, 3.0 / h)
                add("sca_edge", k, r, tx + 4.0, 0.0)
        if kind == "hs":
            ts, cx, cfr = p["ts"], p["cx"], p["cfr"]
            for t in _nb(ts):                                              # potmelt == 0 exactly
                add("temp_at_ts", k, b, t, 0.0)
                add("temp_at_ts", k, b, t, 1.5 / h)
            temp = ts + 6.0
            potmelt = cx * sid * (temp - ts)
            for j in range(n):                                            # a bin with sp == potmelt
                for v in _nb(potmelt):
                    r = b.copy()
                    r[o_sp + j] = v
                    add("sp_at_potmelt", k, r, temp, 0.0)
            # sca < 1e-6 after melt: the front in bin 1 of a pack that only fills bin 0
            r = undistributed(0.0, 0.5 * iv[1], float(n))
            r[o_sp] = potmelt * (1.0 + 1.0e-6)
            r[0] = integrate0(list(r[o_sp:o_sp + n]), iv, n, float(r[1]), True)[0]
            add("sca_tiny_after_melt", k, r, temp, 0.0)
            r = r.copy()
            r[o_sp] = potmelt * 1.5
            r[0] = integrate0(list(r[o_sp:o_sp + n]), iv, n, float(r[1]), True)[0]
            add("front_zero", k, r, temp, 0.0)
            temp = ts - 4.0                                               # sw + rain == -potmelt (no rain)
            pm = cx * sid * (temp - ts) * cfr
            for j in range(n):
                for v in _nb(-pm):
                    r = b.copy()
                    r[o_sp + j] = max(r[o_sp + j], 1.0)
                    r[o_sw + j] = v
                    add("sw_at_refreeze", k, r, temp, 0.0)
        else:
            for c in (0.0, 2.09 / 1.16):                                   # T about 0 and about sst's zero
                for t in _nb(c):
                    for prec in (0.0, 1.0 / h):
                        add("T_edge", k, b, t, prec)
            for sh in (30000.0, 0.0, -40000.0):                            # delta_sh of both signs
                r = b.copy()
                r[2] = sh
                for t in (-6.0, 3.0):
                    add("delta_sh", k, r, t, 0.0, wind=0.0)
                    add("delta_sh", k, r, t, 0.5 / h, rad=0.0)
            # per-bin albedos that differ: some bins melt, others refreeze, in the same step
            r = b.copy()
            r[2] = 0.0
            r[o_sw + MB:o_sw + MB + n] = np.where(np.arange(n) % 2 == 0, p["min_albedo"], p["max_albedo"])
            for t in np.linspace(-3.0, 3.0, 13):
                for rad in (150.0, 400.0, 800.0):
                    add("mixed_albedo", k, r, float(t), 0.0, rad=rad, wind=0.0, rh=0.5)
    return jobs


def _cause(labels):
    for c in ("rescale_idx0", "rescale_idxk", "melt_front_pos", "melt_front_zero", "dist_corr", "refreeze"):
        if c in labels:
            return c
    return "other"


@functools.lru_cache(maxsize=None)
def snow_jobs(kind, dt_name):
    """the selected jobs of one snow routine at one time step: dict k [n], row [n][.], f [n][5], tag, labels, raises.
    Every hand-made row, then walk steps in pool order while they add to a label still below QUOTA clean jobs, then
    up to 6 raising walk steps per cause."""
    dt_us = DTS[dt_name]
    pool = _walk_pool(kind, dt_name)
    all_labels = HS_LABELS if kind == "hs" else HPS_LABELS
    count = {lab: 0 for lab in all_labels}
    causes = {}
    chosen = []
    n_reset = 0

    def take(job, labels):
        chosen.append(job + (labels,))
        if RAISE not in labels:
            for lab in labels:
                count[lab] += 1

    for job in _hand_made(kind, pool, dt_name):
        labels = _run_python(kind, job[0], job[1], dt_us, job[2])[2]
        if RAISE in labels:
            c = _cause(labels)
            if causes.get(c, 0) >= 6:
                continue
            causes[c] = causes.get(c, 0) + 1
        take(job, labels)
    for job in pool:
        labels = _run_python(kind, job[0], job[1], dt_us, job[2])[2]
        if RAISE in labels:
            c = _cause(labels)
            if causes.get(c, 0) < 6:
                causes[c] = causes.get(c, 0) + 1
                take(job, labels)
        elif any(count[lab] < QUOTA for lab in labels):
            if "reset" in labels:
                if n_reset >= 20:
                    continue
                n_reset += 1
            take(job, labels)
    if len(chosen) % 64 == 0:     # a cell count that is a multiple of neither 64 nor 256
        chosen.append(chosen[0])
    return dict(k=np.array([c[0] for c in chosen], dtype=np.int32), row=np.stack([c[1] for c in chosen]),
                f=np.array([c[2] for c in chosen]), tag=[c[3] for c in chosen], labels=[c[4] for c in chosen],
                raises=np.array([RAISE in c[4] for c in chosen]))


def label_counts(jobs, labels):
    """clean jobs per label"""
    return {lab: sum(1 for L, r in zip(jobs["labels"], jobs["raises"]) if lab in L and not r) for lab in labels}


# ---- region rows ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geo_rows(n, seed):
    """varied geo fractions, two catchments: the step tail is not constant across the jobs"""
    from tests import engines
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        glacier = float(rng.choice([0.0, 0.0, 0.05, 0.3, 0.9]))
        lake = float(rng.choice([0.0, 0.05])) if glacier < 0.9 else 0.0
        reservoir = float(rng.choice([0.0, 0.19, 0.04])) if glacier < 0.9 else 0.0
        rows.append(engines.geo_row(x=500.0 + 1000.0 * i, z=100.0 + i % 700, cid=1 + i % 2, glacier=glacier, lake=lake,
                                    reservoir=reservoir, area=float(rng.choice([1.0e6, 2.5e5]))))
    return np.stack(rows)


def stack_state(stack, rows, seed):
    """the stack's flat state rows around the snow rows: hbv_stack's soil moisture and tank levels on either side of
    lp, fc and uz1, the others' kirchner q"""
    rng = np.random.default_rng(seed)
    n = rows.shape[0]
    if stack == "hbv_stack":
        st = np.zeros((n, oracle_lib.HBV_FLAT))
        st[:, 0:2] = rows[:, 0:2]
        st[:, 2] = rng.choice([0.0, 0.03, 5.0, 100.0, 200.0, 400.0], n) * rng.uniform(0.5, 1.5, n)
        st[:, 3] = rng.uniform(0.0, 60.0, n)
        st[:, 4] = rng.uniform(0.0, 40.0, n)
        st[:, 5:] = rows[:, 2:]
    elif stack == "pt_hs_k":
        st = np.zeros((n, oracle_lib.PTHSK_FLAT))
        st[:, :HS_ROW] = rows
        st[:, -1] = np.exp(rng.uniform(np.log(0.01), np.log(5.0), n))
    else:
        st = np.zeros((n, oracle_lib.PTHPSK_FLAT))
        st[:, :HPS_ROW] = rows
        st[:, -1] = np.exp(rng.uniform(np.log(0.01), np.log(5.0), n))
    return st


def stack_jobs(stack, dt_name):
    return snow_jobs("hps" if stack == "pt_hps_k" else "hs", dt_name)


def region_case(stack, dt_name, select=None):
    """the region whose cells are the jobs `select` (bool mask or index array; default: the clean jobs) of a stack at
    one time step: dict geo, params, dist, gm_direct, set_ix, state, forcing [5][1][n], dt_us, jobs (indices)"""
    jobs = stack_jobs(stack, dt_name)
    idx = np.flatnonzero(~jobs["raises"]) if select is None else np.arange(len(jobs["k"]))[select]
    if select is None and len(idx) % 64 == 0:   # a cell count that is a multiple of neither 64 nor 256
        idx = np.append(idx, idx[0])
    seed = STACKS.index(stack) * 10 + list(DTS).index(dt_name)
    n_all = len(jobs["k"])
    geo = geo_rows(n_all, 500 + seed)[idx]
    state = stack_state(stack, jobs["row"], 600 + seed)[idx]
    return dict(geo=geo, params=stack_params(stack), dist=dist_rows(), set_ix=jobs["k"][idx].copy(), state=state,
                forcing=np.ascontiguousarray(jobs["f"][idx].T[:, None, :]), dt_us=DTS[dt_name], jobs=idx,
                gm_direct=list(HPS_GM_DIRECT))


def run_oracle_region(stack, case, set_ix="case", params=None, dist=None, gm_direct=None, **kw):
    """the oracle's region run of a case (T0 = 0): full series, state series and final state"""
    ix = case["set_ix"] if isinstance(set_ix, str) else set_ix
    params = case["params"] if params is None else params
    dist = case["dist"] if dist is None else dist
    args = (case["geo"], params, case["state"], 0, case["dt_us"], case["forcing"])
    kw = dict(dict(full=True, collect_state=True), **kw)
    if stack == "hbv_stack":
        return oracle_lib.hbv_run(*args, set_ix=ix, snow_dist=dist, **kw)
    if stack == "pt_hs_k":
        return oracle_lib.pthsk_run(*args, set_ix=ix, snow_dist=dist, **kw)
    gm = case["gm_direct"] if gm_direct is None else gm_direct
    return oracle_lib.pthpsk_run(*args, set_ix=ix, gm_direct=gm, snow_dist=dist, **kw)


def hbv_tail_labels(case, ref):
    """labels of the rest of an hbv_stack step per cell, from the oracle's response (full series: snow_outflow 4,
    glacier_melt 5, ae 6, soil_outflow 8) and state"""
    pow_ = oracle_lib.load("detmath").oracle_pow
    out = []
    scale = 1 / (3600.0 * 1000.0)
    for c in range(case["geo"].shape[0]):
        p = case["params"][case["set_ix"][c]]
        fc, beta, lp, uz1 = (float(v) for v in p[0:4])
        area = float(case["geo"][c, 3])
        sm, uz = float(case["state"][c, 2]), float(case["state"][c, 3])
        insoil = float(ref["full"][4, 0, c]) / (area * scale)   # back from m3/s: labels only, not compared
        ae = float(ref["full"][6, 0, c])
        soil_out = float(ref["full"][8, 0, c])
        gm_mmh = float(ref["full"][5, 0, c]) / (scale * area)
        L = {"sm_lt_lp" if sm < lp else "sm_ge_lp", "beta2" if beta == 2.0 else "beta_pow"}
        soil_temp = sm + insoil
        L.add("soil_clamp" if insoil * pow_(soil_temp / fc, beta) > soil_temp else "soil_noclamp")
        L.add("sm_clamped0" if sm + insoil - soil_out - ae <= 0.0 else "sm_pos")
        tank_temp = uz + (soil_out + (1 - float(p[20])) * gm_mmh)
        L.add("q12_pos" if (tank_temp - uz1) * float(p[4]) > 0.0 else "q12_zero")
        L.add("tank_above_uz1" if tank_temp > uz1 else "tank_below_uz1")
        out.append(frozenset(L))
    return out


# ---- scripted sequences ----------------------------------------------------------------------------------------------
SEQ_T = 11
SEQ_CELLS = 12
SEQ_REQUIRED = ("snowfall_on_partial_cover", "partial_melt", "rain_on_partial_cover", "refreeze", "melt_to_nothing",
                "reset_then_snowfall")
HPS_SEQ_REQUIRED = SEQ_REQUIRED + ("front_assignment_then_integrated",)


def _script(rng, kind, p, dt_us):
    """one candidate: SEQ_T steps of forcing in which one branch's output is the next step's input (snowfall, partial
    melt, snowfall and rain onto partial cover, refreeze, melt to nothing, reset, snowfall again); the amounts are
    drawn so that candidates differ in which bins the melt front passes"""
    h = dt_us / HOUR
    sid = (dt_us / 1e6) / 86400.0
    tx = p["tx"]
    s = p["s"]
    r1, r2 = rng.uniform(min(s), max(s)), rng.uniform(0.2, 1.5)
    if kind == "hs":
        u = 5.0 * rng.uniform(0.3, 3.0)
        ts, cx = p["ts"], p["cx"]
        melt = lambda x: ts + x / (cx * sid)  # noqa: E731
        f = [(tx - 5.0, 6.0 * u / h), (melt(6.0 * u * r1), 0.0), (tx - 1.0, u / h), (max(tx, ts) + 0.5, 2.0 * u / h),
             (ts - 3.0, 0.0), (ts - 3.0, 0.5 * u / h), (melt(u * r2), 0.0), (melt(100.0 * u), 0.0), (tx + 1.0, 0.0),
             (tx - 2.0, 3.0 * u / h), (melt(0.5 * u), 0.2 * u / h)]
        return [(float(t), float(pr), 2.0, 0.7, 100.0) for t, pr in f]
    u = 2.0 * h * rng.uniform(0.2, 2.0)
    warm = lambda: (rng.uniform(1.0, 12.0), rng.uniform(0.0, 800.0))  # noqa: E731
    (t1, q1), (t2, q2), (t3, q3) = warm(), warm(), warm()
    f = [(tx - 5.0, 6.0 * u * r2 / h, 0.0), (t1, 0.0, q1), (tx - 1.0, u / h, 50.0), (max(tx, 0.0) + 1.5, 2.0 * u / h, q2),
         (-8.0, 0.0, 0.0), (min(tx - 0.5, -0.5), 0.5 * u / h, 0.0), (t3, 0.0, q3), (25.0, 0.0, 800.0), (25.0, 0.0, 800.0),
         (tx - 2.0, 3.0 * u / h, 100.0), (3.0, 0.2 * u / h, 300.0)]
    wind = rng.uniform(0.0, 6.0)
    return [(float(t), float(pr), float(wind), 0.7, float(q)) for t, pr, q in f]


def _seq_events(kind, steps):
    """steps: per step (labels, sca before, forcing) -> the scripted events this sequence passes through"""
    ev = set()
    for i, (L, sca0, f) in enumerate(steps):
        partial = 0.0 < sca0 < 1.0
        if partial and ("rescale_idx0" in L or "rescale_idxk" in L):
            ev.add("snowfall_on_partial_cover")
        if "us_gone" in L and "us_melt" in L:
            ev.add("partial_melt")
        if partial and "rain" in L and f[1] > 0.0 and "reset" not in L:
            ev.add("rain_on_partial_cover")
        if "rf_partial" in L or "rf_all" in L:
            ev.add("refreeze")
        if "melt_idx0" in L:
            ev.add("melt_to_nothing")
        if i > 0 and "reset" in steps[i - 1][0] and "snow" in L and "reset" not in L:
            ev.add("reset_then_snowfall")
        if i > 0 and "melt_front_pos" in steps[i - 1][0] and "swe_zero" not in L and "reset" not in L:
            ev.add("front_assignment_then_integrated")
    return ev


@functools.lru_cache(maxsize=None)
def sequences(kind, dt_name):
    """SEQ_CELLS scripted sequences that run clean on the restatement, picked from 400 seeded candidates so that
    together they pass through every scripted event: dict k [n], f [SEQ_T][n][5], events (per cell)"""
    dt_us = DTS[dt_name]
    sets = hs_sets() if kind == "hs" else hps_sets()
    rng = np.random.default_rng({"hs": 21, "hps": 22}[kind] * 100 + list(DTS).index(dt_name))
    cands = []
    for c in range(400):
        k = c % len(sets)
        f = _script(rng, kind, sets[k], dt_us)
        row = np.zeros(HS_ROW if kind == "hs" else HPS_ROW)
        if kind == "hps":
            row[2] = 30000.0
        steps = []
        for ft in f:
            new, _, L = _run_python(kind, k, row, dt_us, ft)
            if RAISE in L:
                steps = None
                break
            steps.append((L, float(row[1]), ft))
            row = new
        if steps is not None:
            cands.append((k, f, _seq_events(kind, steps)))
    chosen, seen = [], set()
    for k, f, ev in cands:     # first the candidates that add an event, then fill up in order
        if ev - seen and len(chosen) < SEQ_CELLS:
            chosen.append((k, f, ev))
            seen |= ev
    for c in cands:
        if len(chosen) < SEQ_CELLS and not any(c is d for d in chosen):
            chosen.append(c)
    return dict(k=np.array([c[0] for c in chosen], dtype=np.int32),
                f=np.array([c[1] for c in chosen]).transpose(1, 0, 2).copy(), events=[c[2] for c in chosen])


def sequence_case(stack, dt_name):
    """the region of the scripted sequences of a stack: as region_case, with forcing [5][SEQ_T][n]"""
    seq = sequences("hps" if stack == "pt_hps_k" else "hs", dt_name)
    n = len(seq["k"])
    rows = np.zeros((n, HPS_ROW if stack == "pt_hps_k" else HS_ROW))
    if stack == "pt_hps_k":
        rows[:, 2] = 30000.0
    return dict(geo=geo_rows(n, 700), params=stack_params(stack), dist=dist_rows(), set_ix=seq["k"].copy(),
                state=stack_state(stack, rows, 701), forcing=np.ascontiguousarray(seq["f"].transpose(2, 0, 1)),
                dt_us=DTS[dt_name], gm_direct=list(HPS_GM_DIRECT), events=seq["events"])
