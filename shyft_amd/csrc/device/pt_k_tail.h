// The part of a pt_ss_k / pt_hs_k / pt_hps_k step after the snow routine (pt_ss_k.h:262-289, pt_hs_k.h:253-281,
// pt_hps_k.h:268-297: the same statements): glacier melt on the post-step snow covered area, Priestley-Taylor,
// actual evapotranspiration, kirchner, total discharge and charge, expression for expression in the reference's
// order (FP contraction is off; the kernels are compared with the oracle bit for bit).
// pt_gs_k's kernel keeps its own copy: its loop places parameter loads inside this part.
#pragma once
#include "ptgsk_dev.h"  // kirchner_step, pt_pot_evap_exp (pt_dev.h), smax, the error codes (layout.h)

namespace shyft_dev {

// the parameter values the tail reads; gm_routed = 1 - gm_direct
struct pt_k_tail_par { double kc1, kc2, kc3, ae_scale, dtf, pt_albedo, pt_alpha, gm_direct, gm_routed; };
struct pt_k_tail_out { double discharge_m3s, charge_m3s, gm_melt_m3s, ae, pot_evap; };

// The per-cell constants come by reference: a kernel that keeps them in LDS reads each at its point of use.
// sca is the post-step snow covered area, snow_outflow the snow routine's outflow in mm/h; q (kirchner state) and
// err are updated.
template <bool INLINE_MATH>
__device__ __forceinline__ pt_k_tail_out pt_k_tail(
    const pt_k_tail_par& p, const double& glacier_fraction, const double& snow_storage_fraction,
    const double& kirchner_routed_prec, const double& direct_response_fraction, const double& kirchner_fraction,
    const double& cell_area_m2, const double& glacier_area_m2, double t1_hours, double temp, double rad, double rel_hum,
    double prec, double sca, double snow_outflow, double& q, int32_t& err) {
    const double mmh_to_m3s_scale_factor = 1 / (3600.0 * 1000.0);
    pt_k_tail_out o;
    // glacier_melt::step (glacier_melt.h:47-52) on the post-step snow covered area
    const double sca_area = cell_area_m2 * sca;
    o.gm_melt_m3s = 0.0;
    if (!(glacier_area_m2 <= sca_area || temp <= 0.0))
        o.gm_melt_m3s = p.dtf * temp * (glacier_area_m2 - sca_area) * (0.001 / 86400.0);
    double ae_exp;  // actual_evapotranspiration's exp, evaluated beside Priestley-Taylor's (pt_pot_evap_exp)
    o.pot_evap = pt_pot_evap_exp<INLINE_MATH>(p.pt_albedo, p.pt_alpha, temp, rad, rel_hum, -q * 3.0 / p.ae_scale, ae_exp) * 3600.0;
    // actual_evapotranspiration::calculate_step (actual_evapotranspiration.h:40-62)
    o.ae = o.pot_evap * (1.0 - ae_exp) * (1.0 - smax(sca, glacier_fraction));
    const double gm_mmh = o.gm_melt_m3s / (mmh_to_m3s_scale_factor * cell_area_m2);
    double q_avg;
    if (!kirchner_step<INLINE_MATH>(q, q_avg, snow_outflow * snow_storage_fraction + prec * kirchner_routed_prec + p.gm_routed * gm_mmh,
                                    o.ae, t1_hours, p.kc1, p.kc2, p.kc3))
        err = ERR_KIRCHNER_MAX_ITER;
    const double total_discharge = smax(0.0, prec - o.ae) * direct_response_fraction + p.gm_direct * gm_mmh +
                                   q_avg * kirchner_fraction;
    o.charge_m3s = +(cell_area_m2 * prec * mmh_to_m3s_scale_factor) -
                   (cell_area_m2 * o.ae * mmh_to_m3s_scale_factor) + o.gm_melt_m3s -
                   (cell_area_m2 * total_discharge * mmh_to_m3s_scale_factor);
    o.discharge_m3s = cell_area_m2 * total_discharge * mmh_to_m3s_scale_factor;
    return o;
}

}  // namespace shyft_dev
