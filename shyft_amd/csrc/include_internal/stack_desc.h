// Internal: what the host library knows about each method stack, one row per stack. Everything that is a constant
// of the stack (widths, counts, row indices, texts) is read from here; region.hip branches on the stack only where
// the behaviour differs (which launcher runs, pt_gs_k's derived columns).
#pragma once
#include "../../../include/shyft_hip.h"
#include "layout.h"

struct stack_desc {
    int id;                   // SHYFT_HIP_PT_GS_K ...
    const char* run_kernel;   // the run kernel, as named when its stream is synchronised
    int n_ref_params;         // the reference's parameter count (its get/set order)
    int param_width;          // the host row: the reference values, then what this library adds (snow distribution)
    int k_gm_direct;          // row index of gm.direct_response
    int k_rsv_drf;            // row index of reservoir_direct_response_fraction
    int snow_dist_index;      // hbv_snow distribution (n_bins, s[HBV_MAX_BINS], intervals[HBV_MAX_BINS]), or -1
    int n_state_fields;
    int n_state_series;       // state-collector series per cell (pt_ss_k collects 7 series from its 8 state values)
    int n_full_series;        // response series of the full collection
    int n_cellc;              // per-cell constant rows
    int c_area;               // the cell area's row among them
    const char* param_error;  // the reference's text for a parameter vector of the wrong size
};

constexpr stack_desc STACK_TABLE[] = {
    {SHYFT_HIP_PT_GS_K, "ptgsk_run_kernel", PTGSK_NP_REF, PTGSK_NP_REF, PK_GM_DIRECT, PK_RSV_DRF, -1, PTGSK_NS,
     PTGSK_NS, PTGSK_NR, PTGSK_NC, PC_AREA, "PTGSK Parameter Accessor: .set size missmatch"},
    {SHYFT_HIP_HBV_STACK, "hbv_run_kernel", HBV_NP_REF, HBV_NP, HK_GM_DIRECT, HK_RSV_DRF, HK_NB, HBV_NS, HBV_NS,
     HBV_NR, HBV_NC, HC_AREA, "HBV_Stack Parameter Accessor: .set size missmatch"},
    {SHYFT_HIP_PT_SS_K, "ptssk_run_kernel", PTSSK_NP, PTSSK_NP, SK_GM_DIRECT, SK_RSV_DRF, -1, PTSSK_NS, PTSSK_NSC,
     PTGSK_NR, PTGSK_NC, PC_AREA, "pt_ss_k parameter accessor: .set size mismatch"},
    // the two texts below are the reference's own (pt_hs_k.h:68, pt_hps_k.h:70 say pt_ss_k)
    {SHYFT_HIP_PT_HS_K, "pthsk_run_kernel", PTHSK_NP_REF, PTHSK_NP, PH_GM_DIRECT, PH_RSV_DRF, PH_NB, PTHSK_NS,
     PTHSK_NSC, PTGSK_NR, PTGSK_NC, PC_AREA, "pt_ss_k parameter accessor: .set size missmatch"},
    {SHYFT_HIP_PT_HPS_K, "pthpsk_run_kernel", PTHPSK_NP_REF, PTHPSK_NP, PP_GM_DIRECT, PP_RSV_DRF, PP_NB, PTHPSK_NS,
     PTHPSK_NSC, PTGSK_NR, PTGSK_NC, PC_AREA, "pt_ss_k parameter accessor: .set size missmatch"},
};

inline const stack_desc* stack_desc_of(int id) {
    for (const stack_desc& d : STACK_TABLE)
        if (d.id == id) return &d;
    return nullptr;
}
