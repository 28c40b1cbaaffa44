"""shyft_amd.api.pt_hs_k -- the reference's `shyft.api.pt_hs_k` (api/boostpython/pt_hs_k.cpp,
shyft/api/pt_hs_k/__init__.py) over the MI355X engine."""
from __future__ import annotations

from .. import (_api, _FlatState, _make_models, _ModelMixin, _SnowDistributionParameter, _Statistics, _Vector,
                SERIES_STATE, make_state_with_id_types)

# get/set order and names (core/pt_hs_k.h:66-143); defaults of the member structs (kirchner.h:120-125,
# hbv_snow.h:49-53, priestley_taylor.h, glacier_melt.h, routing.h:76, mstack_param.h)
_NAMES = ("kirchner.c1", "kirchner.c2", "kirchner.c3", "ae.ae_scale_factor", "hs.lw", "hs.tx", "hs.cx", "hs.ts",
          "hs.cfr", "gm.dtf", "p_corr.scale_factor", "pt.albedo", "pt.alpha", "routing.velocity", "routing.alpha",
          "routing.beta", "gm.direct_response", "msp.reservoir_direct_response_fraction")
_DEFAULTS = (-2.439, 0.966, -0.10, 1.5, 0.1, 0.0, 1.0, 0.0, 0.5, 6.0, 1.0, 0.2, 1.26, 1.0, 7.0, 0.0, 0.0, 1.0)
MAX_BINS = 8


class PTHSKParameter(_SnowDistributionParameter):
    NAMES = _NAMES
    DEFAULTS = _DEFAULTS
    ERROR = "pt_ss_k parameter accessor: .set size missmatch"  # the reference's text (pt_hs_k.h:68)


class PTHSKState(_FlatState):
    """pt_hs_k::state (pt_hs_k.h:148-172): snow = hbv_snow::state (swe, sca, sp/sw bins), kirchner.q."""
    NAMES = (("snow.swe", "snow.sca", "snow.n_bins") + tuple(f"snow.sp{i}" for i in range(MAX_BINS)) +
             tuple(f"snow.sw{i}" for i in range(MAX_BINS)) + ("kirchner.q",))
    DEFAULTS = (0.0, 0.0, 0.0) + (0.0,) * (2 * MAX_BINS) + (0.1,)


class PTHSKStateVector(_Vector):
    pass


PTHSKParameterMap = dict
_SERIES = ("avg_discharge", "charge_m3s", "snow_sca", "snow_swe", "snow_outflow", "glacier_melt", "ae_output",
           "pe_output")
_STATE_SERIES = (("kirchner_discharge", "snow_sca", "snow_swe") + tuple(f"snow_sp{i}" for i in range(MAX_BINS)) +
                 tuple(f"snow_sw{i}" for i in range(MAX_BINS)))


# cell-identified state (api_state.h:62-75) and its serialisation (api/boostpython/api_state.cpp)
PTHSKStateWithId, PTHSKStateWithIdVector, deserialize_from_bytes = make_state_with_id_types(
    "PTHSK", PTHSKState, PTHSKStateVector, 4)


class _PTHSKBase(_ModelMixin):
    _state_with_id_vector_t = PTHSKStateWithIdVector
    _parameter_t = PTHSKParameter
    _state_t = PTHSKState
    _state_vector_t = PTHSKStateVector
    _SERIES = _SERIES
    _STATE_SERIES = _STATE_SERIES

    @property
    def hbv_snow_state(self):  # hbv_snow_cell_state_statistics (api.h:1050-1162): averages of sc.snow_swe/sca
        return _Statistics(self, {"swe": (SERIES_STATE + 2, True), "sca": (SERIES_STATE + 1, True)})

    @property
    def hbv_snow_response(self):  # hbv_snow_cell_response_statistics (api.h:1163-1206)
        return _Statistics(self, {"outflow": (4, False), "sca": (2, True), "swe": (3, True),
                                  "glacier_melt": (5, False)})

    @property
    def kirchner_state(self):
        return _Statistics(self, {"discharge": (SERIES_STATE + 0, False)})

    @property
    def priestley_taylor_response(self):
        return _Statistics(self, {"output": (7, True)})

    @property
    def actual_evaptranspiration_response(self):
        return _Statistics(self, {"output": (6, True), "pot_ratio": ("pot_ratio", True)})


PTHSKModel, PTHSKOptModel, create_opt_model_clone, create_full_model_clone, PTHSKOptimizer = _make_models(
    "PTHSK", _PTHSKBase, _api._PTHSKRegionModel, _api._PTHSKOptimizer,
    ("region_model<pt_hs_k cell_complete_response_t> (pt_hs_k.cpp models()).",
     "region_model<pt_hs_k cell_discharge_response_t> (pt_hs_k.cpp models())."))
