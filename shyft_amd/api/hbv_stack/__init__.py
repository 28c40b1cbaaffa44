"""shyft_amd.api.hbv_stack -- the reference's `shyft.api.hbv_stack` (api/boostpython/hbv_stack.cpp,
shyft/api/hbv_stack/__init__.py) over the MI355X engine."""
from __future__ import annotations

from .. import (_api, _FlatState, _make_models, _ModelMixin, _SnowDistributionParameter, _Statistics, _Vector,
                SERIES_STATE, make_state_with_id_types)

# get/set order and names (core/hbv_stack.h:82-170), defaults (hbv_soil.h:19-24, hbv_actual_evapotranspiration.h,
# hbv_tank.h:19-31, hbv_snow.h:49-53, routing.h:76)
_NAMES = ("soil.fc", "soil.beta", "ae.lp", "tank.uz1", "tank.kuz2", "tank.kuz1", "tank.perc", "tank.klz", "hs.lw",
          "hs.tx", "hs.cx", "hs.ts", "hs.cfr", "p_corr.scale_factor", "pt.albedo", "pt.alpha", "gm.dtf",
          "routing.velocity", "routing.alpha", "routing.beta", "gm.direct_response",
          "msp.reservoir_direct_response_fraction")
_DEFAULTS = (300.0, 2.0, 150.0, 25.0, 0.5, 0.3, 0.8, 0.02, 0.1, 0.0, 1.0, 0.0, 0.5, 1.0, 0.2, 1.26, 6.0, 1.0, 7.0,
             0.0, 0.0, 1.0)
MAX_BINS = 8


class HbvParameter(_SnowDistributionParameter):
    NAMES = _NAMES
    DEFAULTS = _DEFAULTS
    ERROR = "HBV_Stack Parameter Accessor: .set size missmatch"


class _HbvState(_FlatState):
    NAMES = ("snow.swe", "snow.sca", "soil.sm", "tank.uz", "tank.lz", "snow.n_bins") + \
        tuple(f"snow.sp{i}" for i in range(MAX_BINS)) + tuple(f"snow.sw{i}" for i in range(MAX_BINS))
    DEFAULTS = (0.0, 0.0, 0.0, 20.0, 10.0, 0.0) + (0.0,) * (2 * MAX_BINS)


class HbvState(_HbvState):
    """hbv_stack::state (hbv_stack.h:181-201): snow (swe, sca, sp/sw bins), soil.sm, tank.uz/lz."""


class HbvStateVector(_Vector):
    pass


HbvParameterMap = dict
_SERIES = ("avg_discharge", "charge_m3s", "snow_sca", "snow_swe", "snow_outflow", "glacier_melt", "ae_output",
           "pe_output", "soil_outflow")
_STATE_SERIES = ("snow_swe", "snow_sca", "soil_moisture", "tank_uz", "tank_lz", "snow_n_bins") + \
    tuple(f"sp{i}" for i in range(MAX_BINS)) + tuple(f"sw{i}" for i in range(MAX_BINS))


# cell-identified state (api_state.h:62-75) and its serialisation (api/boostpython/api_state.cpp)
HbvStateWithId, HbvStateWithIdVector, deserialize_from_bytes = make_state_with_id_types(
    "Hbv", HbvState, HbvStateVector, 2)


class _HbvBase(_ModelMixin):
    _state_with_id_vector_t = HbvStateWithIdVector
    _parameter_t = HbvParameter
    _state_t = HbvState
    _state_vector_t = HbvStateVector
    _SERIES = _SERIES
    _STATE_SERIES = _STATE_SERIES

    @property
    def hbv_snow_state(self):  # hbv_snow_cell_state_statistics (api.h:1050-1162): averages of sc.snow_swe/sca
        return _Statistics(self, {"swe": (SERIES_STATE + 0, True), "sca": (SERIES_STATE + 1, True)})

    @property
    def hbv_snow_response(self):  # hbv_snow_cell_response_statistics (api.h:1163-1206)
        return _Statistics(self, {"outflow": (4, False), "sca": (2, True), "swe": (3, True),
                                  "glacier_melt": (5, False)})

    @property
    def soil_state(self):  # hbv_soil_cell_state_statistics (api.h:424-444): sums of sc.soil_moisture
        return _Statistics(self, {"discharge": (SERIES_STATE + 2, False)})

    @property
    def tank_state(self):  # hbv_tank_cell_state_statistics (api.h:446-468): sums of sc.tank_uz
        return _Statistics(self, {"discharge": (SERIES_STATE + 3, False), "uz": (SERIES_STATE + 3, False),
                                  "lz": (SERIES_STATE + 4, False)})

    hbv_tank_state = tank_state

    @property
    def priestley_taylor_response(self):
        return _Statistics(self, {"output": (7, True)})

    @property
    def hbv_actual_evaptranspiration_response(self):
        return _Statistics(self, {"output": (6, True)})

    @property
    def soil_response(self):  # hbv_soil_cell_response_statistics (api.h:1472-1497)
        return _Statistics(self, {"output": (8, True)})


HbvModel, HbvOptModel, create_opt_model_clone, create_full_model_clone, HbvOptimizer = _make_models(
    "Hbv", _HbvBase, _api._HbvRegionModel, _api._HbvOptimizer,
    ("region_model<hbv_stack cell_complete_response_t> (hbv_stack.cpp:140).",
     "region_model<hbv_stack cell_discharge_response_t> (hbv_stack.cpp:141)."))
