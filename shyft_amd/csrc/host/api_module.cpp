// pybind11 module shyft_amd.api._api: the Python surface of the host layer.
//
// The reference exposes region_model<cell_t> and its data types with
// boost.python (api/boostpython/expose.h:98-430, api_*.cpp, pt_gs_k.cpp:34-174,
// hbv_stack.cpp). boost.python is not available here, so this module binds the
// same C++ host classes (host/region_model.hpp) with pybind11; the Python
// package shyft_amd.api adds the reference's names and decorators on top
// (shyft/api/__init__.py, shyft/api/pt_gs_k/__init__.py).
//
// Time crosses the boundary as seconds (int or float, like shyft's `time`);
// internally it is int64 microseconds.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/functional.h>
#include <pybind11/stl.h>

#include <cmath>
#include <optional>
#include <set>

#include "calibration.hpp"
#include "forecast.hpp"
#include "kalman.hpp"
#include "qm.hpp"
#include "region_model.hpp"
#include "ts_expr.hpp"
#include "ts_percentiles.hpp"

namespace py = pybind11;
using namespace shyft_hip::host;

namespace {

utctime to_us(double seconds) { return utctime(std::llround(seconds * 1e6)); }
double to_s(utctime us) { return double(us) / 1e6; }

// the point series of a list as the CSR arrays of the batched series entries: (row, t, v, t_end, fx)
py::tuple series_csr(const py::list& series) {
    std::vector<const point_ts*> src;
    for (auto h : series) src.push_back(&h.cast<const point_ts&>());
    const size_t S = src.size();
    const py::ssize_t n_series = py::ssize_t(S);
    py::array_t<int64_t> row(n_series + 1), t_end(n_series);
    py::array_t<int32_t> fx(n_series);
    int64_t* r = row.mutable_data();
    r[0] = 0;
    for (size_t s = 0; s < S; ++s) {
        r[s + 1] = r[s] + int64_t(src[s]->size());
        t_end.mutable_data()[s] = src[s]->t_end;
        fx.mutable_data()[s] = int32_t(src[s]->fx);
    }
    const py::ssize_t n_points = py::ssize_t(r[S]);
    py::array_t<int64_t> t(n_points);
    py::array_t<double> v(n_points);
    for (size_t s = 0; s < S; ++s) {
        std::copy(src[s]->t.begin(), src[s]->t.end(), t.mutable_data() + r[s]);
        std::copy(src[s]->v.begin(), src[s]->v.end(), v.mutable_data() + r[s]);
    }
    return py::make_tuple(row, t, v, t_end, fx);
}

// The same for api.percentiles: row s keeps the points that its views can read on an axis (view_window of
// host/ts_percentiles.hpp), lo[s] and hi[s] the axis' start and end taken back by the largest and the smallest shift of
// the views of row s
py::tuple percentile_rows(const py::list& series, const std::vector<int64_t>& lo, const std::vector<int64_t>& hi) {
    std::vector<const point_ts*> src;
    for (auto h : series) src.push_back(&h.cast<const point_ts&>());
    const size_t S = src.size();
    if (lo.size() != S || hi.size() != S) throw std::runtime_error("percentiles: one window per stored series");
    const py::ssize_t n_series = py::ssize_t(S);
    py::array_t<int64_t> row(n_series + 1), t_end(n_series);
    py::array_t<int32_t> fx(n_series);
    std::vector<std::pair<size_t, size_t>> keep(S);
    int64_t* r = row.mutable_data();
    r[0] = 0;
    for (size_t s = 0; s < S; ++s) {
        keep[s] = view_window(*src[s], lo[s], hi[s]);
        r[s + 1] = r[s] + int64_t(keep[s].second - keep[s].first);
        t_end.mutable_data()[s] = src[s]->t_end;
        fx.mutable_data()[s] = int32_t(src[s]->fx);
    }
    const py::ssize_t n_points = py::ssize_t(r[S]);
    py::array_t<int64_t> t(n_points);
    py::array_t<double> v(n_points);
    for (size_t s = 0; s < S; ++s) {
        std::copy(src[s]->t.begin() + keep[s].first, src[s]->t.begin() + keep[s].second, t.mutable_data() + r[s]);
        std::copy(src[s]->v.begin() + keep[s].first, src[s]->v.begin() + keep[s].second, v.mutable_data() + r[s]);
    }
    return py::make_tuple(row, t, v, t_end, fx);
}

// An expression tree from Python into expr::tree. A terminal is a _PointTs; any other node a tuple (kind, op, a, b)
// with kind and op of host/ts_expr.hpp: a and b trees for TS_TS, a tree and a float for TS_S and S_TS (the series
// first in both), a tree and None for ABS_TS. A series that occurs more than once is one terminal of the batch.
int32_t add_expr_node(const py::handle& h, expr::tree& tr, py::list& series, std::map<const point_ts*, int32_t>& index) {
    expr::node x;
    if (py::isinstance<point_ts>(h)) {
        const point_ts* p = &h.cast<const point_ts&>();
        auto it = index.find(p);
        if (it == index.end()) {
            it = index.emplace(p, int32_t(series.size())).first;
            series.append(h);
        }
        x.kind = expr::TERMINAL;
        x.a = it->second;
    } else {
        const py::tuple tu = h.cast<py::tuple>();
        if (tu.size() != 4) throw std::runtime_error("ts_expr: a node is a series or a tuple (kind, op, a, b)");
        x.kind = tu[0].cast<int32_t>();
        x.op = tu[1].cast<int32_t>();
        x.a = add_expr_node(tu[2], tr, series, index);
        if (x.kind == expr::TS_TS) x.b = add_expr_node(tu[3], tr, series, index);
        else if (x.kind == expr::TS_S || x.kind == expr::S_TS) x.s = tu[3].cast<double>();
    }
    tr.nodes.push_back(x);
    return int32_t(tr.nodes.size() - 1);
}

template <class T>
py::array_t<T> as_array(const std::vector<T>& v) {
    return py::array_t<T>(py::ssize_t(v.size()), v.data());
}

// The plans of a list of trees: (terminals, prog_row, prog, consts, periods, orow, ot, fx, t_end, depth). terminals
// is the list of distinct _PointTs in terminal order (for _series_csr); fx, t_end and depth are per expression: the
// root's point type, the end of the root axis, and the deepest evaluation stack.
py::tuple ts_expr_plan(const py::list& trees) {
    py::list series;
    std::map<const point_ts*, int32_t> index;
    std::vector<expr::tree> parsed;
    for (auto h : trees) {
        parsed.emplace_back();
        add_expr_node(h, parsed.back(), series, index);
    }
    std::vector<expr::terminal> terminals;
    for (auto h : series) {
        const point_ts& s = h.cast<const point_ts&>();
        terminals.push_back({expr::axis{s.t, s.t_end}, s.fx});
    }
    expr::tables tb;
    std::vector<int64_t> prog_row{0}, orow{0}, ot, t_end;
    std::vector<int32_t> prog, fx, depth;
    for (const auto& tr : parsed) {
        const expr::plan p = expr::make_plan(tr, terminals, tb);
        prog.insert(prog.end(), p.prog.begin(), p.prog.end());
        prog_row.push_back(int64_t(prog.size()));
        ot.insert(ot.end(), p.ta.t.begin(), p.ta.t.end());
        orow.push_back(int64_t(ot.size()));
        fx.push_back(int32_t(p.fx));
        t_end.push_back(p.ta.t_end);
        depth.push_back(p.depth);
    }
    py::array_t<int64_t> periods({py::ssize_t(tb.periods.size() / 2), py::ssize_t(2)});
    std::copy(tb.periods.begin(), tb.periods.end(), periods.mutable_data());
    return py::make_tuple(series, as_array(prog_row), as_array(prog), as_array(tb.consts), periods, as_array(orow),
                          as_array(ot), as_array(fx), as_array(t_end), as_array(depth));
}

template <class Stack>
void bind_model(py::module_& m, const char* name) {
    using M = region_model<Stack>;
    py::class_<M>(m, name, py::dynamic_attr())
        .def(py::init<const std::vector<geo_cell_data>&, const std::vector<double>&, bool, int, const std::vector<int>&,
                      unsigned>(),
             py::arg("geo_data_vector"), py::arg("region_param"), py::arg("full_collection") = true,
             py::arg("device") = -1, py::arg("devices") = std::vector<int>(), py::arg("shard_flags") = 0u)
        .def(py::init<const std::vector<geo_cell_data>&, const std::vector<double>&,
                      const std::map<int64_t, std::vector<double>>&, bool, const std::vector<int>&, unsigned>(),
             py::arg("geo_data_vector"), py::arg("region_param"), py::arg("catchment_parameters"),
             py::arg("full_collection") = true, py::arg("devices") = std::vector<int>(), py::arg("shard_flags") = 0u)
        .def_property_readonly("shard_devices", &M::shard_devices)
        .def(py::init<const M&, bool>(), py::arg("other_model"), py::arg("full_collection"))
        .def_readwrite("ncore", &M::ncore)
        .def_readwrite("_ip_parameter", &M::ip_parameter)
        .def_readwrite("_region_env", &M::region_env)
        .def_readwrite("_initial_state", &M::initial_state)
        .def_readwrite("_river_network", &M::rivers)
        .def_property_readonly("_time_axis", [](const M& x) { return x.time_axis; })
        .def_property_readonly("full_collection", &M::full_collection)
        .def("size", &M::size)
        .def("number_of_catchments", &M::number_of_catchments)
        .def_property_readonly("catchment_ids", &M::catchment_ids)
        .def("extract_geo_cell_data", &M::extract_geo_cell_data)
        .def("_set_region_parameter", &M::set_region_parameter)
        .def("_get_region_parameter", &M::get_region_parameter)
        .def("_set_catchment_parameter", &M::set_catchment_parameter)
        .def("_update_catchment_parameter", &M::update_catchment_parameter)
        .def("remove_catchment_parameter", &M::remove_catchment_parameter, py::arg("catchment_id"))
        .def("has_catchment_parameter", &M::has_catchment_parameter, py::arg("catchment_id"))
        .def("_get_catchment_parameter", &M::get_catchment_parameter)
        .def("set_catchment_calculation_filter", &M::set_catchment_calculation_filter, py::arg("catchment_id_list"))
        .def("set_calculation_filter", &M::set_calculation_filter, py::arg("catchment_id_list"), py::arg("river_id_list"))
        .def("is_calculated", &M::is_calculated, py::arg("catchment_id"))
        .def("initialize_cell_environment", &M::initialize_cell_environment, py::arg("time_axis"))
        .def("_interpolate", &M::interpolate)
        .def("_run_interpolation", &M::run_interpolation)
        .def("is_cell_env_ts_ok", &M::is_cell_env_ts_ok)
        .def("run_cells", &M::run_cells, py::arg("use_ncore") = 0, py::arg("start_step") = 0, py::arg("n_steps") = 0,
             py::call_guard<py::gil_scoped_release>())
        .def("_get_states", [](const M& x) { return x.current_state(); })
        .def("_set_states", &M::set_states)
        .def("revert_to_initial_state", &M::revert_to_initial_state)
        .def("_extract_state", &M::extract_state)
        .def("_apply_state", &M::apply_state)
        .def("adjust_q", &M::adjust_q, py::arg("q_scale"), py::arg("cids"))
        .def("adjust_state_to_target_flow", &M::adjust_state_to_target_flow, py::arg("wanted_flow_m3s"),
             py::arg("cids"), py::arg("start_step") = 0, py::arg("scale_range") = 3.0, py::arg("scale_eps") = 1e-3,
             py::arg("max_iter") = 300, py::arg("n_steps") = 1)
        .def("set_state_collection", &M::set_state_collection, py::arg("catchment_id"), py::arg("on_or_off"))
        .def("set_snow_sca_swe_collection", &M::set_snow_sca_swe_collection, py::arg("catchment_id"), py::arg("on_or_off"))
        .def("_cell_collects_state", &M::cell_collects_state)
        .def("_cell_collects_snow", &M::cell_collects_snow)
        .def("_cell_series", [](const M& x, int s, size_t c) { auto v = x.cell_series(s, c); return py::array_t<double>(v.size(), v.data()); })
        .def("_cell_value", &M::cell_value)
        .def("_set_cell_value", &M::set_cell_value)
        .def("_set_cell_forcing", &M::set_cell_forcing)
        .def("_cell_geo", [](const M& x, size_t i) { return x.cells_geo().at(i); })
        .def("_cell_parameter", &M::cell_parameter)
        .def("_stat_series", [](const M& x, int s, const std::vector<int64_t>& ids, int scope, bool w) {
            auto v = x.stat_series(s, ids, scope, w);
            return py::array_t<double>(v.size(), v.data());
        })
        .def("_percentiles", [](const M& x, int s, const std::vector<int64_t>& ids, int scope,
                                const std::vector<int64_t>& pcts) {
            auto v = x.percentiles(s, ids, scope, pcts);
            py::array_t<double> a({pcts.size(), x.series_length(s)});
            std::copy(v.begin(), v.end(), a.mutable_data());
            return a;
        })
        .def("_catchment_percentiles", [](const M& x, int s, const std::vector<int64_t>& pcts) {
            auto v = x.catchment_percentiles(s, pcts);
            py::array_t<double> a({x.number_of_catchments(), pcts.size(), x.series_length(s)});
            std::copy(v.begin(), v.end(), a.mutable_data());
            return a;
        })
        .def("_stat_value", &M::stat_value)
        .def("_stat_raster", &M::stat_raster)
        .def("_pot_ratio_series", [](const M& x, const std::vector<int64_t>& ids, int scope) {
            auto v = x.pot_ratio_series(ids, scope);
            return py::array_t<double>(v.size(), v.data());
        })
        .def("_pot_ratio_raster", &M::pot_ratio_raster)
        .def("_pot_ratio_value", &M::pot_ratio_value)
        .def("_area_stat", &M::area_stat)
        .def("_catchment_sums", &M::catchment_sums)
        .def("connect_catchment_to_river", &M::connect_catchment_to_river, py::arg("cid"), py::arg("rid"))
        .def("_set_cell_routing", &M::set_cell_routing)
        .def("has_routing", &M::has_routing)
        .def("_river_output_flow_m3s", &M::river_output_flow_m3s)
        .def("_ensemble_run", &M::ensemble_run, py::call_guard<py::gil_scoped_release>())
        .def("_ensemble_last_ms", &M::ensemble_last_ms)
        .def("_ensemble_routed", [](const M& x, const std::vector<int64_t>& rids, int which) {
            auto v = x.ensemble_routed(rids, which);
            const size_t T = x.time_axis.size();
            py::array_t<double> a({T ? v.size() / (T * std::max<size_t>(1, rids.size())) : size_t(0), rids.size(), T});
            std::copy(v.begin(), v.end(), a.mutable_data());
            return a;
        }, py::arg("rids"), py::arg("which") = 2)
        .def("_river_upstream_inflow_m3s", &M::river_upstream_inflow_m3s)
        .def("_river_local_inflow_m3s", &M::river_local_inflow_m3s);
}

// model_calibration::optimizer<region_model> (expose.h:472-730 model_calibrator)
template <class Stack>
void bind_optimizer(py::module_& m, const char* name) {
    using M = region_model<Stack>;
    using O = optimizer<M>;
    py::class_<O>(m, name)
        .def(py::init<M&, const std::vector<target_specification>&, const std::vector<double>&, const std::vector<double>&>(),
             py::arg("model"), py::arg("targets"), py::arg("p_min"), py::arg("p_max"), py::keep_alive<1, 2>())
        .def(py::init<M&>(), py::arg("model"), py::keep_alive<1, 2>())
        .def("_set_target_specification", &O::set_target_specification)
        .def("_set_parameter_ranges", &O::set_parameter_ranges)
        .def_readwrite("_targets", &O::targets)
        .def_readwrite("_lower", &O::parameter_lower_bound)
        .def_readwrite("_upper", &O::parameter_upper_bound)
        .def_readwrite("batch_evaluation", &O::batch_evaluation)
        .def_readwrite("max_batch_members", &O::max_batch_members)
        .def_readonly("n_batched_evaluations", &O::n_batched_evaluations)
        .def_readonly("n_sequential_evaluations", &O::n_sequential_evaluations)
        .def("establish_initial_state_from_model", &O::establish_initial_state_from_model)
        .def("_get_initial_state", &O::get_initial_state)
        .def("set_verbose_level", &O::set_verbose_level, py::arg("level"))
        .def("reset_states", &O::reset_states)
        .def("parameter_active", &O::active_parameter, py::arg("i"))
        .def_property_readonly("trace_size", &O::trace_size)
        .def_readonly("trace_goal_function_values", &O::goal_fn_trace)
        .def("trace_goal_function_value", &O::trace_goal_fn, py::arg("i"))
        .def("_trace_parameter", &O::trace_parameter)
        .def("_calculate_goal_function", &O::calculate_goal_function, py::call_guard<py::gil_scoped_release>())
        .def("_calculate_goal_functions", &O::calculate_goal_functions, py::call_guard<py::gil_scoped_release>())
        .def("_optimize", &O::optimize, py::call_guard<py::gil_scoped_release>())
        .def("_optimize_global", &O::optimize_global, py::call_guard<py::gil_scoped_release>())
        .def("_optimize_sceua", &O::optimize_sceua, py::call_guard<py::gil_scoped_release>())
        .def("_optimize_dream", &O::optimize_dream, py::call_guard<py::gil_scoped_release>())
        .def("_to_scaled", &O::to_scaled)
        .def("_from_scaled", &O::from_scaled);
}

}  // namespace

PYBIND11_MODULE(_api, m) {
    m.doc() = "MI355X region engine host layer (C++ over the shyft_hip C ABI)";

    py::class_<geo_point>(m, "GeoPoint")
        .def(py::init<>())
        .def(py::init<double, double, double>(), py::arg("x"), py::arg("y"), py::arg("z"))
        .def_readwrite("x", &geo_point::x)
        .def_readwrite("y", &geo_point::y)
        .def_readwrite("z", &geo_point::z)
        .def("__deepcopy__", [](const geo_point& p, py::dict) { return p; })
        .def_static("distance2", [](const geo_point& a, const geo_point& b) {
            return (a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y) + (a.z - b.z) * (a.z - b.z);
        })
        .def("__repr__", [](const geo_point& p) {
            return "GeoPoint(" + std::to_string(p.x) + ", " + std::to_string(p.y) + ", " + std::to_string(p.z) + ")";
        });

    py::class_<land_type_fractions>(m, "LandTypeFractions")
        .def(py::init<>())
        .def(py::init<double, double, double, double, double>(), py::arg("glacier"), py::arg("lake"),
             py::arg("reservoir"), py::arg("forest"), py::arg("unspecified"))
        .def("glacier", &land_type_fractions::glacier)
        .def("lake", &land_type_fractions::lake)
        .def("reservoir", &land_type_fractions::reservoir)
        .def("forest", &land_type_fractions::forest)
        .def("unspecified", &land_type_fractions::unspecified)
        .def("snow_storage", &land_type_fractions::snow_storage)
        .def("set_fractions", &land_type_fractions::set_fractions, py::arg("glacier"), py::arg("lake"),
             py::arg("reservoir"), py::arg("forest"));

    py::class_<routing_info>(m, "RoutingInfo")
        .def(py::init<>())
        .def(py::init<int64_t, double>(), py::arg("id"), py::arg("distance") = 0.0)
        .def_readwrite("id", &routing_info::id)
        .def_readwrite("distance", &routing_info::distance);

    py::class_<geo_cell_data>(m, "GeoCellData")
        .def(py::init<>())
        .def(py::init<const geo_point&, double, int64_t, double, const land_type_fractions&>(), py::arg("mid_point"),
             py::arg("area"), py::arg("catchment_id"), py::arg("radiation_slope_factor") = 0.9,
             py::arg("land_type_fractions") = land_type_fractions())
        .def("mid_point", &geo_cell_data::mid_point)
        .def("area", &geo_cell_data::area)
        .def("catchment_id", &geo_cell_data::catchment_id)
        .def("set_catchment_id", [](geo_cell_data& g, int64_t c) { g.catchment_id_ = c; })
        .def("radiation_slope_factor", &geo_cell_data::radiation_slope_factor)
        .def("land_type_fractions_info", [](geo_cell_data& g) -> land_type_fractions& { return g.fractions; },
             py::return_value_policy::reference_internal)
        .def("set_land_type_fractions", [](geo_cell_data& g, const land_type_fractions& f) { g.fractions = f; })
        .def_readwrite("routing_info", &geo_cell_data::routing)
        .def_readwrite("routing", &geo_cell_data::routing);

    py::class_<fixed_dt>(m, "TimeAxisFixedDeltaT")
        .def(py::init([](double t0, double dt, size_t n) { return fixed_dt(to_us(t0), to_us(dt), n); }), py::arg("start"),
             py::arg("delta_t"), py::arg("n"))
        .def("size", &fixed_dt::size)
        .def("__len__", &fixed_dt::size)
        .def_property_readonly("start", [](const fixed_dt& a) { return to_s(a.t); })
        .def_property_readonly("delta_t", [](const fixed_dt& a) { return to_s(a.dt); })
        .def_property_readonly("n", [](const fixed_dt& a) { return a.n; })
        .def("time", [](const fixed_dt& a, size_t i) { return to_s(a.time(i)); })
        .def("period", [](const fixed_dt& a, size_t i) { auto p = a.period(i); return std::make_pair(to_s(p.start), to_s(p.end)); })
        .def("total_period", [](const fixed_dt& a) { auto p = a.total_period(); return std::make_pair(to_s(p.start), to_s(p.end)); })
        .def("index_of", [](const fixed_dt& a, double t) { auto i = a.index_of(to_us(t)); return i == npos ? int64_t(-1) : int64_t(i); })
        .def("__eq__", &fixed_dt::operator==);

    py::enum_<ts_point_fx>(m, "point_interpretation_policy")
        .value("POINT_INSTANT_VALUE", POINT_INSTANT_VALUE)
        .value("POINT_AVERAGE_VALUE", POINT_AVERAGE_VALUE)
        .export_values();

    py::class_<point_ts>(m, "_PointTs")
        .def(py::init([](const fixed_dt& ta, std::vector<double> v, ts_point_fx fx) { return point_ts(ta, std::move(v), fx); }))
        .def(py::init([](const std::vector<double>& t, double t_end, std::vector<double> v, ts_point_fx fx) {
            std::vector<utctime> tu(t.size());
            for (size_t i = 0; i < t.size(); ++i) tu[i] = to_us(t[i]);
            return point_ts(std::move(tu), to_us(t_end), std::move(v), fx);
        }))
        .def("__deepcopy__", [](const point_ts& s, py::dict) { return point_ts(s); })
        .def("size", &point_ts::size)
        .def("value", &point_ts::value)
        .def("set", &point_ts::set)
        .def("time", [](const point_ts& s, size_t i) { return to_s(s.time(i)); })
        .def("point_interpretation", [](const point_ts& s) { return s.fx; })
        .def("total_period", [](const point_ts& s) { auto p = s.total_period(); return std::make_pair(to_s(p.start), to_s(p.end)); })
        .def("__call__", [](const point_ts& s, double t) { return s(to_us(t)); })
        // the interval that holds t, -1 outside the series (point_ts::index_of, core/time_series.h:343)
        .def("index_of", [](const point_ts& s, double t) { auto i = index_of(s, to_us(t)); return i == npos ? int64_t(-1) : int64_t(i); })
        .def_property_readonly("_values", [](const point_ts& s) { return py::array_t<double>(s.v.size(), s.v.data()); })
        .def_property_readonly("_times", [](const point_ts& s) {
            std::vector<double> t(s.t.size());
            for (size_t i = 0; i < t.size(); ++i) t[i] = to_s(s.t[i]);
            return t;
        })
        .def_property_readonly("_t_end", [](const point_ts& s) { return to_s(s.t_end); })
        // the step [us] of the TimeAxisFixedDeltaT the series was built on, 0 for any other series (derivative)
        .def_property_readonly("_fixed_dt_us", [](const point_ts& s) { return s.fixed_step; })
        // the series on the same points with other values (the results of the observation-preparation calls)
        .def("_with_values", [](const point_ts& s, const std::vector<double>& v, ts_point_fx fx) {
            if (v.size() != s.size()) throw std::runtime_error("point_ts: values and time-axis differ in size");
            point_ts r(s);
            r.v = v;
            r.fx = fx;
            return r;
        })
        // f(t) at times in microseconds, and the total period in microseconds
        .def("_sample_us", [](const point_ts& s, const std::vector<int64_t>& t) {
            py::array_t<double> r(py::ssize_t(t.size()));
            for (size_t i = 0; i < t.size(); ++i) r.mutable_data()[i] = s(t[i]);
            return r;
        })
        .def("_total_period_us", [](const point_ts& s) { auto p = s.total_period(); return std::make_pair(p.start, p.end); })
        // the series with dt [s] added to every time and to t_end (a terminal under time_shift, host/ts_expr.hpp)
        .def("_shifted", [](const point_ts& s, double dt) {
            point_ts r(s);
            const utctime d = to_us(dt);
            for (auto& x : r.t) x += d;
            r.t_end += d;
            return r;
        })
        // a series from times in microseconds (the root axis of an expression); no points is the empty series
        .def_static("_from_us", [](const py::array_t<int64_t, py::array::c_style | py::array::forcecast>& t, utctime t_end,
                                   const py::array_t<double, py::array::c_style | py::array::forcecast>& v, ts_point_fx fx) {
            return point_ts(std::vector<utctime>(t.data(), t.data() + t.size()), t_end,
                            std::vector<double>(v.data(), v.data() + v.size()), fx);
        })
        .def("average", [](const point_ts& s, const fixed_dt& ta) {
            auto v = average_values(s, ta);
            return py::array_t<double>(v.size(), v.data());
        });

    py::class_<geo_point_ts>(m, "_GeoPointTs")
        .def(py::init([](const geo_point& p, const point_ts& ts) { return geo_point_ts{p, ts, ""}; }))
        .def_readwrite("_mid_point", &geo_point_ts::mid_point)
        .def_readwrite("_ts", &geo_point_ts::ts)
        .def_readwrite("uid", &geo_point_ts::uid);

    py::class_<region_environment>(m, "_RegionEnvironment")
        .def(py::init<>())
        .def_readwrite("temperature", &region_environment::temperature)
        .def_readwrite("precipitation", &region_environment::precipitation)
        .def_readwrite("wind_speed", &region_environment::wind_speed)
        .def_readwrite("rel_hum", &region_environment::rel_hum)
        .def_readwrite("radiation", &region_environment::radiation);

    py::class_<idw_parameter>(m, "IDWParameter")
        .def(py::init<>())
        .def(py::init([](size_t mm, double md, double f, double zs) {
                 idw_parameter p; p.max_members = mm; p.max_distance = md; p.distance_measure_factor = f; p.zscale = zs;
                 return p;
             }),
             py::arg("max_members") = 10, py::arg("max_distance") = 200000.0, py::arg("distance_measure_factor") = 2.0,
             py::arg("zscale") = 1.0)
        .def_readwrite("max_members", &idw_parameter::max_members)
        .def_readwrite("max_distance", &idw_parameter::max_distance)
        .def_readwrite("distance_measure_factor", &idw_parameter::distance_measure_factor)
        .def_readwrite("zscale", &idw_parameter::zscale);
    py::class_<idw_temperature_parameter, idw_parameter>(m, "IDWTemperatureParameter")
        .def(py::init<>())
        .def(py::init([](double g, size_t mm, double md, bool eq) {
                 idw_temperature_parameter p; p.default_temp_gradient = g; p.max_members = mm; p.max_distance = md;
                 p.gradient_by_equation = eq; return p;
             }),
             py::arg("default_gradient") = -0.006, py::arg("max_members") = 20, py::arg("max_distance") = 200000.0,
             py::arg("gradient_by_equation") = false)
        .def_readwrite("default_temp_gradient", &idw_temperature_parameter::default_temp_gradient)
        .def_readwrite("gradient_by_equation", &idw_temperature_parameter::gradient_by_equation);
    py::class_<idw_precipitation_parameter, idw_parameter>(m, "IDWPrecipitationParameter")
        .def(py::init<>())
        .def(py::init([](double s, size_t mm, double md) {
                 idw_precipitation_parameter p; p.scale_factor = s; p.max_members = mm; p.max_distance = md; return p;
             }),
             py::arg("scale_factor") = 1.02, py::arg("max_members") = 20, py::arg("max_distance") = 200000.0)
        .def_readwrite("scale_factor", &idw_precipitation_parameter::scale_factor);
    // CellStateId (api/api_state.h:34-59; api/boostpython/api_state.cpp)
    py::class_<cell_state_id>(m, "CellStateId")
        .def(py::init<>())
        .def(py::init<int64_t, int64_t, int64_t, int64_t>(), py::arg("cid"), py::arg("x"), py::arg("y"), py::arg("area"))
        .def_readwrite("cid", &cell_state_id::cid)
        .def_readwrite("x", &cell_state_id::x)
        .def_readwrite("y", &cell_state_id::y)
        .def_readwrite("area", &cell_state_id::area)
        .def("__eq__", &cell_state_id::operator==)
        .def("__ne__", &cell_state_id::operator!=)
        .def("__lt__", &cell_state_id::operator<)
        .def("__hash__", [](const cell_state_id& c) { return py::hash(py::make_tuple(c.cid, c.x, c.y, c.area)); })
        .def("__repr__", [](const cell_state_id& c) {
            return "CellStateId(" + std::to_string(c.cid) + ", " + std::to_string(c.x) + ", " + std::to_string(c.y) +
                   ", " + std::to_string(c.area) + ")";
        });
    m.def("_serialize_states", [](int stack, size_t n_fields, const std::vector<state_with_id>& v) {
        auto b = serialize_states(stack, n_fields, v);
        return py::bytes(b.data(), b.size());
    });
    m.def("_deserialize_states", [](const py::bytes& b, int stack, size_t n_fields) {
        std::string s = b;
        return deserialize_states(std::vector<char>(s.begin(), s.end()), stack, n_fields);
    });
    // BTKParameter (api/boostpython/api_interpolation.cpp:188-200)
    py::class_<btk_parameter>(m, "BTKParameter")
        .def(py::init<>())
        .def(py::init<double, double>(), py::arg("temperature_gradient"), py::arg("temperature_gradient_sd"))
        .def(py::init<double, double, double, double, double, double>(), py::arg("temperature_gradient"),
             py::arg("temperature_gradient_sd"), py::arg("sill"), py::arg("nugget"), py::arg("range"), py::arg("zscale"))
        .def("temperature_gradient", [](const btk_parameter& p, std::pair<double, double> period) {
                 return p.temperature_gradient(utcperiod(to_us(period.first), to_us(period.second)));
             }, py::arg("p"))
        .def("temperature_gradient_sd", &btk_parameter::temperature_gradient_sd)
        .def("sill", &btk_parameter::sill)
        .def("nug", &btk_parameter::nug)
        .def("range", &btk_parameter::range)
        .def("zscale", &btk_parameter::zscale);
    // bayesian_kriging_temperature (api_interpolation.cpp:54-71): validation, sources averaged onto the axis,
    // one source copied, else the device BTK
    m.def("_bayesian_kriging_temperature", [](const std::vector<geo_point_ts>& src, const std::vector<geo_point>& dst,
                                              const fixed_dt& ta, const btk_parameter& p) {
        if (src.empty() || dst.empty())
            throw std::runtime_error("the supplied src and dst_points should be non-null and have at least one time-series");
        if (ta.size() == 0 || ta.dt == 0)
            throw std::runtime_error("the supplied destination time-axis should have more than 0 element, and a delta-t larger than 0");
        const size_t S = src.size(), T = ta.size(), D = dst.size();
        std::vector<double> xyz(3 * S), vals(T * S), prior(T), prm(5), dxyz(3 * D), out(T * D);
        for (size_t s = 0; s < S; ++s) {
            xyz[3 * s] = src[s].mid_point.x;
            xyz[3 * s + 1] = src[s].mid_point.y;
            xyz[3 * s + 2] = src[s].mid_point.z;
            auto v = average_values(src[s].ts, ta);
            for (size_t t = 0; t < T; ++t) vals[t * S + s] = v[t];
        }
        for (size_t d = 0; d < D; ++d) {
            dxyz[3 * d] = dst[d].x;
            dxyz[3 * d + 1] = dst[d].y;
            dxyz[3 * d + 2] = dst[d].z;
        }
        for (size_t t = 0; t < T; ++t) prior[t] = p.temperature_gradient(ta.period(t));
        p.as_abi(prm.data());
        {
            py::gil_scoped_release nogil;
            throw_if(shyft_hip_btk(-1, S, xyz.data(), vals.data(), T, prior.data(), prm.data(), D, dxyz.data(),
                                   out.data()),
                     nullptr);
        }
        return py::array_t<double>({T, D}, out.data());
    });
    // OKCovarianceType, OKParameter (api_interpolation.cpp:73-84, 149-162)
    py::enum_<ok_covariance_type>(m, "OKCovarianceType", py::arithmetic())
        .value("GAUSSIAN", ok_covariance_type::GAUSSIAN)
        .value("EXPONENTIAL", ok_covariance_type::EXPONENTIAL)
        .export_values();
    py::class_<ok_parameter>(m, "OKParameter")
        .def(py::init([](double c, double a, ok_covariance_type cov_type, double z_scale) {
                 return ok_parameter{c, a, z_scale, cov_type};
             }),
             py::arg("c") = 1.0, py::arg("a") = 10 * 1000.0, py::arg("cov_type") = ok_covariance_type::EXPONENTIAL,
             py::arg("z_scale") = 1.0)
        .def_readwrite("c", &ok_parameter::c)
        .def_readwrite("a", &ok_parameter::a)
        .def_readwrite("cov_type", &ok_parameter::cov_type)
        .def_readwrite("z_scale", &ok_parameter::z_scale);
    // ordinary_kriging (api_interpolation.cpp:86-148): validate_parameters' checks, sources averaged onto the axis,
    // then shyft_hip_ordinary_kriging (its parameter checks, the single-source copy, else the device path)
    m.def("_ordinary_kriging", [](const std::vector<geo_point_ts>& src, const std::vector<geo_point>& dst,
                                  const fixed_dt& ta, const ok_parameter& p) {
        if (src.empty() || dst.empty())
            throw std::runtime_error("the supplied src and dst_points should be non-null and have at least one time-series");
        if (ta.size() == 0 || ta.dt == 0)
            throw std::runtime_error("the supplied destination time-axis should have more than 0 element, and a delta-t larger than 0");
        const size_t S = src.size(), T = ta.size(), D = dst.size();
        std::vector<double> xyz(3 * S), vals(T * S), dxyz(3 * D), out(T * D);
        for (size_t s = 0; s < S; ++s) {
            xyz[3 * s] = src[s].mid_point.x;
            xyz[3 * s + 1] = src[s].mid_point.y;
            xyz[3 * s + 2] = src[s].mid_point.z;
            auto v = average_values(src[s].ts, ta);
            for (size_t t = 0; t < T; ++t) vals[t * S + s] = v[t];
        }
        for (size_t d = 0; d < D; ++d) {
            dxyz[3 * d] = dst[d].x;
            dxyz[3 * d + 1] = dst[d].y;
            dxyz[3 * d + 2] = dst[d].z;
        }
        const double prm[5] = {p.c, p.a, p.z_scale, double(int(p.cov_type)), 0.0};
        {
            py::gil_scoped_release nogil;
            throw_if(shyft_hip_ordinary_kriging(-1, S, xyz.data(), vals.data(), T, prm, D, dxyz.data(), out.data()),
                     nullptr);
        }
        return py::array_t<double>({T, D}, out.data());
    });
    // KalmanParameter, KalmanState, KalmanFilter, KalmanBiasPredictor (api/boostpython/api_kalman.cpp:22-204 over
    // core/kalman.h); the single-filter objects run on the host path of the batched entry (shyft_hip_kalman_run_host)
    {
        namespace kf = shyft_hip::host::kalman;
        auto vec = [](const std::vector<double>& v) { return py::array_t<double>(v.size(), v.data()); };
        auto mat = [](const std::vector<double>& v, int n) {
            return py::array_t<double>({py::ssize_t(n), py::ssize_t(n)}, v.data());
        };
        py::class_<kf::parameter>(m, "KalmanParameter",
                                  "Defines the parameters that tune the kalman-filter algorithm for temperature type of signals")
            .def(py::init<int, double, double, double, double>(), py::arg("n_daily_observations") = 8,
                 py::arg("hourly_correlation") = 0.93, py::arg("covariance_init") = 0.5,
                 py::arg("std_error_bias_measurements") = 2.0, py::arg("ratio_std_w_over_v") = 0.15)
            .def(py::init<const kf::parameter&>(), py::arg("const_ref"))
            .def_readwrite("n_daily_observations", &kf::parameter::n_daily_observations)
            .def_readwrite("hourly_correlation", &kf::parameter::hourly_correlation)
            .def_readwrite("covariance_init", &kf::parameter::covariance_init)
            .def_readwrite("std_error_bias_measurements", &kf::parameter::std_error_bias_measurements)
            .def_readwrite("ratio_std_w_over_v", &kf::parameter::ratio_std_w_over_v);
        py::class_<kf::state>(m, "KalmanState",
                              "The state of the kalman bias filter: x [n] best estimate, k [n] gain, P [n x n] covariance, "
                              "W [n x n] process noise")
            .def(py::init<>())
            .def(py::init<int, double, double, double>(), py::arg("n_daily_observations"), py::arg("covariance_init"),
                 py::arg("hourly_correlation"), py::arg("process_noise_init"))
            .def(py::init<const kf::state&>(), py::arg("clone"))
            .def("size", &kf::state::size)
            .def_static("get_x", [](const kf::state& s) { return s.x; }, py::arg("state"))
            .def_static("get_k", [](const kf::state& s) { return s.k; }, py::arg("state"))
            .def_static("get_P", [](const kf::state& s) { return s.P; }, py::arg("state"))
            .def_static("get_W", [](const kf::state& s) { return s.W; }, py::arg("state"))
            .def_property_readonly("x", [vec](const kf::state& s) { return vec(s.x); })
            .def_property_readonly("k", [vec](const kf::state& s) { return vec(s.k); })
            .def_property_readonly("P", [mat](const kf::state& s) { return mat(s.P, s.size()); })
            .def_property_readonly("W", [mat](const kf::state& s) { return mat(s.W, s.size()); })
            .def("_set", [](kf::state& s, const std::vector<double>& x, const std::vector<double>& k,
                            const std::vector<double>& P) {
                if (x.size() != s.x.size() || k.size() != s.k.size() || P.size() != s.P.size())
                    throw std::runtime_error("kalman: state size mismatch");
                s.x = x;
                s.k = k;
                s.P = P;
            })
            .def("__deepcopy__", [](const kf::state& s, py::dict) { return kf::state(s); });
        py::class_<kf::filter>(m, "KalmanFilter",
                               "Specialized kalman filter for temperature (solar-driven daily bias patterns)")
            .def(py::init<>())
            .def(py::init<const kf::parameter&>(), py::arg("p"))
            .def("create_initial_state", &kf::filter::create_initial_state)
            .def("update", [](const kf::filter& f, double observed_bias, double t, kf::state& s) {
                     f.update(observed_bias, to_us(t), s);
                 }, py::arg("observed_bias"), py::arg("t"), py::arg("state"))
            .def("_fold_to_daily_observation", [](const kf::filter& f, double t) {
                     return f.fold_to_daily_observation(to_us(t));
                 }, py::arg("t"))
            .def("_tables", [](const kf::filter& f, const fixed_dt& ta, bool running) {
                     py::dict d;
                     const auto fold = f.fold_table(ta);
                     d["fold"] = py::array_t<int32_t>(fold.size(), fold.data());
                     d["v2"] = f.v2();
                     if (running) {
                         const auto r = f.running(ta);
                         d["save_every"] = r.save_every;
                         d["piece_begin"] = py::array_t<int32_t>(r.piece_begin.size(), r.piece_begin.data());
                         d["piece_ix"] = py::array_t<int32_t>(r.piece_ix.size(), r.piece_ix.data());
                         d["piece_seconds"] = py::array_t<double>(r.piece_seconds.size(), r.piece_seconds.data());
                     }
                     return d;
                 }, py::arg("time_axis"), py::arg("running") = false)
            .def_readwrite("parameter", &kf::filter::p);
        py::class_<kf::bias_predictor>(m, "_KalmanBiasPredictor")
            .def(py::init<>())
            .def(py::init<const kf::filter&>(), py::arg("filter"))
            .def(py::init<const kf::filter&, const kf::state&>(), py::arg("filter"), py::arg("state"))
            .def("_update_with_forecast", &kf::bias_predictor::update_with_forecast)
            .def("_compute_running_bias", [](kf::bias_predictor& bp, const point_ts& fc, const point_ts& obs,
                                             const fixed_dt& ta) {
                auto v = bp.compute_running_bias(fc, obs, ta);
                return py::array_t<double>(v.size(), v.data());
            })
            .def_readonly("filter", &kf::bias_predictor::f)
            .def_readwrite("state", &kf::bias_predictor::s);
        // the host preparation of KalmanBiasPredictorVector, one call per set instead of one per point:
        // the averages of a set of series on ta, [T][M], and fc - obs of a forecast cycle against them
        m.def("_kalman_average_set", [](const py::list& set, const fixed_dt& ta) {
            const size_t T = ta.size(), M = set.size();
            py::array_t<double> out({py::ssize_t(T), py::ssize_t(M)});
            double* o = out.mutable_data();
            for (size_t j = 0; j < M; ++j) {
                const auto v = average_values(set[j].cast<const point_ts&>(), ta);
                for (size_t i = 0; i < T; ++i) o[i * M + j] = v[i];
            }
            return out;
        });
        m.def("_kalman_observed_bias_set", [](const py::list& fc, const py::array_t<double, py::array::c_style>& obs_avg,
                                              const fixed_dt& ta) {
            const size_t T = ta.size(), M = fc.size();
            if (obs_avg.ndim() != 2 || size_t(obs_avg.shape(0)) != T || size_t(obs_avg.shape(1)) != M)
                throw std::runtime_error("kalman: the observation averages do not match the forecast set");
            py::array_t<double> out({py::ssize_t(T), py::ssize_t(M)});
            double* o = out.mutable_data();
            const double* a = obs_avg.data();
            std::vector<double> col(T);
            for (size_t j = 0; j < M; ++j) {
                for (size_t i = 0; i < T; ++i) col[i] = a[i * M + j];
                const auto v = kf::observed_bias(fc[j].cast<const point_ts&>(), col, ta);
                for (size_t i = 0; i < T; ++i) o[i * M + j] = v[i];
            }
            return out;
        });
        // true when every series of the set has the time axis of the first
        m.def("_kalman_same_axis", [](const py::list& set) {
            for (size_t j = 1; j < set.size(); ++j) {
                const point_ts &a = set[0].cast<const point_ts&>(), &b = set[j].cast<const point_ts&>();
                if (a.t != b.t || a.t_end != b.t_end) return false;
            }
            return true;
        });
    }
    // The host work of quantile_map_forecast (core/time_series_qm.h:401-450; host/qm.hpp): the qm axis, every series
    // averaged onto it once as dense [T][F] / [T][P] matrices (NaN = not covered), the per-step modes, and the
    // historical tail. The mapping itself is region.quantile_map.
    {
        namespace qm = shyft_hip::host::qm;
        static const double no_utctime_s = double(qm::no_utctime) / 1e6;
        m.attr("no_utctime") = no_utctime_s;
        auto qm_us = [](double s) { return s > no_utctime_s ? to_us(s) : qm::no_utctime; };
        m.def("_qm_plan", [qm_us](const py::list& forecasts, const py::list& historical, const fixed_dt& ta,
                                  double interpolation_start, double interpolation_end) {
            std::vector<const point_ts*> fc;
            for (auto h : forecasts) fc.push_back(&h.cast<const point_ts&>());
            const utctime i_start = qm_us(interpolation_start), i_end = qm_us(interpolation_end);
            const qm::plan_t pl = qm::plan(fc, ta, i_start, i_end);
            const size_t T = pl.qm_n_steps, F = fc.size(), P = historical.size();
            py::array_t<double> fcm({py::ssize_t(T), py::ssize_t(F)}), prim({py::ssize_t(T), py::ssize_t(P)});
            double* o = fcm.mutable_data();
            for (size_t j = 0; j < F; ++j) {
                const auto v = average_values(*fc[j], pl.qm_time_axis);
                for (size_t i = 0; i < T; ++i) o[i * F + j] = v[i];
            }
            o = prim.mutable_data();
            for (size_t j = 0; j < P; ++j) {
                const auto v = average_values(historical[j].cast<const point_ts&>(), pl.qm_time_axis);
                for (size_t i = 0; i < T; ++i) o[i * P + j] = v[i];
            }
            std::vector<int32_t> mode;
            std::vector<double> iw;
            qm::step_modes(pl.qm_time_axis, pl.fc_period, i_start, i_end, mode, iw);
            return py::make_tuple(T, fcm, prim, py::array_t<int32_t>(mode.size(), mode.data()),
                                  py::array_t<double>(iw.size(), iw.data()));
        });
        m.def("_qm_tail", [](const py::list& historical, const fixed_dt& ta, size_t qm_n_steps) {
            if (qm_n_steps > ta.size()) throw std::runtime_error("quantile_map_forecast: qm axis longer than the time axis");
            const size_t n = ta.size() - qm_n_steps, P = historical.size();
            py::array_t<double> out({py::ssize_t(P), py::ssize_t(n)});
            double* o = out.mutable_data();
            for (size_t j = 0; j < P; ++j) {
                const auto v = qm::historical_tail(historical[j].cast<const point_ts&>(), ta, qm_n_steps);
                std::copy(v.begin(), v.end(), o + j * n);
            }
            return out;
        });
        // accumulate_stair_case / accumulate_linear (core/time_series_average.h:105-275) by the series' point type
        m.def("_accumulate", [](const point_ts& ts, const fixed_dt& ta, bool avg) {
            const auto v = ts.fx == POINT_AVERAGE_VALUE ? accumulate_stair_case(ta, ts, avg) : accumulate_linear(ta, ts, avg);
            return py::array_t<double>(v.size(), v.data());
        });
    }
    // The host work of region.resample: the point series of a list as the CSR arrays of shyft_hip_resample (row, t, v,
    // t_end, fx) and the axis in microseconds (t0, dt, n).
    m.def("_resample_plan", [](const py::list& series, const fixed_dt& ta) {
        return series_csr(series) + py::make_tuple(int64_t(ta.t), int64_t(ta.dt), ta.size());
    });
    // The host work of region.forecast_skill_csr callers: the CSR arrays alone, and seconds as ticks.
    m.def("_series_csr", &series_csr);
    m.def("_percentile_rows", &percentile_rows);
    m.def("_to_us", &to_us);
    m.def("_ts_expr_plan", &ts_expr_plan);
    // TsVector.forecast_merge (host/forecast.hpp; core/time_series_merge.h:47-99)
    m.def("_forecast_merge", [](const py::list& series, double lead_time, double fc_interval) {
        std::vector<const point_ts*> tsv;
        for (auto h : series) tsv.push_back(&h.cast<const point_ts&>());
        return forecast_merge(tsv, to_us(lead_time), to_us(fc_interval));
    });
    py::class_<interpolation_parameter>(m, "InterpolationParameter")
        .def(py::init<>())
        .def(py::init([](const btk_parameter& t, const idw_precipitation_parameter& p, const idw_parameter& ws,
                         const idw_parameter& rad, const idw_parameter& rh) {
                 interpolation_parameter ip;
                 ip.temperature = t; ip.precipitation = p; ip.wind_speed = ws; ip.radiation = rad; ip.rel_hum = rh;
                 return ip;
             }),
             py::arg("temperature"), py::arg("precipitation"), py::arg("wind_speed"), py::arg("radiation"),
             py::arg("rel_hum"))
        .def(py::init([](const idw_temperature_parameter& t, const idw_precipitation_parameter& p, const idw_parameter& ws,
                         const idw_parameter& rad, const idw_parameter& rh) {
                 interpolation_parameter ip;
                 ip.temperature_idw = t; ip.use_idw_for_temperature = true;  // api_interpolation.cpp:447
                 ip.precipitation = p; ip.wind_speed = ws; ip.radiation = rad; ip.rel_hum = rh;
                 return ip;
             }),
             py::arg("temperature"), py::arg("precipitation"), py::arg("wind_speed"), py::arg("radiation"),
             py::arg("rel_hum"))
        .def_readwrite("temperature", &interpolation_parameter::temperature)
        .def_readwrite("use_idw_for_temperature", &interpolation_parameter::use_idw_for_temperature)
        .def_readwrite("temperature_idw", &interpolation_parameter::temperature_idw)
        .def_readwrite("precipitation", &interpolation_parameter::precipitation)
        .def_readwrite("wind_speed", &interpolation_parameter::wind_speed)
        .def_readwrite("radiation", &interpolation_parameter::radiation)
        .def_readwrite("rel_hum", &interpolation_parameter::rel_hum);

    py::class_<uhg_parameter>(m, "UHGParameter")
        .def(py::init<>())
        .def(py::init<double, double, double>(), py::arg("velocity"), py::arg("alpha") = 7.0, py::arg("beta") = 0.0)
        .def_readwrite("velocity", &uhg_parameter::velocity)
        .def_readwrite("alpha", &uhg_parameter::alpha)
        .def_readwrite("beta", &uhg_parameter::beta);
    py::class_<river>(m, "River")
        .def(py::init([](int64_t id, const routing_info& ds, const uhg_parameter& p) { return river(id, ds.id, ds.distance, p); }),
             py::arg("id"), py::arg("downstream") = routing_info(), py::arg("parameter") = uhg_parameter())
        .def_readwrite("id", &river::id)
        .def_property("downstream", [](const river& r) { return routing_info(r.downstream_id, r.downstream_distance); },
                      [](river& r, const routing_info& ri) { r.downstream_id = ri.id; r.downstream_distance = ri.distance; })
        .def_readwrite("parameter", &river::parameter)
        .def("uhg", [](const river& r, double dt) { return r.uhg(to_us(dt)); });
    py::class_<q_adjust_result>(m, "FlowAdjustResult")
        .def(py::init<>())
        .def_readwrite("q_0", &q_adjust_result::q_0)
        .def_readwrite("q_r", &q_adjust_result::q_r)
        .def_readwrite("diagnostics", &q_adjust_result::diagnostics);
    // the state tuner's 1-D minimiser, exposed for host-side tests (no device work)
    m.def(
        "find_min_single_variable",
        [](const std::function<double(double)>& f, double x, double begin, double end, double eps, long max_iter,
           double radius) {
            const double fx = find_min_single_variable(f, x, begin, end, eps, max_iter, radius);
            return std::make_pair(x, fx);
        },
        py::arg("f"), py::arg("starting_point"), py::arg("begin"), py::arg("end"), py::arg("eps") = 1e-3,
        py::arg("max_iter") = 100, py::arg("initial_search_radius") = 1.0);
    py::class_<river_network>(m, "RiverNetwork")
        .def(py::init<>())
        .def("add", [](river_network& n, const river& r) -> river_network& { return n.add(r); }, py::return_value_policy::reference_internal)
        .def("remove_by_id", &river_network::remove_by_id)
        .def("river_by_id", [](river_network& n, int64_t rid) -> river& { return n.river_by_id(rid); }, py::return_value_policy::reference_internal)
        .def("upstreams_by_id", &river_network::upstreams_by_id)
        .def("downstream_by_id", &river_network::downstream_by_id)
        .def("set_downstream_by_id", &river_network::set_downstream_by_id)
        .def("network_contains_directed_cycle", &river_network::network_contains_directed_cycle);
    m.def("make_uhg_from_gamma", &make_uhg_from_gamma, py::arg("n_steps"), py::arg("alpha"), py::arg("beta"));
    // the routing groups one (velocity, alpha, beta) gives the cells (host only): (group of each cell, river id and
    // UHG weights of each group); rivers restricts the groups to cells routed to those rivers
    m.def(
        "routing_groups",
        [](const std::vector<int64_t>& cell_rid, const std::vector<double>& cell_distance, double dt, double velocity,
           double alpha, double beta, const std::optional<std::vector<int64_t>>& only) {
            if (cell_rid.size() != cell_distance.size()) throw std::runtime_error("routing_groups: one distance per cell");
            std::set<int64_t> net;
            if (only) net.insert(only->begin(), only->end());
            const auto rg = make_routing_groups_of(uhg_parameter(velocity, alpha, beta), cell_rid, cell_distance, to_us(dt),
                                                   only ? &net : nullptr);
            std::vector<int64_t> rid;
            std::vector<std::vector<double>> w;
            for (const auto& g : rg.groups) {
                rid.push_back(g.rid);
                w.push_back(g.w);
            }
            return py::make_tuple(rg.group_of, rid, w);
        },
        py::arg("cell_rid"), py::arg("cell_distance"), py::arg("dt"), py::arg("velocity"), py::arg("alpha") = 7.0,
        py::arg("beta") = 0.0, py::arg("rivers") = py::none());

    m.def("utc_time", [](int y, int mo, int d, int h, int mi, int s) { return to_s(utc_time(y, mo, d, h, mi, s)); });
    m.def("average_values", [](const point_ts& s, const fixed_dt& ta) {
        auto v = average_values(s, ta);
        return py::array_t<double>(v.size(), v.data());
    });

    bind_model<pt_gs_k_stack>(m, "_PTGSKRegionModel");
    bind_model<hbv_stack_stack>(m, "_HbvRegionModel");
    bind_model<pt_ss_k_stack>(m, "_PTSSKRegionModel");
    bind_model<pt_hs_k_stack>(m, "_PTHSKRegionModel");
    bind_model<pt_hps_k_stack>(m, "_PTHPSKRegionModel");

    py::enum_<target_spec_calc_type>(m, "target_spec_calc_type")
        .value("NASH_SUTCLIFFE", NASH_SUTCLIFFE)
        .value("KLING_GUPTA", KLING_GUPTA)
        .value("ABS_DIFF", ABS_DIFF)
        .value("RMSE", RMSE)
        .export_values();
    py::enum_<target_property_type>(m, "target_property_type")
        .value("DISCHARGE", DISCHARGE)
        .value("SNOW_COVERED_AREA", SNOW_COVERED_AREA)
        .value("SNOW_WATER_EQUIVALENT", SNOW_WATER_EQUIVALENT)
        .value("ROUTED_DISCHARGE", ROUTED_DISCHARGE)
        .value("CELL_CHARGE", CELL_CHARGE)
        .export_values();
    py::class_<target_specification>(m, "_TargetSpecification")
        .def(py::init<>())
        .def_readwrite("ts", &target_specification::ts)
        .def_readwrite("catchment_indexes", &target_specification::catchment_indexes)
        .def_readwrite("river_id", &target_specification::river_id)
        .def_readwrite("scale_factor", &target_specification::scale_factor)
        .def_readwrite("calc_mode", &target_specification::calc_mode)
        .def_readwrite("catchment_property", &target_specification::catchment_property)
        .def_readwrite("s_r", &target_specification::s_r)
        .def_readwrite("s_a", &target_specification::s_a)
        .def_readwrite("s_b", &target_specification::s_b)
        .def_readwrite("uid", &target_specification::uid);
    // goal functions on value vectors (time_series.h:2301-2450), for tests and direct use
    m.def("nash_sutcliffe_goal_function", &goal::nash_sutcliffe, py::arg("observed"), py::arg("model"));
    m.def("kling_gupta_goal_function", &goal::kling_gupta, py::arg("observed"), py::arg("model"), py::arg("s_r"),
          py::arg("s_a"), py::arg("s_b"));
    m.def("rmse_goal_function", &goal::rmse, py::arg("observed"), py::arg("model"));
    m.def("abs_diff_sum_goal_function", &goal::abs_diff_sum, py::arg("observed"), py::arg("model"));
    m.def("abs_diff_sum_goal_function_scaled", &goal::abs_diff_sum_scaled, py::arg("observed"), py::arg("model"),
          py::arg("scale"));
    m.def("_average_onto", &average_onto);
    // search algorithms over a Python callable (scaled space [0,1]^n), for tests of the restatements
    m.def("_sceua_find_min", [](const std::function<double(const std::vector<double>&)>& f, std::vector<double> x,
                                size_t max_n, double x_eps, double y_eps) {
        const size_t n = x.size();
        std::vector<double> lo(n, 0.0), hi(n, 1.0), xe(n, x_eps);
        scaled_fx fx{f, [&f](const std::vector<std::vector<double>>& xs) {
                         std::vector<double> r;
                         for (const auto& v : xs) r.push_back(f(v));
                         return r;
                     }};
        double y = 0;
        auto st = sceua_search().find_min(lo, hi, x, y, fx, y_eps, -1.0, -2.0, xe, max_n, false);
        return std::make_tuple(x, y, int(st));
    });
    m.def("_dream_find_max", [](const std::function<double(const std::vector<double>&)>& f, std::vector<double> x,
                                size_t max_n) {
        scaled_fx fx{f, [&f](const std::vector<std::vector<double>>& xs) {
                         std::vector<double> r;
                         for (const auto& v : xs) r.push_back(f(v));
                         return r;
                     }};
        double y = dream_search().find_max(fx, x, max_n, false);
        return std::make_pair(x, y);
    });
    m.def("_box_trust_region_min", [](const std::function<double(const std::vector<double>&)>& f, std::vector<double> x,
                                      double rho_begin, double rho_end, size_t max_n) {
        scaled_fx fx{f, [&f](const std::vector<std::vector<double>>& xs) {
                         std::vector<double> r;
                         for (const auto& v : xs) r.push_back(f(v));
                         return r;
                     }};
        auto r = box_trust_region::minimize(fx, x, rho_begin, rho_end, max_n);
        return std::make_tuple(r.x, r.f, r.evaluations);
    });
    bind_optimizer<pt_gs_k_stack>(m, "_PTGSKOptimizer");
    bind_optimizer<hbv_stack_stack>(m, "_HbvOptimizer");
    bind_optimizer<pt_ss_k_stack>(m, "_PTSSKOptimizer");
    bind_optimizer<pt_hs_k_stack>(m, "_PTHSKOptimizer");
    bind_optimizer<pt_hps_k_stack>(m, "_PTHPSKOptimizer");

    py::register_exception_translator([](std::exception_ptr p) {
        try {
            if (p) std::rethrow_exception(p);
        } catch (const std::invalid_argument& e) {
            PyErr_SetString(PyExc_RuntimeError, e.what());
        }
    });
}
