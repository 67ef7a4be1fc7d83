"""ctypes binding of the C ABI in include/heat_amd.h.

``HeatBatch`` mirrors, at batch level, the reference's ``ThermalModel`` contract
(src/model.rs:188-428): ``HeatBatch(md)`` ≙ ``ThermalModel::new`` + ``allocate_memory``,
``HeatBatch.march(state, weather)`` ≙ ``ThermalModel::march``. Errors become ``HeatError``
(the reference returns ``Err(String)`` or panics).

The library is loaded from ``heat_amd/lib/libheat_amd.so``. If it is missing this module
raises: the HIP path is the only path.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_d = C.c_double
_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)


class HeatError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("heat_amd error %d: %s" % (code, message))
        self.code = code
        self.message = message


class Cavity(C.Structure):
    _fields_ = [("thickness", _d), ("height", _d), ("angle", _d), ("eout", _d), ("ein", _d),
                ("gas", C.c_int32), ("reserved", C.c_int32)]


CAVITY_DTYPE = np.dtype([("thickness", "f8"), ("height", "f8"), ("angle", "f8"), ("eout", "f8"),
                         ("ein", "f8"), ("gas", "i4"), ("reserved", "i4")])


class Weather(C.Structure):
    _fields_ = [("dry_bulb", _d), ("wind_direction", _d), ("wind_speed", _d)]


class Desc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("reserved", C.c_int32),
        ("n_surfaces", C.c_int64), ("n_zones", C.c_int64), ("n_cavities", C.c_int64), ("n_state", C.c_int64),
        ("dt", _d),
        ("node_offset", _i64p), ("mass", _dp), ("uvalue", _dp), ("seg_cavity", _i32p),
        ("front_alpha", _dp), ("back_alpha", _dp), ("cavities", C.POINTER(Cavity)),
        ("front_kind", _i32p), ("back_kind", _i32p), ("front_zone", _i32p), ("back_zone", _i32p),
        ("front_ambient", _dp), ("back_ambient", _dp), ("front_emissivity", _dp), ("back_emissivity", _dp),
        ("area", _dp), ("perimeter", _dp), ("cos_tilt", _dp), ("normal_x", _dp), ("normal_y", _dp),
        ("wind_modifier", _dp), ("front_hs_fix", _dp), ("back_hs_fix", _dp),
        ("first_node_slot", _i64p), ("hs_front_slot", _i64p), ("hs_back_slot", _i64p),
        ("flow_front_slot", _i64p), ("flow_back_slot", _i64p), ("solar_front_slot", _i64p),
        ("solar_back_slot", _i64p), ("ir_front_slot", _i64p), ("ir_back_slot", _i64p),
        ("zone_volume", _dp), ("zone_slot", _i64p),
    ]


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("force_general", C.c_int32), ("nodes_per_lane", C.c_int32),
                ("use_graph", C.c_int32), ("stream", C.c_void_p), ("n_ranks", C.c_int32), ("rank", C.c_int32),
                ("no_palette", C.c_int32), ("no_fusion", C.c_int32)]


class Series(C.Structure):
    """heat_series (include/heat_amd.h): the schedules, driven inputs and probes of a series march"""
    _fields_ = [("n_steps", C.c_int32), ("n_sub", C.c_int32), ("weather", C.POINTER(Weather)),
                ("n_zone_term_steps", C.c_int32), ("zone_a0", _dp), ("zone_b0", _dp),
                ("n_channels", C.c_int32), ("channel", _dp),
                ("solar_front_chan", _i32p), ("solar_back_chan", _i32p), ("ir_front_chan", _i32p), ("ir_back_chan", _i32p),
                ("solar_front_gain", _dp), ("solar_back_gain", _dp), ("ir_front_gain", _dp), ("ir_back_gain", _dp),
                ("ir_own_face", C.POINTER(C.c_uint8)), ("n_probes", C.c_int64), ("probe_slot", _i64p)]


class ZoneLoads(C.Structure):
    """heat_zone_loads (include/heat_amd.h): gains, air flows and thermostats a series forms on the device at every step"""
    _fields_ = [("n_gains", C.c_int64), ("gain_zone", _i32p), ("gain_chan", _i32p), ("gain_factor", _dp),
                ("n_flows", C.c_int64), ("flow_zone", _i32p), ("flow_volume_chan", _i32p), ("flow_temp_chan", _i32p),
                ("flow_volume_gain", _dp),
                ("n_thermostats", C.c_int64), ("th_sensor_zone", _i32p), ("th_target_zone", _i32p), ("th_heat_chan", _i32p),
                ("th_cool_chan", _i32p), ("th_heat_power", _dp), ("th_cool_power", _dp), ("th_band", _dp),
                ("th_mode", C.POINTER(C.c_uint8))]


class Report(C.Structure):
    """heat_series_report (include/heat_amd.h): statistics and weighted group sums a series maintains on the device"""
    _fields_ = [("resume", C.c_int32), ("step_base", C.c_int64),
                ("n_groups", C.c_int64), ("group_offset", _i64p), ("group_slot", _i64p), ("group_weight", _dp),
                ("group_trace", _dp),
                ("q_min", _dp), ("q_step_min", _i64p), ("q_max", _dp), ("q_step_max", _i64p), ("q_sum", _dp),
                ("q_lo", _dp), ("q_n_below", _i64p), ("q_deg_below", _dp),
                ("q_hi", _dp), ("q_n_above", _i64p), ("q_deg_above", _dp),
                ("th_steps_heating", _i64p), ("th_steps_cooling", _i64p), ("th_switches", _i64p),
                ("th_sum_heating", _dp), ("th_sum_cooling", _dp)]


class IdealLoads(C.Structure):
    """heat_ideal_loads (include/heat_amd.h): zones held at their setpoints in every sub-timestep, the power being the result"""
    _fields_ = [("n_loads", C.c_int64), ("zone", _i32p), ("heat_chan", _i32p), ("cool_chan", _i32p),
                ("heat_cap", _dp), ("cool_cap", _dp), ("resume", C.c_int32), ("step_base", C.c_int64),
                ("sum_heating", _dp), ("sum_cooling", _dp), ("peak_heating", _dp), ("step_peak_heating", _i64p),
                ("peak_cooling", _dp), ("step_peak_cooling", _i64p), ("n_sat_heating", _i64p), ("n_sat_cooling", _i64p)]


class SkyRecord(C.Structure):
    """heat_sky_record (include/heat_amd.h): the sun and sky of one site at one step, 64 bytes"""
    _fields_ = [("sun_x", _d), ("sun_y", _d), ("sun_z", _d), ("beam", _d), ("diffuse", _d), ("ground", _d), ("ir_sky", _d),
                ("ir_ground", _d)]


class Sky(C.Structure):
    """heat_sky (include/heat_amd.h): per-site records, per-surface normals and mode bytes of the sky of a series"""
    _fields_ = [("record", C.POINTER(SkyRecord)), ("normal_x", _dp), ("normal_y", _dp), ("normal_z", _dp),
                ("mode", C.POINTER(C.c_uint8))]


class SolarGains(C.Structure):
    """heat_solar_gains (include/heat_amd.h): the apertures (windows seen from the sky) and the entries (shares of an
    aperture's power that land on a receiving side) of the solar gains of a series"""
    _fields_ = [("n_apertures", C.c_int64), ("ap_surface", _i64p), ("ap_normal_x", _dp), ("ap_normal_y", _dp), ("ap_normal_z", _dp),
                ("ap_tau_coef", _dp), ("ap_tau_diffuse", _dp), ("ap_scale", _dp), ("ap_sum", _dp),
                ("n_entries", C.c_int64), ("en_surface", _i64p), ("en_side", C.POINTER(C.c_uint8)), ("en_aperture", _i32p),
                ("en_beam", _dp), ("en_diffuse", _dp)]


class AirPaths(C.Structure):
    """heat_air_paths (include/heat_amd.h): air that moves between zones, and vents controlled on both of their ends"""
    _fields_ = [("n_paths", C.c_int64), ("target", _i32p), ("source", _i32p), ("temp_chan", _i32p), ("volume_chan", _i32p),
                ("volume_gain", _dp), ("open_chan", _i32p), ("sense", C.POINTER(C.c_int8)), ("band", _dp), ("min_delta", _dp),
                ("state", C.POINTER(C.c_uint8)), ("sum_q", _dp), ("steps_open", _i64p), ("switches", _i64p)]


_SHADE_F64 = ("sh_normal_x", "sh_normal_y", "sh_normal_z", "sh_right_x", "sh_right_y", "sh_right_z", "sh_up_x", "sh_up_y", "sh_up_z",
              "sh_width", "sh_height", "overhang_depth", "overhang_gap", "fin_pos_depth", "fin_pos_gap", "fin_neg_depth", "fin_neg_gap",
              "diffuse_factor", "ground_factor")


class Shades(C.Structure):
    """heat_shades (include/heat_amd.h): overhangs, side fins and horizon profiles, and the sides and apertures they shade"""
    _fields_ = ([("n_shades", C.c_int64), ("sh_surface", _i64p)] + [(name, _dp) for name in _SHADE_F64] +
                [("sh_horizon", _i32p), ("n_horizons", C.c_int64), ("horizon_tan2", _dp), ("front_shade", _i32p),
                 ("back_shade", _i32p), ("aperture_shade", _i32p)])


class RoomRadiation(C.Structure):
    """heat_room_radiation (include/heat_amd.h): long-wave exchange among the faces of a room"""
    _fields_ = [("n_receivers", C.c_int64), ("rc_surface", _i64p), ("rc_side", C.POINTER(C.c_uint8)), ("sum_irradiance", _dp),
                ("n_entries", C.c_int64), ("en_receiver", _i64p), ("en_surface", _i64p), ("en_side", C.POINTER(C.c_uint8)),
                ("en_chan", _i32p), ("en_factor", _dp)]


class AmbientDrive(C.Structure):
    """heat_ambient_drive (include/heat_amd.h): ambient-side temperatures of a series, per step"""
    _fields_ = [("n_sides", C.c_int64), ("surface", _i64p), ("side", C.POINTER(C.c_uint8)), ("chan", _i32p), ("gain", _dp),
                ("offset", _dp), ("mix_zone", _i32p), ("mix", _dp), ("sum_temperature", _dp)]


class Blinds(C.Structure):
    """heat_blinds (include/heat_amd.h): movable solar protection that rides on shades, controlled or scheduled"""
    _fields_ = [("n_blinds", C.c_int64), ("shade", _i32p), ("beam_closed", _dp), ("diffuse_closed", _dp), ("ground_closed", _dp),
                ("pos_chan", _i32p), ("irr_close", _dp), ("irr_open", _dp), ("zone", _i32p), ("set_chan", _i32p), ("band", _dp),
                ("enable_chan", _i32p), ("state", C.POINTER(C.c_uint8)), ("steps_closed", _i64p), ("switches", _i64p),
                ("sum_position", _dp)]


class SkyCoef(C.Structure):
    """heat_sky_coef (include/heat_amd.h): the circumsolar fraction and the horizon coefficient of one site at one step, 16 bytes"""
    _fields_ = [("circ", _d), ("horiz", _d)]


class SkyAniso(C.Structure):
    """heat_sky_aniso (include/heat_amd.h): per-site coefficient pairs beside the sky records, and the consumers' bands"""
    _fields_ = [("coef", C.POINTER(SkyCoef)), ("front_band", _dp), ("back_band", _dp), ("aperture_band", _dp), ("shade_band", _dp)]


class SeriesCall(C.Structure):
    """heat_series_call (include/heat_amd.h): every term of a series march by name, for heat_batch_march_series_call"""
    _fields_ = [("size", C.c_size_t), ("s", C.POINTER(Series)), ("sky", C.POINTER(Sky)), ("aniso", C.POINTER(SkyAniso)),
                ("shades", C.POINTER(Shades)), ("gains", C.POINTER(SolarGains)), ("l", C.POINTER(ZoneLoads)),
                ("air", C.POINTER(AirPaths)), ("il", C.POINTER(IdealLoads)), ("r", C.POINTER(Report)),
                ("radiation", C.POINTER(RoomRadiation)), ("ambient", C.POINTER(AmbientDrive)), ("blinds", C.POINTER(Blinds)),
                ("trace", _dp), ("applied", _dp), ("ideal_q", _dp), ("transmitted", _dp), ("path_q", _dp), ("sunlit", _dp),
                ("irradiance", _dp), ("ambient_t", _dp), ("position", _dp), ("blind_incident", _dp), ("failed_step", _i32p)]


class Comfort(C.Structure):
    """heat_comfort (include/heat_amd.h): operative-temperature sensors of a series, their limits and accumulators"""
    _fields_ = [("n_sensors", C.c_int64), ("zone", _i32p), ("air_weight", _dp), ("control", C.POINTER(C.c_uint8)),
                ("n_entries", C.c_int64), ("en_sensor", _i32p), ("en_surface", _i64p), ("en_side", C.POINTER(C.c_uint8)),
                ("en_weight", _dp), ("occ_chan", _i32p), ("lo_chan", _i32p), ("hi_chan", _i32p), ("resume", C.c_int32),
                ("step_base", C.c_int64), ("n_occupied", _i64p), ("sum_operative", _dp), ("min_operative", _dp), ("step_min", _i64p),
                ("max_operative", _dp), ("step_max", _i64p), ("n_below", _i64p), ("deg_below", _dp), ("n_above", _i64p),
                ("deg_above", _dp), ("max_above", _dp), ("step_max_above", _i64p)]


class AirHandlers(C.Structure):
    """heat_air_handlers (include/heat_amd.h): ventilation units with heat recovery, a bypass and supply-air coils, and their
    branches into the zones"""
    _fields_ = [("n_units", C.c_int64), ("outdoor_chan", _i32p), ("eff_chan", _i32p), ("eff_gain", _dp), ("bypass_chan", _i32p),
                ("bypass_band", _dp), ("bypass_min_delta", _dp), ("heat_chan", _i32p), ("cool_chan", _i32p), ("heat_cap", _dp),
                ("cool_cap", _dp), ("n_branches", C.c_int64), ("br_unit", _i32p), ("br_zone", _i32p), ("br_volume_chan", _i32p),
                ("br_volume_gain", _dp), ("br_kind", C.POINTER(C.c_uint8)), ("bypass", C.POINTER(C.c_uint8)), ("sum_recovered", _dp),
                ("sum_heating", _dp), ("sum_cooling", _dp), ("steps_bypass", _i64p), ("switches", _i64p),
                ("steps_heat_saturated", _i64p), ("steps_cool_saturated", _i64p), ("sum_branch_q", _dp)]


class AirSpecies(C.Structure):
    """heat_air_species (include/heat_amd.h): concentrations per species and zone carried by the air a series moves, their
    sources and statistics, and demand vents whose volume flow follows a concentration"""
    _fields_ = [("n_species", C.c_int64), ("outdoor_chan", _i32p), ("n_sources", C.c_int64), ("src_zone", _i32p), ("src_species", _i32p),
                ("src_chan", _i32p), ("src_factor", _dp), ("n_vents", C.c_int64), ("vent_zone", _i32p), ("vent_species", _i32p),
                ("vent_temp_chan", _i32p), ("vent_enable_chan", _i32p), ("vent_v_min", _dp), ("vent_v_max", _dp), ("vent_c_lo", _dp),
                ("vent_c_hi", _dp), ("limit_chan", _i32p), ("occ_chan", _i32p), ("resume", C.c_int64), ("step_base", C.c_int64),
                ("conc", _dp), ("n_occupied", _i64p), ("sum_conc", _dp), ("max_conc", _dp), ("step_max", _i64p), ("n_above", _i64p),
                ("excess_above", _dp), ("sum_volume", _dp), ("sum_q", _dp), ("steps_saturated", _i64p)]


class Openings(C.Structure):
    """heat_openings (include/heat_amd.h): wind- and stack-driven volume flows through openings, written into derived channels"""
    _fields_ = [("n_openings", C.c_int64), ("zone_a", _i32p), ("zone_b", _i32p), ("temp_chan", _i32p), ("wind_chan", _i32p),
                ("frac_chan", _i32p), ("out_chan", _i32p), ("area", _dp), ("cw", _dp), ("cs", _dp), ("ca", _dp), ("c0", _dp),
                ("resume", C.c_int64), ("step_base", C.c_int64), ("sum_v", _dp), ("max_v", _dp), ("step_max", _i64p)]


class Controllers(C.Structure):
    """heat_controllers (include/heat_amd.h): modulating control loops whose outputs are written into derived channels"""
    _fields_ = [("n_controllers", C.c_int64), ("sense_kind", _i32p), ("sense_index", _i32p), ("sense_node", _i32p), ("set_chan", _i32p),
                ("action", _i32p), ("en_chan", _i32p), ("lim_kind", _i32p), ("lim_index", _i32p), ("lim_node", _i32p), ("out_chan", _i32p),
                ("kp", _dp), ("ki", _dp), ("bias", _dp), ("out_lo", _dp), ("out_hi", _dp), ("lim_hi", _dp), ("lim_lo", _dp),
                ("resume", C.c_int64), ("integral", _dp), ("tripped", C.POINTER(C.c_uint8)), ("sum_u", _dp), ("sum_out", _dp), ("steps_on", _i64p),
                ("steps_sat", _i64p), ("trips", _i64p)]


class AirNetworks(C.Structure):
    """heat_air_networks (include/heat_amd.h): pressure-balanced flows through the links of zone networks, written into derived channels"""
    _fields_ = [("n_networks", C.c_int64), ("n_nodes", C.c_int64), ("n_links", C.c_int64), ("net_offset", _i32p), ("tol", _dp),
                ("max_iter", _i32p), ("g_min", _dp), ("node_zone", _i32p), ("src_chan", _i32p), ("src_gain", _dp), ("zone_a", _i32p),
                ("zone_b", _i32p), ("temp_chan", _i32p), ("wp_chan", _i32p), ("frac_chan", _i32p), ("out_ab", _i32p), ("out_ba", _i32p),
                ("c", _dp), ("gh", _dp), ("p_lin", _dp), ("wp_gain", _dp), ("resume", C.c_int64), ("pressure", _dp), ("sum_ab", _dp),
                ("sum_ba", _dp), ("iters_sum", _i64p), ("unconverged", _i64p), ("max_res", _dp)]


class Layer(C.Structure):
    """heat_layer (include/heat_amd_setup.h)"""
    _fields_ = [("is_gas", C.c_int32), ("gas", C.c_int32), ("thickness", _d), ("conductivity", _d), ("density", _d),
                ("specific_heat", _d), ("front_thermal_absorbtance", _d), ("back_thermal_absorbtance", _d),
                ("solar_transmittance", _d), ("front_solar_absorbtance", _d), ("back_solar_absorbtance", _d)]


class SurfaceIn(C.Structure):
    """heat_surface_in (include/heat_amd_setup.h)"""
    _fields_ = [("layers", C.POINTER(Layer)), ("n_layers", C.c_int32), ("is_fenestration", C.c_int32),
                ("area", _d), ("perimeter", _d), ("normal", _d * 3), ("centroid_z", _d),
                ("front_kind", C.c_int32), ("back_kind", C.c_int32), ("front_zone", C.c_int32),
                ("back_zone", C.c_int32), ("front_ambient", _d), ("back_ambient", _d)]


# Every symbol include/heat_amd.h and include/heat_amd_setup.h declare: (name, restype, argtypes)
_H = C.c_void_p
SYMBOLS = [
    ("heat_batch_create", C.c_int, [C.POINTER(Desc), C.POINTER(_H)]),
    ("heat_batch_create_ex", C.c_int, [C.POINTER(Desc), C.POINTER(Options), C.POINTER(_H)]),
    ("heat_batch_create_sites", C.c_int, [C.POINTER(Desc), C.POINTER(Options), C.c_int32, _i32p, C.POINTER(_H)]),
    ("heat_batch_n_sites", C.c_int32, [_H]),
    ("heat_batch_destroy", None, [_H]),
    ("heat_batch_upload_state", C.c_int, [_H, _dp, C.c_size_t]),
    ("heat_batch_download_state", C.c_int, [_H, _dp, C.c_size_t]),
    ("heat_batch_upload_inputs", C.c_int, [_H, _dp, C.c_size_t]),
    ("heat_batch_march", C.c_int, [_H, _dp, C.c_size_t, C.POINTER(Weather), C.c_int32, _dp, _dp]),
    ("heat_batch_march_ex", C.c_int, [_H, _dp, C.c_size_t, C.POINTER(Weather), C.c_int32, _dp, _dp, C.c_int32]),
    ("heat_batch_download_outputs", C.c_int, [_H, _dp, C.c_size_t, C.c_int32]),
    ("heat_batch_march_resident", C.c_int, [_H, C.POINTER(Weather), C.c_int32, _dp, _dp]),
    ("heat_batch_synchronize", C.c_int, [_H]),
    ("heat_batch_failed_surface", C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("heat_series_check", C.c_int, [C.POINTER(Desc), C.c_int32, C.POINTER(Series)]),
    ("heat_batch_march_series", C.c_int, [_H, C.POINTER(Series), _dp, _i32p]),
    ("heat_zone_loads_check", C.c_int, [C.POINTER(Desc), C.POINTER(Series), C.POINTER(ZoneLoads)]),
    ("heat_batch_march_series_loads", C.c_int, [_H, C.POINTER(Series), C.POINTER(ZoneLoads), _dp, _dp, _i32p]),
    ("heat_series_report_check", C.c_int, [C.POINTER(Desc), C.POINTER(Series), C.POINTER(ZoneLoads), C.POINTER(Report)]),
    ("heat_batch_march_series_report", C.c_int, [_H, C.POINTER(Series), C.POINTER(ZoneLoads), C.POINTER(Report), _dp, _dp, _i32p]),
    ("heat_ideal_loads_check", C.c_int, [C.POINTER(Desc), C.POINTER(Series), C.POINTER(IdealLoads)]),
    ("heat_batch_march_series_ideal", C.c_int, [_H, C.POINTER(Series), C.POINTER(ZoneLoads), C.POINTER(IdealLoads), C.POINTER(Report),
                                                _dp, _dp, _dp, _i32p]),
    ("heat_sky_check", C.c_int, [C.POINTER(Desc), C.c_int32, C.POINTER(Series), C.POINTER(Sky)]),
    ("heat_batch_march_series_sky", C.c_int, [_H, C.POINTER(Series), C.POINTER(Sky), C.POINTER(ZoneLoads), C.POINTER(IdealLoads),
                                              C.POINTER(Report), _dp, _dp, _dp, _i32p]),
    ("heat_solar_gains_check", C.c_int, [C.POINTER(Desc), C.c_int32, C.POINTER(Series), C.POINTER(Sky), C.POINTER(SolarGains)]),
    ("heat_batch_march_series_gains", C.c_int, [_H, C.POINTER(Series), C.POINTER(Sky), C.POINTER(SolarGains), C.POINTER(ZoneLoads),
                                                C.POINTER(IdealLoads), C.POINTER(Report), _dp, _dp, _dp, _dp, _i32p]),
    ("heat_air_paths_check", C.c_int, [C.POINTER(Desc), C.c_int32, C.POINTER(Series), C.POINTER(AirPaths)]),
    ("heat_batch_march_series_air", C.c_int, [_H, C.POINTER(Series), C.POINTER(Sky), C.POINTER(SolarGains), C.POINTER(ZoneLoads),
                                              C.POINTER(AirPaths), C.POINTER(IdealLoads), C.POINTER(Report), _dp, _dp, _dp, _dp, _dp,
                                              _i32p]),
    ("heat_shades_check", C.c_int, [C.POINTER(Desc), C.c_int32, C.POINTER(Series), C.POINTER(Sky), C.POINTER(SolarGains),
                                    C.POINTER(Shades)]),
    ("heat_batch_march_series_shaded", C.c_int, [_H, C.POINTER(Series), C.POINTER(Sky), C.POINTER(Shades), C.POINTER(SolarGains),
                                                 C.POINTER(ZoneLoads), C.POINTER(AirPaths), C.POINTER(IdealLoads), C.POINTER(Report),
                                                 _dp, _dp, _dp, _dp, _dp, _dp, _i32p]),
    ("heat_room_radiation_check", C.c_int, [C.POINTER(Desc), C.c_int32, C.POINTER(Series), C.POINTER(Sky), C.POINTER(RoomRadiation)]),
    ("heat_batch_march_series_radiation", C.c_int, [_H, C.POINTER(Series), C.POINTER(Sky), C.POINTER(Shades), C.POINTER(SolarGains),
                                                    C.POINTER(ZoneLoads), C.POINTER(AirPaths), C.POINTER(IdealLoads),
                                                    C.POINTER(Report), _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(RoomRadiation), _dp,
                                                    _i32p]),
    ("heat_batch_set_ambient", C.c_int, [_H, C.c_int64, _i64p, C.POINTER(C.c_uint8), _dp]),
    ("heat_ambient_check", C.c_int, [C.POINTER(Desc), C.c_int32, C.POINTER(Series), C.POINTER(AmbientDrive)]),
    ("heat_batch_march_series_ambient", C.c_int, [_H, C.POINTER(Series), C.POINTER(Sky), C.POINTER(Shades), C.POINTER(SolarGains),
                                                  C.POINTER(ZoneLoads), C.POINTER(AirPaths), C.POINTER(IdealLoads),
                                                  C.POINTER(Report), _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(RoomRadiation), _dp,
                                                  C.POINTER(AmbientDrive), _dp, _i32p]),
    ("heat_blinds_check", C.c_int, [C.POINTER(Desc), C.c_int32, C.POINTER(Series), C.POINTER(Sky), C.POINTER(SolarGains),
                                    C.POINTER(Shades), C.POINTER(Blinds)]),
    ("heat_batch_march_series_blinds", C.c_int, [_H, C.POINTER(Series), C.POINTER(Sky), C.POINTER(Shades), C.POINTER(SolarGains),
                                                 C.POINTER(ZoneLoads), C.POINTER(AirPaths), C.POINTER(IdealLoads),
                                                 C.POINTER(Report), _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(RoomRadiation), _dp,
                                                 C.POINTER(AmbientDrive), _dp, C.POINTER(Blinds), _dp, _dp, _i32p]),
    ("heat_sky_aniso_check", C.c_int, [C.POINTER(Desc), C.c_int32, C.POINTER(Series), C.POINTER(Sky), C.POINTER(SolarGains),
                                       C.POINTER(Shades), C.POINTER(SkyAniso)]),
    ("heat_batch_march_series_call", C.c_int, [_H, C.POINTER(SeriesCall)]),
    ("heat_comfort_check", C.c_int, [C.POINTER(Desc), C.POINTER(Series), C.POINTER(Comfort)]),
    ("heat_batch_march_series_comfort", C.c_int, [_H, C.POINTER(SeriesCall), C.POINTER(Comfort), _dp, _dp]),
    ("heat_air_handlers_check", C.c_int, [C.POINTER(Desc), C.POINTER(Series), C.POINTER(AirHandlers)]),
    ("heat_batch_march_series_handlers", C.c_int, [_H, C.POINTER(SeriesCall), C.POINTER(Comfort), _dp, _dp, C.POINTER(AirHandlers),
                                                   _dp, _dp, _dp, _dp]),
    ("heat_air_species_check", C.c_int, [C.POINTER(Desc), C.POINTER(Series), C.POINTER(ZoneLoads), C.POINTER(AirPaths),
                                         C.POINTER(AirHandlers), C.POINTER(AirSpecies)]),
    ("heat_batch_march_series_species", C.c_int, [_H, C.POINTER(SeriesCall), C.POINTER(Comfort), _dp, _dp, C.POINTER(AirHandlers),
                                                  _dp, _dp, _dp, _dp, C.POINTER(AirSpecies), _dp, _dp, _dp]),
    ("heat_openings_check", C.c_int, [C.POINTER(Desc), C.POINTER(Series), C.POINTER(Openings)]),
    ("heat_batch_march_series_openings", C.c_int, [_H, C.POINTER(SeriesCall), C.POINTER(Comfort), _dp, _dp, C.POINTER(AirHandlers),
                                                   _dp, _dp, _dp, _dp, C.POINTER(AirSpecies), _dp, _dp, _dp, C.POINTER(Openings), _dp]),
    ("heat_controllers_check", C.c_int, [C.POINTER(Desc), C.POINTER(Series), C.POINTER(Openings), C.POINTER(Controllers)]),
    ("heat_batch_march_series_controllers", C.c_int, [_H, C.POINTER(SeriesCall), C.POINTER(Comfort), _dp, _dp, C.POINTER(AirHandlers),
                                                      _dp, _dp, _dp, _dp, C.POINTER(AirSpecies), _dp, _dp, _dp, C.POINTER(Openings), _dp,
                                                      C.POINTER(Controllers), _dp, _dp]),
    ("heat_air_networks_check", C.c_int, [C.POINTER(Desc), C.POINTER(Series), C.POINTER(Openings), C.POINTER(Controllers),
                                          C.POINTER(AirNetworks)]),
    ("heat_batch_march_series_networks", C.c_int, [_H, C.POINTER(SeriesCall), C.POINTER(Comfort), _dp, _dp, C.POINTER(AirHandlers),
                                                   _dp, _dp, _dp, _dp, C.POINTER(AirSpecies), _dp, _dp, _dp, C.POINTER(Openings), _dp,
                                                   C.POINTER(Controllers), _dp, _dp, C.POINTER(AirNetworks), _dp, _dp, _i32p]),
    ("heat_batch_set_weather", C.c_int, [_H, C.POINTER(Weather), C.c_int32, _dp, _dp]),
    ("heat_batch_step_surfaces", C.c_int, [_H, C.c_int32]),
    ("heat_batch_step_zones", C.c_int, [_H, C.c_void_p, C.c_int32]),
    ("heat_batch_zone_partials", C.c_void_p, [_H]),
    ("heat_batch_use_partials", C.c_int, [_H, C.c_void_p]),
    ("heat_batch_touched_zones", C.c_int, [_H, C.POINTER(C.c_uint8)]),
    ("heat_batch_set_shared_zones", C.c_int, [_H, _i32p, C.c_int32]),
    ("heat_comm_available", C.c_int, []),
    ("heat_comm_unique_id", C.c_int, [C.POINTER(C.c_uint8)]),
    ("heat_batch_comm_init", C.c_int, [_H, C.POINTER(C.c_uint8)]),
    ("heat_batch_comm_init_ex", C.c_int, [_H, C.POINTER(C.c_uint8), _i32p, C.c_int32]),
    ("heat_batch_set_owned_zones", C.c_int, [_H, C.POINTER(C.c_uint8)]),
    ("heat_batch_n_shared_zones", C.c_int32, [_H]),
    ("heat_batch_comm_ranks", C.c_int32, [_H]),
    ("heat_batch_comm_destroy", C.c_int, [_H]),
    ("heat_batch_set_fusion", C.c_int, [_H, C.c_int32]),
    ("heat_batch_n_fused_surfaces", C.c_int64, [_H]),
    ("heat_batch_n_fused_launches", C.c_int64, [_H]),
    ("heat_batch_set_ideal_resident", C.c_int, [_H, C.c_int32]),
    ("heat_batch_ideal_resident", C.c_int32, [_H]),
    ("heat_batch_n_surfaces", C.c_int64, [_H]),
    ("heat_batch_n_nodes", C.c_int64, [_H]),
    ("heat_batch_n_zones", C.c_int64, [_H]),
    ("heat_batch_algorithmic_bytes", C.c_int64, [_H]),
    ("heat_batch_nomass_iterations", C.c_int64, [_H]),
    ("heat_batch_class_counts", C.c_int, [_H, _i64p]),
    ("heat_batch_set_timing", C.c_int, [_H, C.c_int32]),
    ("heat_batch_get_timing", C.c_int, [_H, _dp, _dp, _i64p]),
    ("heat_partition", C.c_int, [C.POINTER(Desc), C.c_int32, _i32p, _i64p]),
    ("heat_batch_create_shard", C.c_int, [C.POINTER(Desc), C.POINTER(Options), _i32p, C.POINTER(_H)]),
    ("heat_plan_check", C.c_int, [C.POINTER(Desc), C.POINTER(Options), _i64p]),
    ("heat_plan_check_sites", C.c_int, [C.POINTER(Desc), C.POINTER(Options), C.c_int32, _i32p, _i64p]),
    ("heat_plan_ideal_resident", C.c_int, [C.POINTER(Desc), C.POINTER(Options), C.c_int32, _i32p, _i32p]),
    ("heat_last_error", C.c_char_p, []),
    ("heat_amd_abi_version", C.c_int, []),
    # include/heat_amd_setup.h
    ("heat_discretize_construction", C.c_int, [C.c_int32, C.POINTER(Layer), _d, _d, _d, _i32p]),
    ("heat_count_nodes", C.c_int32, [C.c_int32, _i32p]),
    ("heat_build_segments", C.c_int, [C.c_int32, C.POINTER(Layer), _i32p, _d, _d, _dp, _dp, _i32p,
                                      C.POINTER(Cavity), C.c_int32]),
    ("heat_get_chunks", C.c_int, [C.c_int32, _dp, _i32p, _i32p, _i32p, _i32p]),
    ("heat_glazing_alphas", C.c_int, [C.c_int32, _dp, _dp, _dp, _dp]),
    ("heat_node_alphas", C.c_int, [C.c_int32, C.POINTER(Layer), _i32p, C.c_int32, _dp, _dp]),
    ("heat_wind_speed_modifier", _d, [_d, C.c_int32]),
    ("heat_model_builder_create", C.c_void_p, [C.c_int32, C.c_int32]),
    ("heat_model_builder_destroy", None, [C.c_void_p]),
    ("heat_model_builder_add_zone", C.c_int, [C.c_void_p, _d]),
    ("heat_model_builder_add_surface", C.c_int, [C.c_void_p, C.POINTER(SurfaceIn)]),
    ("heat_model_builder_finish", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(Desc)), C.POINTER(_dp), _i32p]),
    ("heat_model_builder_surface_info", C.c_int, [C.c_void_p, C.c_int64, _i32p, _i32p, _i32p, C.c_int32]),
]

_lib = None


def lib_path():
    # HEAT_AMD_LIB: another build of the same sources (measurement variants); the default is the in-tree library
    return os.environ.get("HEAT_AMD_LIB") or _build.LIB


def build_library(force=False):
    return _build.build(force=force)


def load_library():
    """Loads libheat_amd.so and binds every declared symbol. Raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            "heat_amd: %s is missing. Build it with `python -m heat_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback." % path)
    L = C.CDLL(path)
    for name, res, args in SYMBOLS:
        f = getattr(L, name)  # AttributeError if the library does not export it
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise HeatError(rc, load_library().heat_last_error().decode("utf-8", "replace"))


def as_weather(weather, n_sites=1):
    """[n,3] array (dry bulb C, wind direction RADIANS, wind speed m/s) -> (ctypes array, n). A batch of weather sites
    takes exactly [n_sub, n_sites, 3] (record [k, s]: site s at sub-timestep k) -> (ctypes array, n_sub); a batch of one
    site takes [n, 3] or [n, 1, 3]."""
    w = np.ascontiguousarray(weather, dtype=np.float64)
    if n_sites > 1 and (w.ndim != 3 or w.shape[1:] != (n_sites, 3)):
        raise ValueError("a batch of %d weather sites takes weather [n_sub, %d, 3], not %s" % (n_sites, n_sites, w.shape))
    if n_sites == 1 and w.ndim == 3 and w.shape[1] != 1:
        raise ValueError("weather of %d sites for a batch of one" % w.shape[1])
    w = w.reshape(-1, 3)
    arr = (Weather * len(w))()
    if len(w):
        C.memmove(arr, w.ctypes.data, w.nbytes)
    return arr, len(w) // n_sites


_F64 = ["mass", "uvalue", "front_alpha", "back_alpha", "front_ambient", "back_ambient", "front_emissivity",
        "back_emissivity", "area", "perimeter", "cos_tilt", "normal_x", "normal_y", "wind_modifier", "zone_volume"]
_I32 = ["front_kind", "back_kind", "front_zone", "back_zone"]
_I64 = ["node_offset", "first_node_slot", "hs_front_slot", "hs_back_slot", "flow_front_slot", "flow_back_slot",
        "solar_front_slot", "solar_back_slot", "ir_front_slot", "ir_back_slot", "zone_slot"]


def make_desc(md):
    """Builds a heat_batch_desc from the model dict (heat_amd.modeldict). Returns (desc, keepalive)."""
    keep = {}
    d = Desc()
    d.abi_version = 1
    d.n_surfaces = int(md["n_surfaces"])
    d.n_zones = int(md["n_zones"])
    d.n_state = int(md["n_state"])
    d.dt = float(md["dt"])
    for k in _F64:
        a = np.ascontiguousarray(md[k], dtype=np.float64)
        keep[k] = a
        setattr(d, k, a.ctypes.data_as(_dp))
    for k in _I32:
        a = np.ascontiguousarray(md[k], dtype=np.int32)
        keep[k] = a
        setattr(d, k, a.ctypes.data_as(_i32p))
    for k in _I64:
        a = np.ascontiguousarray(md[k], dtype=np.int64)
        keep[k] = a
        setattr(d, k, a.ctypes.data_as(_i64p))
    if md.get("front_hs_fix") is not None:
        for k in ("front_hs_fix", "back_hs_fix"):
            a = np.ascontiguousarray(md[k], dtype=np.float64)
            keep[k] = a
            setattr(d, k, a.ctypes.data_as(_dp))
    cav = md.get("cavities")
    if cav is not None and len(cav) and md.get("seg_cavity") is not None:
        sc = np.ascontiguousarray(md["seg_cavity"], dtype=np.int32)
        cv = np.zeros(len(cav), dtype=CAVITY_DTYPE)
        for f in ("thickness", "height", "angle", "eout", "ein", "gas"):
            cv[f] = cav[f]
        keep["seg_cavity"] = sc
        keep["cavities"] = cv
        d.seg_cavity = sc.ctypes.data_as(_i32p)
        d.cavities = cv.ctypes.data_as(C.POINTER(Cavity))
        d.n_cavities = len(cv)
    return d, keep


HOST_ONLY_SYMBOLS = ("heat_partition", "heat_plan_check", "heat_plan_check_sites", "heat_plan_ideal_resident", "heat_series_check",
                     "heat_zone_loads_check",
                     "heat_series_report_check", "heat_ideal_loads_check", "heat_sky_check", "heat_solar_gains_check",
                     "heat_air_paths_check", "heat_shades_check", "heat_room_radiation_check", "heat_ambient_check",
                     "heat_blinds_check", "heat_sky_aniso_check", "heat_comfort_check", "heat_air_handlers_check",
                     "heat_air_species_check", "heat_openings_check", "heat_controllers_check", "heat_air_networks_check",
                     "heat_last_error", "heat_amd_abi_version")


def load_host_library(path):
    """Binds the host-only entry points (csrc/plan.cpp) of a library built without HIP: the sanitizer build of the
    planner that tests/test_planner_host.py runs in a child process."""
    L = C.CDLL(path)
    for name, res, args in SYMBOLS:
        if name in HOST_ONLY_SYMBOLS:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
    return L


def make_options(device=-1, force_general=False, nodes_per_lane=0, use_graph=False, stream=None, n_ranks=1, rank=0,
                 no_palette=False, no_fusion=False, fuse_always=False):
    opt = Options()
    opt.device = device
    opt.force_general = 1 if force_general else 0
    opt.nodes_per_lane = nodes_per_lane
    opt.use_graph = 1 if use_graph else 0
    opt.stream = stream
    opt.n_ranks = n_ranks
    opt.rank = rank
    opt.no_palette = 1 if no_palette else 0
    opt.no_fusion = 1 if no_fusion else (2 if fuse_always else 0)
    return opt


def partition(md, n_ranks, lib=None):
    """heat_partition: (rank of every surface, number of zones shared between ranks). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    ranks = np.zeros(int(md["n_surfaces"]), dtype=np.int32)
    n_shared = C.c_int64(0)
    rc = L.heat_partition(C.byref(desc), n_ranks, ranks.ctypes.data_as(_i32p), C.byref(n_shared))
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))
    return ranks, int(n_shared.value)


def plan_check(md, lib=None, **opts):
    """heat_plan_check: plans the model as heat_batch_create_ex would and verifies the plan. Returns the summary
    (surfaces per class [5], fused surfaces, fused workgroups, tiles). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    opt = make_options(**opts)
    summary = (C.c_int64 * 8)()
    rc = L.heat_plan_check(C.byref(desc), C.byref(opt), summary)
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))
    return list(summary)


def plan_check_sites(md, n_sites, site_of_surface, lib=None, **opts):
    """heat_plan_check_sites: plan_check for a batch of weather sites (also verifies that every tile, fused workgroup
    and team holds one site). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    opt = make_options(**opts)
    sites = np.ascontiguousarray(site_of_surface, dtype=np.int32)
    summary = (C.c_int64 * 8)()
    rc = L.heat_plan_check_sites(C.byref(desc), C.byref(opt), int(n_sites), sites.ctypes.data_as(_i32p), summary)
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))
    return list(summary)


# heat_ideal_resident_reason (include/heat_amd.h): why a batch's ideal series cannot keep its resident clusters resident
IDEAL_RESIDENT_OK, IDEAL_RESIDENT_NONE_PLANNED, IDEAL_RESIDENT_TEAMS, IDEAL_RESIDENT_CAVITY_CLASS, IDEAL_RESIDENT_CHUNK_LOOP_CLASS = range(5)


def plan_ideal_resident(md, n_sites=1, site_of_surface=None, lib=None, **opts):
    """heat_plan_ideal_resident: (eligible, reason) — whether an ideal series of a batch made from this model and these
    options could keep its resident clusters resident (HeatBatch.set_ideal_resident), and if not why (IDEAL_RESIDENT_*).
    Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    opt = make_options(**opts)
    sites = None if site_of_surface is None else np.ascontiguousarray(site_of_surface, dtype=np.int32)
    reason = C.c_int32(-1)
    rc = L.heat_plan_ideal_resident(C.byref(desc), C.byref(opt), int(n_sites),
                                    sites.ctypes.data_as(_i32p) if sites is not None else None, C.byref(reason))
    if rc < 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))
    return bool(rc), int(reason.value)


def make_series(weather, n_sub, n_sites=1, channel=None, solar_front=None, solar_back=None, ir_front=None, ir_back=None,
                ir_own_face=None, zone_a0=None, zone_b0=None, probes=None, n_steps=None):
    """Builds a heat_series. Returns (series, keepalive).
    weather: n_steps * n_sub records of (dry bulb C, wind direction RADIANS, wind speed m/s), step-major — any shape
    [..., 3] (one site) or [..., n_sites, 3], e.g. [n_steps, n_sub, 3]; n_steps is its length over n_sub (with
    n_sub == 0: ``n_steps``, or the rows of ``channel``).
    channel [n_steps, n_channels]; solar_front / solar_back / ir_front / ir_back: a channel number per surface (-1: not
    driven), or a pair (channel numbers, gains); ir_own_face: bits per surface; zone_a0 / zone_b0: [n_zones] (one row for
    every step) or [n_steps, n_zones]; probes: state slots."""
    keep = {}
    s = Series()
    n_sub = int(n_sub)
    w = np.ascontiguousarray(weather if weather is not None else np.zeros((0, 3)), dtype=np.float64)
    if w.ndim < 2 or w.shape[-1] != 3:
        raise ValueError("weather records are (dry bulb, wind direction, wind speed), not %s" % (w.shape,))
    if n_sites > 1 and (w.ndim < 3 or w.shape[-2] != n_sites):
        raise ValueError("a series of %d weather sites takes weather [..., %d, 3], not %s" % (n_sites, n_sites, w.shape))
    if n_sites == 1 and w.ndim > 3 and w.shape[-2] != 1:
        raise ValueError("weather of %d sites for a batch of one" % w.shape[-2])
    records = w.size // 3
    ch = None if channel is None else np.ascontiguousarray(channel, dtype=np.float64)
    if ch is not None and ch.ndim != 2:
        raise ValueError("channel is [n_steps, n_channels], not %s" % (ch.shape,))
    if n_sub > 0:
        if records % (n_sub * n_sites):
            raise ValueError("%d weather records are no whole number of steps of %d x %d" % (records, n_sub, n_sites))
        steps = records // (n_sub * n_sites)
        if n_steps is not None and int(n_steps) != steps:
            raise ValueError("weather of %d steps, n_steps = %d" % (steps, n_steps))
    else:
        steps = int(n_steps) if n_steps is not None else (len(ch) if ch is not None else 0)
    if ch is not None and len(ch) != steps:
        raise ValueError("channel of %d rows for %d steps" % (len(ch), steps))
    s.n_steps, s.n_sub = steps, n_sub
    keep["weather"] = w
    s.weather = C.cast(w.ctypes.data, C.POINTER(Weather)) if w.size else None
    rows = {}
    for name, a in (("zone_a0", zone_a0), ("zone_b0", zone_b0)):
        if a is None:
            continue
        a = np.ascontiguousarray(a, dtype=np.float64)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        rows[name] = len(a)
        keep[name] = a
        setattr(s, name, a.ctypes.data_as(_dp))
    if len(set(rows.values())) > 1:
        raise ValueError("zone_a0 and zone_b0 of different numbers of rows: %s" % rows)
    s.n_zone_term_steps = next(iter(rows.values())) if rows else 0
    if ch is not None:
        keep["channel"] = ch
        s.n_channels = ch.shape[1]
        s.channel = ch.ctypes.data_as(_dp)
    for name, v in (("solar_front", solar_front), ("solar_back", solar_back), ("ir_front", ir_front), ("ir_back", ir_back)):
        if v is None:
            continue
        chan, gain = v if isinstance(v, tuple) else (v, None)
        chan = np.ascontiguousarray(chan, dtype=np.int32)
        keep[name + "_chan"] = chan
        setattr(s, name + "_chan", chan.ctypes.data_as(_i32p))
        if gain is not None:
            gain = np.ascontiguousarray(gain, dtype=np.float64)
            if gain.shape != chan.shape:
                raise ValueError("%s: %d channel numbers, %d gains" % (name, chan.size, gain.size))
            keep[name + "_gain"] = gain
            setattr(s, name + "_gain", gain.ctypes.data_as(_dp))
    if ir_own_face is not None:
        own = np.ascontiguousarray(ir_own_face, dtype=np.uint8)
        keep["ir_own_face"] = own
        s.ir_own_face = own.ctypes.data_as(C.POINTER(C.c_uint8))
    pr = np.ascontiguousarray(probes if probes is not None else [], dtype=np.int64).reshape(-1)
    keep["probe_slot"] = pr
    s.n_probes = len(pr)
    s.probe_slot = pr.ctypes.data_as(_i64p) if len(pr) else None
    return s, keep


def _series_arrays_fit(keep, n_surfaces):
    for k, a in keep.items():
        if (k.endswith("_chan") or k.endswith("_gain") or k == "ir_own_face") and a.shape != (n_surfaces,):
            raise ValueError("%s: %s for %d surfaces" % (k, a.shape, n_surfaces))


def series_check(md, n_sites=1, lib=None, **series):
    """heat_series_check: everything about a series that needs no device (arguments as HeatBatch.march_series). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(n_sites=n_sites, **series)
    _series_arrays_fit(skeep, int(md["n_surfaces"]))
    for k in ("zone_a0", "zone_b0"):
        if k in skeep and skeep[k].shape[1] != int(md["n_zones"]):
            raise ValueError("%s: rows of %d for %d zones" % (k, skeep[k].shape[1], int(md["n_zones"])))
    rc = L.heat_series_check(C.byref(desc), int(n_sites), C.byref(s))
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


_GAIN_KEYS = ("zone", "chan", "factor")
_FLOW_KEYS = ("zone", "volume_chan", "temp_chan", "volume_gain")
_TH_KEYS = ("sensor_zone", "target_zone", "heat_chan", "cool_chan", "heat_power", "cool_power", "band", "mode")


def make_zone_loads(gains=None, flows=None, thermostats=None):
    """Builds a heat_zone_loads. Returns (loads, keepalive). Each group is a dict of equally long arrays (or a tuple in
    the order of the keys):
    gains        zone, chan, factor (optional: 1)
    flows        zone, volume_chan, temp_chan, volume_gain (optional: 1)
    thermostats  sensor_zone, target_zone, heat_chan, cool_chan (-1: none), heat_power, cool_power, band,
                 mode (optional: all off). keepalive["th_mode"] is the array the march updates in place."""
    keep = {}
    l = ZoneLoads()

    def group(v, keys, what):
        if v is None:
            return {}
        if not isinstance(v, dict):
            v = dict(zip(keys, v))
        unknown = set(v) - set(keys)
        if unknown:
            raise ValueError("%s: unknown %s (known: %s)" % (what, sorted(unknown), ", ".join(keys)))
        return {k: a for k, a in v.items() if a is not None}

    def put(prefix, g, keys, n_optional, what):
        n = None
        for i, k in enumerate(keys):
            if k not in g:
                if i < len(keys) - n_optional and g:
                    raise ValueError("%s: %s is missing" % (what, k))
                continue
            dtype = np.uint8 if k == "mode" else (np.int32 if k.endswith("zone") or k.endswith("chan") else np.float64)
            a = np.atleast_1d(np.array(g[k], dtype=dtype))  # (a copy: the mode bytes are written by the march)
            if a.ndim != 1 or (n is not None and len(a) != n):
                raise ValueError("%s: %s of shape %s, %s terms" % (what, k, a.shape, n))
            n = len(a)
            keep[prefix + k] = a
            setattr(l, prefix + k, a.ctypes.data_as({np.uint8: C.POINTER(C.c_uint8), np.int32: _i32p, np.float64: _dp}[dtype]))
        return n or 0

    l.n_gains = put("gain_", group(gains, _GAIN_KEYS, "gains"), _GAIN_KEYS, 1, "gains")
    l.n_flows = put("flow_", group(flows, _FLOW_KEYS, "flows"), _FLOW_KEYS, 1, "flows")
    th = group(thermostats, _TH_KEYS, "thermostats")
    if th and "mode" not in th:
        th["mode"] = np.zeros(len(np.atleast_1d(th["sensor_zone"])) if "sensor_zone" in th else 0, np.uint8)
    l.n_thermostats = put("th_", th, _TH_KEYS, 1, "thermostats")
    return l, keep


def zone_loads_check(md, loads=None, lib=None, **series):
    """heat_zone_loads_check: everything about the zone loads of a series that needs no device (series arguments as
    HeatBatch.march_series; loads: the arguments of make_zone_loads). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(**series)
    l, lkeep = make_zone_loads(**(loads or {}))
    rc = L.heat_zone_loads_check(C.byref(desc), C.byref(s), C.byref(l))
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


Q_STATS = ("min", "step_min", "max", "step_max", "sum", "n_below", "deg_below", "n_above", "deg_above")
TH_STATS = ("steps_heating", "steps_cooling", "switches", "sum_heating", "sum_cooling")
_INT_STATS = ("step_min", "step_max", "n_below", "n_above", "steps_heating", "steps_cooling", "switches")


def make_report(n_probes=0, n_thermostats=0, n_steps=0, groups=None, stats=None, limits=None, thermostat_stats=None,
                group_trace=False, resume=None, step_base=0):
    """Builds a heat_series_report. Returns (report, keepalive); the march updates the arrays of keepalive in place.
    groups            a list of groups, each an array of state slots or a pair (slots, weights) — or a dict with offset,
                      slot and (optional) weight in CSR form
    stats             names out of Q_STATS: which statistics of the Q = n_probes + n_groups quantities are maintained
    limits            dict(lo=[Q], hi=[Q]): the limits of n_below / deg_below and n_above / deg_above (NaN: never)
    thermostat_stats  names out of TH_STATS
    group_trace       True: keepalive["group_trace"] [n_steps, n_groups] is recorded
    resume            a dict of arrays a previous report returned (keys as in keepalive): the accumulators start from them
    step_base         the number the first step of this series has in q_step_min / q_step_max"""
    keep = {}
    r = Report()
    r.step_base = int(step_base)
    n_groups = 0
    if groups is not None:
        if isinstance(groups, dict):
            off = np.ascontiguousarray(groups["offset"], dtype=np.int64)
            slot = np.ascontiguousarray(groups["slot"], dtype=np.int64)
            weight = groups.get("weight")
            weight = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
        else:
            parts = [g if isinstance(g, tuple) else (g, None) for g in groups]
            slots = [np.asarray(g[0], dtype=np.int64).reshape(-1) for g in parts]
            off = np.concatenate([[0], np.cumsum([len(x) for x in slots])]).astype(np.int64)
            slot = np.concatenate(slots).astype(np.int64) if slots else np.zeros(0, np.int64)
            weight = None
            if any(g[1] is not None for g in parts):
                weight = np.concatenate([np.ones(len(x)) if g[1] is None else np.asarray(g[1], dtype=np.float64).reshape(-1)
                                         for x, g in zip(slots, parts)]) if slots else np.zeros(0)
        if weight is not None and weight.shape != slot.shape:
            raise ValueError("groups: %d slots, %d weights" % (slot.size, weight.size))
        n_groups = len(off) - 1
        if n_groups < 0 or (n_groups > 0 and off[-1] != len(slot)):
            raise ValueError("groups: offsets end at %s for %d slots" % (off[-1:] if len(off) else "nothing", len(slot)))
        keep["group_offset"], keep["group_slot"] = off, slot
        r.n_groups = n_groups
        r.group_offset = off.ctypes.data_as(_i64p) if n_groups > 0 else None
        r.group_slot = slot.ctypes.data_as(_i64p) if len(slot) else None
        if weight is not None:
            keep["group_weight"] = weight
            r.group_weight = weight.ctypes.data_as(_dp)
        if group_trace:
            keep["group_trace"] = np.zeros((int(n_steps), n_groups))
            r.group_trace = keep["group_trace"].ctypes.data_as(_dp)
    elif group_trace:
        raise ValueError("group_trace without groups")
    Q = int(n_probes) + n_groups
    resume = dict(resume) if resume is not None else None
    r.resume = 0 if resume is None else 1

    def accumulator(prefix, name, n, known):
        if name not in known:
            raise ValueError("unknown statistic %r (known: %s)" % (name, ", ".join(known)))
        dtype = np.int64 if name in _INT_STATS else np.float64
        key = prefix + name
        if resume is not None:
            if key not in resume:
                raise ValueError("resume: %s is missing" % key)
            a = np.array(resume[key], dtype=dtype).reshape(-1)      # (a copy: the march writes it)
            if len(a) != n:
                raise ValueError("resume: %s of %d values for %d" % (key, len(a), n))
        else:
            a = np.zeros(n, dtype)  # (the library initialises on the device)
        keep[key] = a
        setattr(r, key, a.ctypes.data_as(_i64p if dtype == np.int64 else _dp))

    for name in (stats or ()):
        accumulator("q_", name, Q, Q_STATS)
    for name in (thermostat_stats or ()):
        accumulator("th_", name, int(n_thermostats), TH_STATS)
    for name, a in (limits or {}).items():
        if name not in ("lo", "hi"):
            raise ValueError("limits are lo and hi, not %r" % name)
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if len(a) != Q:
            raise ValueError("limits: %s of %d values for %d quantities" % (name, len(a), Q))
        keep["q_" + name] = a
        setattr(r, "q_" + name, a.ctypes.data_as(_dp))
    return r, keep


def series_report_check(md, report=None, loads=None, lib=None, **series):
    """heat_series_report_check: everything about the report of a series that needs no device (series arguments as
    HeatBatch.march_series; loads / report: the arguments of make_zone_loads / make_report). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(**series)
    l, lkeep = make_zone_loads(**(loads or {}))
    r, rkeep = make_report(n_probes=s.n_probes, n_thermostats=l.n_thermostats, n_steps=s.n_steps, **(report or {}))
    rc = L.heat_series_report_check(C.byref(desc), C.byref(s), C.byref(l), C.byref(r))
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


IDEAL_STATS = ("sum_heating", "sum_cooling", "peak_heating", "step_peak_heating", "peak_cooling", "step_peak_cooling",
               "n_sat_heating", "n_sat_cooling")
_IDEAL_INT = ("step_peak_heating", "step_peak_cooling", "n_sat_heating", "n_sat_cooling")


def make_ideal_loads(zone=None, heat_chan=None, cool_chan=None, heat_cap=None, cool_cap=None, stats=IDEAL_STATS, resume=None,
                     step_base=0):
    """Builds a heat_ideal_loads. Returns (ideal, keepalive); the march updates the accumulators of keepalive in place.
    zone, heat_chan, cool_chan   equally long: the zone of every load and its setpoint channels (-1: none; a missing array: all -1)
    heat_cap, cool_cap           W >= 0, inf = unlimited (optional: all unlimited)
    stats                        names out of IDEAL_STATS: which accumulators are maintained (default: all)
    resume                       a dict of arrays a previous series returned: the accumulators start from them
    step_base                    the number the first step of this series has in step_peak_heating / step_peak_cooling"""
    keep = {}
    il = IdealLoads()
    il.step_base = int(step_base)
    il.resume = 0 if resume is None else 1
    z = np.atleast_1d(np.array(zone if zone is not None else [], dtype=np.int32))
    n = len(z)
    il.n_loads = n
    if z.ndim != 1:
        raise ValueError("ideal loads: zone of shape %s" % (z.shape,))
    for name, v, dtype in (("zone", z, np.int32), ("heat_chan", heat_chan, np.int32), ("cool_chan", cool_chan, np.int32),
                           ("heat_cap", heat_cap, np.float64), ("cool_cap", cool_cap, np.float64)):
        if v is None:
            if not name.endswith("_chan"):
                continue
            v = np.full(n, -1)
        a = np.atleast_1d(np.array(v, dtype=dtype))
        if a.shape != (n,):
            raise ValueError("ideal loads: %s of shape %s for %d loads" % (name, a.shape, n))
        keep[name] = a
        if n:
            setattr(il, name, a.ctypes.data_as(_i32p if dtype == np.int32 else _dp))
    for name in (stats or ()):
        if name not in IDEAL_STATS:
            raise ValueError("unknown ideal-load statistic %r (known: %s)" % (name, ", ".join(IDEAL_STATS)))
        dtype = np.int64 if name in _IDEAL_INT else np.float64
        if resume is not None:
            if name not in resume:
                raise ValueError("resume: %s is missing" % name)
            a = np.array(resume[name], dtype=dtype).reshape(-1)  # (a copy: the march writes it)
            if len(a) != n:
                raise ValueError("resume: %s of %d values for %d loads" % (name, len(a), n))
        else:
            a = np.zeros(n, dtype)  # (the library initialises on the device)
        keep[name] = a
        setattr(il, name, a.ctypes.data_as(_i64p if dtype == np.int64 else _dp))
    return il, keep


def ideal_loads_check(md, ideal=None, lib=None, **series):
    """heat_ideal_loads_check: everything about the ideal loads of a series that needs no device (series arguments as
    HeatBatch.march_series; ideal: the arguments of make_ideal_loads). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(**series)
    il, ikeep = make_ideal_loads(**(ideal or {}))
    rc = L.heat_ideal_loads_check(C.byref(desc), C.byref(s), C.byref(il))
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


SKY_SOLAR_FRONT, SKY_SOLAR_BACK, SKY_IR_FRONT, SKY_IR_BACK = 1, 2, 4, 8


def make_sky(record, mode, normals=None):
    """Builds a heat_sky. Returns (sky, keepalive).
    record   [n_steps, n_sites, 8] (or [n_steps, 8] for one site): sun_x, sun_y, sun_z, beam, diffuse, ground, ir_sky,
             ir_ground of every site at every step (heat_sky_record)
    mode     a byte per surface: SKY_SOLAR_FRONT | SKY_SOLAR_BACK | SKY_IR_FRONT | SKY_IR_BACK
    normals  (x, y, z), each per surface: the outward normal of the front face (HeatBatch.march_series and sky_check take
             the model's normal_x, normal_y, cos_tilt when it is None)"""
    keep = {}
    sky = Sky()
    if record is not None:
        rec = np.ascontiguousarray(record, dtype=np.float64)
        if rec.ndim not in (2, 3) or rec.shape[-1] != 8:
            raise ValueError("sky records are [n_steps, n_sites, 8], not %s" % (rec.shape,))
        keep["record"] = rec
        sky.record = C.cast(rec.ctypes.data, C.POINTER(SkyRecord)) if rec.size else None
    if mode is not None:
        m = np.ascontiguousarray(mode, dtype=np.uint8).reshape(-1)
        keep["mode"] = m
        sky.mode = m.ctypes.data_as(C.POINTER(C.c_uint8))
    if normals is not None:
        for name, a in zip(("normal_x", "normal_y", "normal_z"), normals):
            a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
            keep[name] = a
            setattr(sky, name, a.ctypes.data_as(_dp))
    return sky, keep


def _sky_fits(skeep, n_steps, n_sites, n_surfaces):
    rec = skeep.get("record")
    if rec is not None and rec.size and (rec.size // 8 != n_steps * n_sites or (rec.ndim == 3 and rec.shape[1] != n_sites)):
        raise ValueError("sky records %s for %d steps of %d sites" % (rec.shape, n_steps, n_sites))
    for k in ("mode", "normal_x", "normal_y", "normal_z"):
        if k in skeep and skeep[k].shape != (n_surfaces,):
            raise ValueError("sky %s: %s for %d surfaces" % (k, skeep[k].shape, n_surfaces))


def _model_normals(md):
    return md["normal_x"], md["normal_y"], md["cos_tilt"]


def sky_check(md, sky, n_sites=1, lib=None, **series):
    """heat_sky_check: everything about the sky of a series that needs no device (series arguments as
    HeatBatch.march_series; sky: the arguments of make_sky, normals defaulting to the model's). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(n_sites=n_sites, **series)
    _series_arrays_fit(skeep, int(md["n_surfaces"]))
    sky = dict(sky)
    if sky.get("normals") is None:
        sky["normals"] = _model_normals(md)
    k, kkeep = make_sky(**sky)
    _sky_fits(kkeep, s.n_steps, int(n_sites), int(md["n_surfaces"]))
    rc = L.heat_sky_check(C.byref(desc), int(n_sites), C.byref(s), C.byref(k))
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


_GAIN_ARRAYS = (("ap_surface", np.int64, "n_apertures"), ("ap_normal_x", np.float64, "n_apertures"),
                ("ap_normal_y", np.float64, "n_apertures"), ("ap_normal_z", np.float64, "n_apertures"),
                ("ap_tau_diffuse", np.float64, "n_apertures"), ("ap_scale", np.float64, "n_apertures"),
                ("en_surface", np.int64, "n_entries"), ("en_side", np.uint8, "n_entries"), ("en_aperture", np.int32, "n_entries"),
                ("en_beam", np.float64, "n_entries"), ("en_diffuse", np.float64, "n_entries"))


def make_solar_gains(ap_surface=(), ap_normal=None, ap_tau_coef=None, ap_tau_diffuse=(), ap_scale=(), ap_sum=None,
                     en_surface=(), en_side=(), en_aperture=(), en_beam=(), en_diffuse=()):
    """Builds a heat_solar_gains. Returns (gains, keepalive); the march adds onto keepalive["ap_sum"] in place.
    ap_surface      [n_apertures] the window's surface (its site's sky record is read)
    ap_normal       (x, y, z), each [n_apertures]: the outward normal of the side that sees the sky
    ap_tau_coef     [n_apertures, 6] beam transmittance as a polynomial in the cosine of incidence, constant term first
    ap_tau_diffuse  [n_apertures] hemispherical transmittance;  ap_scale [n_apertures] m2
    ap_sum          [n_apertures] what a previous series returned (it is copied), None: zeros
    en_*            [n_entries] the receiver (surface, side 0 front / 1 back), its aperture, its shares in 1/m2"""
    nx, ny, nz = ap_normal if ap_normal is not None else ((), (), ())
    given = dict(ap_surface=ap_surface, ap_normal_x=nx, ap_normal_y=ny, ap_normal_z=nz, ap_tau_diffuse=ap_tau_diffuse, ap_scale=ap_scale,
                 en_surface=en_surface, en_side=en_side, en_aperture=en_aperture, en_beam=en_beam, en_diffuse=en_diffuse)
    g = SolarGains()
    g.n_apertures, g.n_entries = len(np.asarray(ap_surface).reshape(-1)), len(np.asarray(en_surface).reshape(-1))
    keep = {}
    for name, dtype, count in _GAIN_ARRAYS:
        a = np.ascontiguousarray(given[name], dtype=dtype).reshape(-1)
        if a.shape != (getattr(g, count),):
            raise ValueError("solar gains %s: %s for %s = %d" % (name, a.shape, count, getattr(g, count)))
        keep[name] = a
        setattr(g, name, a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if a.size else None)
    coef = np.ascontiguousarray(ap_tau_coef if ap_tau_coef is not None else np.zeros((0, 6)), dtype=np.float64)
    if coef.shape != (g.n_apertures, 6):
        raise ValueError("solar gains ap_tau_coef: %s for %d apertures of 6 coefficients" % (coef.shape, g.n_apertures))
    keep["ap_tau_coef"] = coef
    g.ap_tau_coef = coef.ctypes.data_as(_dp) if coef.size else None
    total = np.zeros(g.n_apertures) if ap_sum is None else np.array(ap_sum, dtype=np.float64).reshape(-1)
    if total.shape != (g.n_apertures,):
        raise ValueError("solar gains ap_sum: %s for %d apertures" % (total.shape, g.n_apertures))
    keep["ap_sum"] = total
    g.ap_sum = total.ctypes.data_as(_dp) if total.size else None
    return g, keep


def _sky_for_gains(sky, normals, n_surfaces):
    """The sky of a call with gains: the records are the gains' too; without mode bytes no side takes its input from the sky."""
    sky = dict(sky or {})
    sky.setdefault("record", None)
    if sky.get("mode") is None:
        sky["mode"] = np.zeros(n_surfaces, np.uint8)
    if sky.get("normals") is None:
        sky["normals"] = normals
    return sky


def solar_gains_check(md, gains, sky=None, n_sites=1, lib=None, **series):
    """heat_solar_gains_check: everything about the solar gains of a series that needs no device (series arguments as
    HeatBatch.march_series; sky: the arguments of make_sky, of which the gains need the records; gains: the arguments of
    make_solar_gains, or None). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(n_sites=n_sites, **series)
    _series_arrays_fit(skeep, int(md["n_surfaces"]))
    k, kkeep = make_sky(**_sky_for_gains(sky, _model_normals(md), int(md["n_surfaces"])))
    _sky_fits(kkeep, s.n_steps, int(n_sites), int(md["n_surfaces"]))
    g, gkeep = make_solar_gains(**gains) if gains is not None else (None, None)
    rc = L.heat_solar_gains_check(C.byref(desc), int(n_sites), C.byref(s), C.byref(k), C.byref(g) if g is not None else None)
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


AIR_STATS = ("sum_q", "steps_open", "switches")
_AIR_ARRAYS = (("target", np.int32), ("source", np.int32), ("temp_chan", np.int32), ("volume_chan", np.int32),
               ("volume_gain", np.float64), ("open_chan", np.int32), ("sense", np.int8), ("band", np.float64),
               ("min_delta", np.float64))
_AIR_OPTIONAL = ("temp_chan", "volume_gain", "open_chan", "sense", "band", "min_delta")
_AIR_INOUT = (("state", np.uint8), ("sum_q", np.float64), ("steps_open", np.int64), ("switches", np.int64))


def make_air_paths(target=(), source=(), temp_chan=None, volume_chan=(), volume_gain=None, open_chan=None, sense=None, band=None,
                   min_delta=None, state=None, sum_q=None, steps_open=None, switches=None, stats=AIR_STATS):
    """Builds a heat_air_paths. Returns (air, keepalive); the march updates keepalive["state"] and the accumulators in place.
    target, source   [n_paths] zones; source -1: supply air at the temperature of channel temp_chan
    temp_chan        [n_paths], -1 where the source is a zone; None: no source is -1
    volume_chan      [n_paths] m3/s;  volume_gain [n_paths], None: 1
    open_chan        [n_paths] the target's setpoint channel of a controlled path, -1: uncontrolled; None: all uncontrolled
    sense, band, min_delta   [n_paths] +1 cooling / -1 heating, K, K: read only where controlled
    state, sum_q, steps_open, switches   [n_paths] what a previous series returned (copied); None: zeros
    stats            which of sum_q, steps_open, switches the march maintains (the others stay NULL)"""
    given = dict(target=target, source=source, temp_chan=temp_chan, volume_chan=volume_chan, volume_gain=volume_gain,
                 open_chan=open_chan, sense=sense, band=band, min_delta=min_delta)
    unknown = set(stats) - set(AIR_STATS)
    if unknown:
        raise ValueError("air paths: unknown stats %s (known: %s)" % (sorted(unknown), ", ".join(AIR_STATS)))
    a = AirPaths()
    n = len(np.asarray(target).reshape(-1))
    a.n_paths = n
    keep = {}
    for name, dtype in _AIR_ARRAYS:
        if given[name] is None and name in _AIR_OPTIONAL:
            continue
        v = np.ascontiguousarray(given[name], dtype=dtype).reshape(-1)
        if v.shape != (n,):
            raise ValueError("air paths %s: %s for %d paths" % (name, v.shape, n))
        keep[name] = v
        setattr(a, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if n else None)
    for (name, dtype), v in zip(_AIR_INOUT, (state, sum_q, steps_open, switches)):
        if name != "state" and name not in stats:
            if v is not None:
                raise ValueError("air paths %s given, but not among stats %s" % (name, tuple(stats)))
            continue
        v = np.zeros(n, dtype) if v is None else np.array(v, dtype=dtype).reshape(-1)  # (a copy: the march writes it)
        if v.shape != (n,):
            raise ValueError("air paths %s: %s for %d paths" % (name, v.shape, n))
        keep[name] = v
        setattr(a, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if n else None)
    return a, keep


def air_paths_check(md, air, n_sites=1, lib=None, **series):
    """heat_air_paths_check: everything about the air paths of a series that needs no device (series arguments as
    HeatBatch.march_series; air: the arguments of make_air_paths, or None). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(n_sites=n_sites, **series)
    _series_arrays_fit(skeep, int(md["n_surfaces"]))
    a, akeep = make_air_paths(**air) if air is not None else (None, None)
    rc = L.heat_air_paths_check(C.byref(desc), int(n_sites), C.byref(s), C.byref(a) if a is not None else None)
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


def make_shades(surface=(), normal=None, right=None, up=None, width=(), height=(), overhang_depth=None, overhang_gap=None,
                fin_pos_depth=None, fin_pos_gap=None, fin_neg_depth=None, fin_neg_gap=None, diffuse_factor=None, ground_factor=None,
                horizon=None, horizon_tan2=None, front_shade=None, back_shade=None, aperture_shade=None):
    """Builds a heat_shades. Returns (shades, keepalive).
    surface          [n_shades] a surface of the shade's weather site (its site's sky record is read)
    normal, right, up   (x, y, z) each, [n_shades]: the outward normal n of the shaded plane, its in-plane horizontal axis u
                     (to the right seen from outside) and its in-plane upward axis v (shading.frame_of builds u and v)
    width, height    [n_shades] m, > 0
    overhang_depth, overhang_gap, fin_pos_depth, fin_pos_gap, fin_neg_depth, fin_neg_gap   [n_shades] m, >= 0; None: zeros
    diffuse_factor, ground_factor   [n_shades]; None: NULL = 1
    horizon          [n_shades] the shade's horizon profile, -1: none; None: NULL = none
    horizon_tan2     [n_horizons, 16] (shading.horizon_tan2)
    front_shade, back_shade   [n_surfaces] the shade of the side's sky-driven solar input, -1: none; None: NULL
    aperture_shade   [n_apertures] the shade of an aperture of the solar gains, -1: none; None: NULL"""
    sh = Shades()
    n = len(np.asarray(surface).reshape(-1))
    sh.n_shades = n
    keep = {}

    def put(name, value, dtype, shape, what):
        a = np.ascontiguousarray(value, dtype=dtype)
        if shape is not None and a.reshape(-1).shape != shape:
            raise ValueError("shades %s: %s for %s" % (name, a.shape, what))
        keep[name] = a
        setattr(sh, name, a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if a.size else None)

    put("sh_surface", surface, np.int64, (n,), "%d shades" % n)
    for prefix, vec in (("sh_normal", normal), ("sh_right", right), ("sh_up", up)):
        vec = vec if vec is not None else ((), (), ())
        for axis, a in zip("xyz", vec):
            put("%s_%s" % (prefix, axis), a, np.float64, (n,), "%d shades" % n)
    put("sh_width", width, np.float64, (n,), "%d shades" % n)
    put("sh_height", height, np.float64, (n,), "%d shades" % n)
    for name, v in (("overhang_depth", overhang_depth), ("overhang_gap", overhang_gap), ("fin_pos_depth", fin_pos_depth),
                    ("fin_pos_gap", fin_pos_gap), ("fin_neg_depth", fin_neg_depth), ("fin_neg_gap", fin_neg_gap)):
        put(name, np.zeros(n) if v is None else v, np.float64, (n,), "%d shades" % n)
    for name, v in (("diffuse_factor", diffuse_factor), ("ground_factor", ground_factor)):
        if v is not None:
            put(name, v, np.float64, (n,), "%d shades" % n)
    if horizon is not None:
        put("sh_horizon", horizon, np.int32, (n,), "%d shades" % n)
    tan2 = np.ascontiguousarray(horizon_tan2 if horizon_tan2 is not None else np.zeros((0, 16)), dtype=np.float64)
    if tan2.ndim != 2 or tan2.shape[1] != 16:
        raise ValueError("shades horizon_tan2: %s, not [n_horizons, 16]" % (tan2.shape,))
    sh.n_horizons = len(tan2)
    put("horizon_tan2", tan2, np.float64, None, "")
    for name, v in (("front_shade", front_shade), ("back_shade", back_shade), ("aperture_shade", aperture_shade)):
        if v is not None:
            put(name, np.asarray(v).reshape(-1), np.int32, None, "")
    return sh, keep


def _shades_fit(hkeep, n_surfaces, n_apertures):
    for k in ("front_shade", "back_shade"):
        if k in hkeep and hkeep[k].shape != (n_surfaces,):
            raise ValueError("shades %s: %s for %d surfaces" % (k, hkeep[k].shape, n_surfaces))
    if "aperture_shade" in hkeep and n_apertures is not None and hkeep["aperture_shade"].shape != (n_apertures,):
        raise ValueError("shades aperture_shade: %s for %d apertures" % (hkeep["aperture_shade"].shape, n_apertures))


def shades_check(md, shades, sky=None, gains=None, n_sites=1, lib=None, **series):
    """heat_shades_check: everything about the shades of a series that needs no device (series arguments as
    HeatBatch.march_series; sky: the arguments of make_sky, or None; gains: those of make_solar_gains, or None; shades: those
    of make_shades, or None). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(n_sites=n_sites, **series)
    _series_arrays_fit(skeep, int(md["n_surfaces"]))
    k = None
    if sky is not None or gains is not None:
        k, kkeep = make_sky(**_sky_for_gains(sky, _model_normals(md), int(md["n_surfaces"])))
        _sky_fits(kkeep, s.n_steps, int(n_sites), int(md["n_surfaces"]))
    g, gkeep = make_solar_gains(**gains) if gains is not None else (None, None)
    h, hkeep = make_shades(**shades) if shades is not None else (None, None)
    if h is not None:
        _shades_fit(hkeep, int(md["n_surfaces"]), g.n_apertures if g is not None else None)
    rc = L.heat_shades_check(C.byref(desc), int(n_sites), C.byref(s), C.byref(k) if k is not None else None,
                             C.byref(g) if g is not None else None, C.byref(h) if h is not None else None)
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


_RADIATION_ARRAYS = (("rc_surface", np.int64, "n_receivers"), ("rc_side", np.uint8, "n_receivers"),
                     ("en_receiver", np.int64, "n_entries"), ("en_surface", np.int64, "n_entries"), ("en_side", np.uint8, "n_entries"),
                     ("en_factor", np.float64, "n_entries"))


def make_room_radiation(rc_surface=(), rc_side=(), en_receiver=(), en_surface=(), en_side=(), en_factor=(), en_chan=None,
                        sum_irradiance=None):
    """Builds a heat_room_radiation. Returns (radiation, keepalive); the march adds onto keepalive["sum_irradiance"] in place.
    rc_surface, rc_side   [n_receivers] the sides whose long-wave input the rule forms (0 front, 1 back)
    en_receiver      [n_entries] the receiver the entry belongs to
    en_surface, en_side   [n_entries] the emitter side; en_surface -1: the entry is the value of channel en_chan
    en_factor        [n_entries] view factor times the caller's emissivity convention
    en_chan          [n_entries] -1 where the emitter is a surface; None: NULL (no entry is a channel)
    sum_irradiance   [n_receivers] what a previous series returned (it is copied), None: zeros
    (room_radiation.exchange_by_area builds the first six for the rooms of a model)"""
    given = dict(rc_surface=rc_surface, rc_side=rc_side, en_receiver=en_receiver, en_surface=en_surface, en_side=en_side,
                 en_factor=en_factor)
    rr = RoomRadiation()
    rr.n_receivers, rr.n_entries = len(np.asarray(rc_surface).reshape(-1)), len(np.asarray(en_receiver).reshape(-1))
    keep = {}
    for name, dtype, count in _RADIATION_ARRAYS:
        a = np.ascontiguousarray(given[name], dtype=dtype).reshape(-1)
        if a.shape != (getattr(rr, count),):
            raise ValueError("room radiation %s: %s for %s = %d" % (name, a.shape, count, getattr(rr, count)))
        keep[name] = a
        setattr(rr, name, a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if a.size else None)
    if en_chan is not None:
        chan = np.ascontiguousarray(en_chan, dtype=np.int32).reshape(-1)
        if chan.shape != (rr.n_entries,):
            raise ValueError("room radiation en_chan: %s for n_entries = %d" % (chan.shape, rr.n_entries))
        keep["en_chan"] = chan
        rr.en_chan = chan.ctypes.data_as(_i32p) if chan.size else None
    total = np.zeros(rr.n_receivers) if sum_irradiance is None else np.array(sum_irradiance, dtype=np.float64).reshape(-1)
    if total.shape != (rr.n_receivers,):
        raise ValueError("room radiation sum_irradiance: %s for %d receivers" % (total.shape, rr.n_receivers))
    keep["sum_irradiance"] = total
    rr.sum_irradiance = total.ctypes.data_as(_dp) if total.size else None
    return rr, keep


def room_radiation_check(md, radiation, sky=None, n_sites=1, lib=None, **series):
    """heat_room_radiation_check: everything about the room radiation of a series that needs no device (series arguments as
    HeatBatch.march_series; sky: the arguments of make_sky, or None; radiation: those of make_room_radiation, or None).
    Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(n_sites=n_sites, **series)
    _series_arrays_fit(skeep, int(md["n_surfaces"]))
    k = None
    if sky is not None:
        sky = dict(sky)
        if sky.get("normals") is None:
            sky["normals"] = _model_normals(md)
        k, kkeep = make_sky(**sky)
        _sky_fits(kkeep, s.n_steps, int(n_sites), int(md["n_surfaces"]))
    rr, rkeep = make_room_radiation(**radiation) if radiation is not None else (None, None)
    rc = L.heat_room_radiation_check(C.byref(desc), int(n_sites), C.byref(s), C.byref(k) if k is not None else None,
                                     C.byref(rr) if rr is not None else None)
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


_AMBIENT_ARRAYS = (("surface", np.int64, True), ("side", np.uint8, True), ("chan", np.int32, True), ("gain", np.float64, False),
                   ("offset", np.float64, False), ("mix_zone", np.int32, False), ("mix", np.float64, False))


def make_ambient(surface=(), side=(), chan=(), gain=None, offset=None, mix_zone=None, mix=None, sum_temperature=None):
    """Builds a heat_ambient_drive. Returns (drive, keepalive); the march adds onto keepalive["sum_temperature"] in place.
    surface, side    [n_sides] the driven sides (0 front, 1 back), each of kind AMBIENT
    chan             [n_sides] the channel of the series that carries the temperature, C
    gain, offset     [n_sides] or None (NULL: 1 / 0)
    mix_zone         [n_sides] the zone a side's temperature is mixed with, -1: none; None: NULL
    mix              [n_sides] 1 - b of EN ISO 13789 (ambient.b_factor), read where mix_zone >= 0; None: NULL
    sum_temperature  [n_sides] what a previous series returned (it is copied), None: zeros, False: NULL (no sums are kept)
    (ambient.apply is the rule in numpy and takes the same dict)"""
    given = dict(surface=surface, side=side, chan=chan, gain=gain, offset=offset, mix_zone=mix_zone, mix=mix)
    a = AmbientDrive()
    a.n_sides = len(np.asarray(surface).reshape(-1))
    keep = {}
    for name, dtype, needed in _AMBIENT_ARRAYS:
        if given[name] is None and not needed:
            continue
        v = np.ascontiguousarray(given[name], dtype=dtype).reshape(-1)
        if v.shape != (a.n_sides,):
            raise ValueError("ambient drive %s: %s for n_sides = %d" % (name, v.shape, a.n_sides))
        keep[name] = v
        setattr(a, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if v.size else None)
    if sum_temperature is False:
        keep["sum_temperature"] = np.zeros(0)
    else:
        total = np.zeros(a.n_sides) if sum_temperature is None else np.array(sum_temperature, dtype=np.float64).reshape(-1)
        if total.shape != (a.n_sides,):
            raise ValueError("ambient drive sum_temperature: %s for %d sides" % (total.shape, a.n_sides))
        keep["sum_temperature"] = total
        a.sum_temperature = total.ctypes.data_as(_dp) if total.size else None
    return a, keep


def ambient_check(md, ambient, n_sites=1, lib=None, **series):
    """heat_ambient_check: everything about the ambient drive of a series that needs no device (series arguments as
    HeatBatch.march_series; ambient: the arguments of make_ambient, or None). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(n_sites=n_sites, **series)
    _series_arrays_fit(skeep, int(md["n_surfaces"]))
    a, akeep = make_ambient(**ambient) if ambient is not None else (None, None)
    rc = L.heat_ambient_check(C.byref(desc), int(n_sites), C.byref(s), C.byref(a) if a is not None else None)
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


BLIND_STATS = ("steps_closed", "switches", "sum_position")
_BLIND_ARRAYS = (("shade", np.int32, True), ("beam_closed", np.float64, True), ("diffuse_closed", np.float64, True),
                 ("ground_closed", np.float64, True), ("pos_chan", np.int32, False), ("irr_close", np.float64, False),
                 ("irr_open", np.float64, False), ("zone", np.int32, False), ("set_chan", np.int32, False), ("band", np.float64, False),
                 ("enable_chan", np.int32, False))
_BLIND_INOUT = (("state", np.uint8), ("steps_closed", np.int64), ("switches", np.int64), ("sum_position", np.float64))


def make_blinds(shade=(), beam_closed=(), diffuse_closed=(), ground_closed=(), pos_chan=None, irr_close=None, irr_open=None, zone=None,
                set_chan=None, band=None, enable_chan=None, state=None, steps_closed=None, switches=None, sum_position=None,
                stats=BLIND_STATS):
    """Builds a heat_blinds. Returns (blinds, keepalive); the march updates keepalive["state"] and the accumulators in place.
    shade            [n_blinds] the shade of the call's shades the blind rides on (at most one blind per shade)
    beam_closed, diffuse_closed, ground_closed   [n_blinds] the factors of the fully closed blind, >= 0
    pos_chan         [n_blinds] the position channel of a SCHEDULED blind, -1: controlled; None: all controlled
    irr_close, irr_open   [n_blinds] W/m2 on the shade's plane, irr_open <= irr_close: read only where controlled
    zone             [n_blinds] the zone whose temperature gates the blind, -1: none; None: no room condition anywhere
    set_chan, band   [n_blinds] the zone's setpoint channel (C) and the band (K): read only where zone >= 0
    enable_chan      [n_blinds] enabled where row[chan] > 0, -1: always; None: always enabled
    state, steps_closed, switches, sum_position   [n_blinds] what a previous series returned (copied); None: zeros
    stats            which of steps_closed, switches, sum_position the march maintains (the others stay NULL)
    (blinds.apply is the rule in numpy and takes the same dict)"""
    given = dict(shade=shade, beam_closed=beam_closed, diffuse_closed=diffuse_closed, ground_closed=ground_closed, pos_chan=pos_chan,
                 irr_close=irr_close, irr_open=irr_open, zone=zone, set_chan=set_chan, band=band, enable_chan=enable_chan)
    unknown = set(stats) - set(BLIND_STATS)
    if unknown:
        raise ValueError("blinds: unknown stats %s (known: %s)" % (sorted(unknown), ", ".join(BLIND_STATS)))
    bl = Blinds()
    n = len(np.asarray(shade).reshape(-1))
    bl.n_blinds = n
    keep = {}
    for name, dtype, needed in _BLIND_ARRAYS:
        if given[name] is None and not needed:
            continue
        v = np.ascontiguousarray(given[name], dtype=dtype).reshape(-1)
        if v.shape != (n,):
            raise ValueError("blinds %s: %s for %d blinds" % (name, v.shape, n))
        keep[name] = v
        setattr(bl, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if n else None)
    for (name, dtype), v in zip(_BLIND_INOUT, (state, steps_closed, switches, sum_position)):
        if name != "state" and name not in stats:
            if v is not None:
                raise ValueError("blinds %s given, but not among stats %s" % (name, tuple(stats)))
            continue
        v = np.zeros(n, dtype) if v is None else np.array(v, dtype=dtype).reshape(-1)  # (a copy: the march writes it)
        if v.shape != (n,):
            raise ValueError("blinds %s: %s for %d blinds" % (name, v.shape, n))
        keep[name] = v
        setattr(bl, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if n else None)
    return bl, keep


def blinds_check(md, blinds, shades=None, sky=None, gains=None, n_sites=1, lib=None, **series):
    """heat_blinds_check: everything about the blinds of a series that needs no device (series arguments as
    HeatBatch.march_series; sky, gains, shades as shades_check takes them; blinds: the arguments of make_blinds, or None).
    Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(n_sites=n_sites, **series)
    _series_arrays_fit(skeep, int(md["n_surfaces"]))
    k = None
    if sky is not None or gains is not None:
        k, kkeep = make_sky(**_sky_for_gains(sky, _model_normals(md), int(md["n_surfaces"])))
        _sky_fits(kkeep, s.n_steps, int(n_sites), int(md["n_surfaces"]))
    g, gkeep = make_solar_gains(**gains) if gains is not None else (None, None)
    h, hkeep = make_shades(**shades) if shades is not None else (None, None)
    if h is not None:
        _shades_fit(hkeep, int(md["n_surfaces"]), g.n_apertures if g is not None else None)
    bl, bkeep = make_blinds(**blinds) if blinds is not None else (None, None)
    ref = lambda x: C.byref(x) if x is not None else None
    rc = L.heat_blinds_check(C.byref(desc), int(n_sites), C.byref(s), ref(k), ref(g), ref(h), ref(bl))
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


_ANISO_BANDS = ("front_band", "back_band", "aperture_band", "shade_band")


def make_sky_aniso(coef=None, front_band=None, back_band=None, aperture_band=None, shade_band=None):
    """Builds a heat_sky_aniso. Returns (aniso, keepalive).
    coef            [n_steps, n_sites, 2] (or [n_steps, 2] for one site): (circ, horiz) = (F1, F2) of every site at every step,
                    beside the sky's records (sky.hay_davies and sky.reindl give pairs: np.stack them on the last axis)
    front_band, back_band   a value per surface: the band of the front / back solar input (sky.band_reindl, sky.band_perez);
                    None: zeros
    aperture_band   a value per aperture of the call's gains; None: zeros
    shade_band      a value per shade of the call's shades, read by the blinds for the irradiance they decide on; None: zeros"""
    keep = {}
    an = SkyAniso()
    if coef is not None:
        q = np.ascontiguousarray(coef, dtype=np.float64)
        if q.ndim not in (2, 3) or q.shape[-1] != 2:
            raise ValueError("sky coefficients are [n_steps, n_sites, 2], not %s" % (q.shape,))
        keep["coef"] = q
        an.coef = C.cast(q.ctypes.data, C.POINTER(SkyCoef)) if q.size else None
    for name, v in zip(_ANISO_BANDS, (front_band, back_band, aperture_band, shade_band)):
        if v is None:
            continue
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        keep[name] = v
        setattr(an, name, v.ctypes.data_as(_dp))   # (also of no length: a band that was given is not NULL)
    return an, keep


def _aniso_fits(akeep, n_steps, n_sites, n_surfaces, n_apertures, n_shades):
    q = akeep.get("coef")
    if q is not None and q.size and (q.size // 2 != n_steps * n_sites or (q.ndim == 3 and q.shape[1] != n_sites)):
        raise ValueError("sky coefficients %s for %d steps of %d sites" % (q.shape, n_steps, n_sites))
    for name, n, what in (("front_band", n_surfaces, "surfaces"), ("back_band", n_surfaces, "surfaces"),
                          ("aperture_band", n_apertures, "apertures"), ("shade_band", n_shades, "shades")):
        if name in akeep and n is not None and akeep[name].shape != (n,):
            raise ValueError("sky aniso %s: %s for %d %s" % (name, akeep[name].shape, n, what))


def sky_aniso_check(md, aniso, sky=None, gains=None, shades=None, n_sites=1, lib=None, **series):
    """heat_sky_aniso_check: everything about the anisotropic sky of a series that needs no device (series arguments as
    HeatBatch.march_series; sky, gains, shades as shades_check takes them, or None; aniso: the arguments of make_sky_aniso, or
    None). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(n_sites=n_sites, **series)
    _series_arrays_fit(skeep, int(md["n_surfaces"]))
    k = None
    if sky is not None or gains is not None:
        k, kkeep = make_sky(**_sky_for_gains(sky, _model_normals(md), int(md["n_surfaces"])))
        _sky_fits(kkeep, s.n_steps, int(n_sites), int(md["n_surfaces"]))
    g, gkeep = make_solar_gains(**gains) if gains is not None else (None, None)
    h, hkeep = make_shades(**shades) if shades is not None else (None, None)
    if h is not None:
        _shades_fit(hkeep, int(md["n_surfaces"]), g.n_apertures if g is not None else None)
    an, akeep = make_sky_aniso(**aniso) if aniso is not None else (None, None)
    if an is not None:
        _aniso_fits(akeep, s.n_steps, int(n_sites), int(md["n_surfaces"]), g.n_apertures if g is not None else None,
                    h.n_shades if h is not None else None)
    ref = lambda x: C.byref(x) if x is not None else None
    rc = L.heat_sky_aniso_check(C.byref(desc), int(n_sites), C.byref(s), ref(k), ref(g), ref(h), ref(an))
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


COMFORT_STATS = ("n_occupied", "sum_operative", "min_operative", "step_min", "max_operative", "step_max", "n_below", "deg_below",
                 "n_above", "deg_above", "max_above", "step_max_above")
_COMFORT_INT = ("n_occupied", "step_min", "step_max", "n_below", "n_above", "step_max_above")
_COMFORT_SENSOR = (("zone", np.int32, True), ("air_weight", np.float64, False), ("control", np.uint8, False), ("occ_chan", np.int32, False),
                   ("lo_chan", np.int32, False), ("hi_chan", np.int32, False))
_COMFORT_ENTRY = (("en_sensor", np.int32), ("en_surface", np.int64), ("en_side", np.uint8), ("en_weight", np.float64))


def make_comfort(zone=(), air_weight=None, control=None, en_sensor=(), en_surface=(), en_side=(), en_weight=(), occ_chan=None,
                 lo_chan=None, hi_chan=None, stats=COMFORT_STATS, resume=None, step_base=0):
    """Builds a heat_comfort. Returns (comfort, keepalive); the march updates the accumulators of keepalive in place.
    zone             [n_sensors] the zone whose air the sensor stands in
    air_weight       [n_sensors] the share of the air temperature in the operative temperature, in [0, 1]; None: 0.5
    control          [n_sensors] 1: the sensor is the control temperature of its zone (at most one per zone); None: none
    en_sensor, en_surface, en_side, en_weight   [n_entries] the faces a sensor sees: its number, the surface, 0 first / 1 last
                     node, the weight (comfort.by_area makes them sum to 1 per sensor); in any order
    occ_chan, lo_chan, hi_chan   [n_sensors] occupied where row[chan] > 0 / the band's limits, -1 or None: always / no limit
    stats            names out of COMFORT_STATS: which accumulators are maintained (default: all)
    resume           a dict of arrays a previous series returned: the accumulators start from them
    step_base        the number the first step of this series has in step_min, step_max, step_max_above
    (comfort.operative, control_temperatures and accumulate are the rule in numpy and take the same dict)"""
    given = dict(zone=zone, air_weight=air_weight, control=control, occ_chan=occ_chan, lo_chan=lo_chan, hi_chan=hi_chan,
                 en_sensor=en_sensor, en_surface=en_surface, en_side=en_side, en_weight=en_weight)
    unknown = set(stats or ()) - set(COMFORT_STATS)
    if unknown:
        raise ValueError("comfort: unknown stats %s (known: %s)" % (sorted(unknown), ", ".join(COMFORT_STATS)))
    cf = Comfort()
    keep = {}
    n = len(np.asarray(zone if zone is not None else ()).reshape(-1))
    ne = len(np.asarray(en_sensor if en_sensor is not None else ()).reshape(-1))
    cf.n_sensors, cf.n_entries, cf.resume, cf.step_base = n, ne, 0 if resume is None else 1, int(step_base)
    for name, dtype, needed in _COMFORT_SENSOR:
        if given[name] is None and not needed:
            continue
        v = np.ascontiguousarray(given[name] if given[name] is not None else (), dtype=dtype).reshape(-1)
        if v.shape != (n,):
            raise ValueError("comfort %s: %s for %d sensors" % (name, v.shape, n))
        keep[name] = v
        setattr(cf, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if n else None)
    for name, dtype in _COMFORT_ENTRY:
        v = np.ascontiguousarray(given[name] if given[name] is not None else (), dtype=dtype).reshape(-1)
        if v.shape != (ne,):
            raise ValueError("comfort %s: %s for %d entries" % (name, v.shape, ne))
        keep[name] = v
        setattr(cf, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if ne else None)
    for name in (stats or ()):
        dtype = np.int64 if name in _COMFORT_INT else np.float64
        if resume is not None:
            if name not in resume:
                raise ValueError("comfort resume: %s is missing" % name)
            a = np.array(resume[name], dtype=dtype).reshape(-1)  # (a copy: the march writes it)
            if len(a) != n:
                raise ValueError("comfort resume: %s of %d values for %d sensors" % (name, len(a), n))
        else:
            a = np.zeros(n, dtype)  # (the library initialises on the device)
        keep[name] = a
        setattr(cf, name, a.ctypes.data_as(_i64p if dtype == np.int64 else _dp))
    return cf, keep


def comfort_check(md, comfort, lib=None, **series):
    """heat_comfort_check: everything about the comfort term of a series that needs no device (series arguments as
    HeatBatch.march_series; comfort: the arguments of make_comfort, or None). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(**series)
    cf, ckeep = make_comfort(**comfort) if comfort is not None else (None, None)
    rc = L.heat_comfort_check(C.byref(desc), C.byref(s), C.byref(cf) if cf is not None else None)
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


HANDLER_STATS = ("sum_recovered", "sum_heating", "sum_cooling", "steps_bypass", "switches", "steps_heat_saturated",
                 "steps_cool_saturated", "sum_branch_q")
_HANDLER_UNIT = (("outdoor_chan", np.int32, True), ("eff_chan", np.int32, False), ("eff_gain", np.float64, False),
                 ("bypass_chan", np.int32, False), ("bypass_band", np.float64, False), ("bypass_min_delta", np.float64, False),
                 ("heat_chan", np.int32, False), ("cool_chan", np.int32, False), ("heat_cap", np.float64, False),
                 ("cool_cap", np.float64, False))
_HANDLER_BRANCH = (("br_unit", np.int32, True), ("br_zone", np.int32, True), ("br_volume_chan", np.int32, True),
                   ("br_volume_gain", np.float64, False), ("br_kind", np.uint8, False))
_HANDLER_INT = ("steps_bypass", "switches", "steps_heat_saturated", "steps_cool_saturated")


def make_air_handlers(outdoor_chan=(), eff_chan=None, eff_gain=None, bypass_chan=None, bypass_band=None, bypass_min_delta=None,
                      heat_chan=None, cool_chan=None, heat_cap=None, cool_cap=None, br_unit=(), br_zone=(), br_volume_chan=(),
                      br_volume_gain=None, br_kind=None, bypass=None, stats=HANDLER_STATS, **acc):
    """Builds a heat_air_handlers. Returns (handlers, keepalive); the march updates keepalive["bypass"] and the accumulators in
    place.
    outdoor_chan     [n_units] the channel of the outdoor-air temperature, C
    eff_gain, eff_chan   [n_units] the effectiveness: the gain (None: 1) times the channel's value (None / -1: none)
    bypass_chan, bypass_band, bypass_min_delta   [n_units] the setpoint channel of the extract air (None / -1: no bypass), K, K
    heat_chan, cool_chan   [n_units] the channel of the minimum / maximum supply temperature (None / -1: no coil)
    heat_cap, cool_cap     [n_units] W, inf allowed; None: inf
    br_unit, br_zone, br_volume_chan   [n_branches] the unit, the zone, the channel of the volume flow in m3/s
    br_volume_gain, br_kind   [n_branches] None: 1 / None: 3 (1 supplies, 2 extracts, 3 both)
    bypass and the names of HANDLER_STATS   what a previous series returned (copied); None: zeros
    stats            which of HANDLER_STATS the march maintains (the others stay NULL)
    (air_handlers.apply and accumulate are the rule in numpy and take the same dict)"""
    given = dict(outdoor_chan=outdoor_chan, eff_chan=eff_chan, eff_gain=eff_gain, bypass_chan=bypass_chan, bypass_band=bypass_band,
                 bypass_min_delta=bypass_min_delta, heat_chan=heat_chan, cool_chan=cool_chan, heat_cap=heat_cap, cool_cap=cool_cap,
                 br_unit=br_unit, br_zone=br_zone, br_volume_chan=br_volume_chan, br_volume_gain=br_volume_gain, br_kind=br_kind)
    unknown = (set(stats or ()) | set(acc)) - set(HANDLER_STATS)
    if unknown:
        raise ValueError("air handlers: unknown stats %s (known: %s)" % (sorted(unknown), ", ".join(HANDLER_STATS)))
    h = AirHandlers()
    keep = {}
    n = len(np.asarray(outdoor_chan if outdoor_chan is not None else ()).reshape(-1))
    nb = len(np.asarray(br_unit if br_unit is not None else ()).reshape(-1))
    h.n_units, h.n_branches = n, nb
    for rows, count, what in ((_HANDLER_UNIT, n, "units"), (_HANDLER_BRANCH, nb, "branches")):
        for name, dtype, needed in rows:
            if given[name] is None and not needed:
                continue
            v = np.ascontiguousarray(given[name] if given[name] is not None else (), dtype=dtype).reshape(-1)
            if v.shape != (count,):
                raise ValueError("air handlers %s: %s for %d %s" % (name, v.shape, count, what))
            keep[name] = v
            setattr(h, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if count else None)
    inout = [("bypass", np.uint8, n, bypass)]
    for name in HANDLER_STATS:
        if name not in (stats or ()):
            if acc.get(name) is not None:
                raise ValueError("air handlers %s given, but not among stats %s" % (name, tuple(stats or ())))
            continue
        inout.append((name, np.int64 if name in _HANDLER_INT else np.float64, nb if name == "sum_branch_q" else n, acc.get(name)))
    for name, dtype, count, v in inout:
        v = np.zeros(count, dtype) if v is None else np.array(v, dtype=dtype).reshape(-1)  # (a copy: the march writes it)
        if v.shape != (count,):
            raise ValueError("air handlers %s: %s for %d" % (name, v.shape, count))
        keep[name] = v
        setattr(h, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if count else None)
    return h, keep


def air_handlers_check(md, handlers, lib=None, **series):
    """heat_air_handlers_check: everything about the air handlers of a series that needs no device (series arguments as
    HeatBatch.march_series; handlers: the arguments of make_air_handlers, or None). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(**series)
    h, hkeep = make_air_handlers(**handlers) if handlers is not None else (None, None)
    rc = L.heat_air_handlers_check(C.byref(desc), C.byref(s), C.byref(h) if h is not None else None)
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


SPECIES_STATS = ("n_occupied", "sum_conc", "max_conc", "step_max", "n_above", "excess_above", "sum_volume", "sum_q", "steps_saturated")
_SPECIES_VENT_STATS = ("sum_volume", "sum_q", "steps_saturated")
_SPECIES_INT = ("n_occupied", "step_max", "n_above", "steps_saturated")
_SPECIES_SOURCE = (("src_zone", np.int32, True), ("src_species", np.int32, True), ("src_chan", np.int32, True), ("src_factor", np.float64, False))
_SPECIES_VENT = (("vent_zone", np.int32, True), ("vent_species", np.int32, True), ("vent_temp_chan", np.int32, True),
                 ("vent_enable_chan", np.int32, False), ("vent_v_min", np.float64, True), ("vent_v_max", np.float64, True),
                 ("vent_c_lo", np.float64, True), ("vent_c_hi", np.float64, True))


def make_air_species(outdoor_chan=None, conc=None, src_zone=(), src_species=(), src_chan=(), src_factor=None, vent_zone=(), vent_species=(),
                     vent_temp_chan=(), vent_enable_chan=None, vent_v_min=(), vent_v_max=(), vent_c_lo=(), vent_c_hi=(), limit_chan=None,
                     occ_chan=None, stats=SPECIES_STATS, resume=None, step_base=0):
    """Builds a heat_air_species. Returns (species, keepalive); the march updates keepalive["conc"] and the accumulators in place.
    outdoor_chan     [n_species, n_zones] the channel of the concentration of the OUTSIDE air entering a zone, -1: 0.0
                     (air_species.per_zone broadcasts one channel per species); None: no species
    conc             [n_species, n_zones] the concentrations the series starts with (copied); None: zeros
    src_zone, src_species, src_chan, src_factor   [n_sources] amount per second = factor (None: 1) * the channel's value
    vent_zone, vent_species, vent_temp_chan, vent_enable_chan, vent_v_min, vent_v_max, vent_c_lo, vent_c_hi   [n_vents] the demand
                     vents: the zone, the species whose concentration in that zone drives it, the channel of the outdoor-air
                     temperature, the enable channel (None / -1: always), m3/s at and below c_lo, m3/s at and above c_hi
    limit_chan       [n_species] the channel of the limit n_above / excess_above count against, None / -1: none
    occ_chan         [n_zones] occupied where row[chan] > 0, None / -1: always
    stats            names out of SPECIES_STATS: which accumulators are maintained (default: all)
    resume           a dict of arrays a previous series returned: the accumulators start from them
    step_base        the number the first step of this series has in step_max
    (air_species.apply and accumulate are the rule in numpy and take the same dict)"""
    given = dict(src_zone=src_zone, src_species=src_species, src_chan=src_chan, src_factor=src_factor, vent_zone=vent_zone,
                 vent_species=vent_species, vent_temp_chan=vent_temp_chan, vent_enable_chan=vent_enable_chan, vent_v_min=vent_v_min,
                 vent_v_max=vent_v_max, vent_c_lo=vent_c_lo, vent_c_hi=vent_c_hi)
    unknown = set(stats or ()) - set(SPECIES_STATS)
    if unknown:
        raise ValueError("air species: unknown stats %s (known: %s)" % (sorted(unknown), ", ".join(SPECIES_STATS)))
    sp = AirSpecies()
    keep = {}
    oc = np.zeros((0, 0), np.int32) if outdoor_chan is None else np.ascontiguousarray(outdoor_chan, dtype=np.int32)
    if oc.ndim != 2:
        raise ValueError("air species outdoor_chan: shape %s is not [n_species, n_zones]" % (oc.shape,))
    ns, nz = oc.shape
    nq = len(np.asarray(src_zone if src_zone is not None else ()).reshape(-1))
    nv = len(np.asarray(vent_zone if vent_zone is not None else ()).reshape(-1))
    sp.n_species, sp.n_sources, sp.n_vents, sp.resume, sp.step_base = ns, nq, nv, 0 if resume is None else 1, int(step_base)
    keep["outdoor_chan"] = oc
    sp.outdoor_chan = oc.ctypes.data_as(_i32p) if oc.size else None
    c = np.zeros((ns, nz)) if conc is None else np.array(conc, dtype=np.float64)  # (a copy: the march writes it)
    if c.shape != (ns, nz):
        raise ValueError("air species conc: %s for %d species in %d zones" % (c.shape, ns, nz))
    keep["conc"] = c
    sp.conc = c.ctypes.data_as(_dp) if c.size else None
    for rows, count, what in ((_SPECIES_SOURCE, nq, "sources"), (_SPECIES_VENT, nv, "vents")):
        for name, dtype, needed in rows:
            if given[name] is None and not needed:
                continue
            v = np.ascontiguousarray(given[name] if given[name] is not None else (), dtype=dtype).reshape(-1)
            if v.shape != (count,):
                raise ValueError("air species %s: %s for %d %s" % (name, v.shape, count, what))
            keep[name] = v
            setattr(sp, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if count else None)
    for name, v, count in (("limit_chan", limit_chan, ns), ("occ_chan", occ_chan, nz)):
        if v is None:
            continue
        v = np.ascontiguousarray(v, dtype=np.int32).reshape(-1)
        if v.shape != (count,):
            raise ValueError("air species %s: %s for %d" % (name, v.shape, count))
        keep[name] = v
        setattr(sp, name, v.ctypes.data_as(_i32p) if count else None)
    for name in (stats or ()):
        dtype = np.int64 if name in _SPECIES_INT else np.float64
        shape = (nv,) if name in _SPECIES_VENT_STATS else (ns, nz)
        if resume is not None:
            if name not in resume:
                raise ValueError("air species resume: %s is missing" % name)
            a = np.array(resume[name], dtype=dtype)  # (a copy: the march writes it)
            if a.shape != shape:
                raise ValueError("air species resume: %s of shape %s, not %s" % (name, a.shape, shape))
        else:
            a = np.zeros(shape, dtype)  # (the library initialises on the device)
        keep[name] = a
        setattr(sp, name, a.ctypes.data_as(_i64p if dtype == np.int64 else _dp) if a.size else None)
    return sp, keep


def air_species_check(md, species, loads=None, air=None, handlers=None, lib=None, **series):
    """heat_air_species_check: everything about the air species of a series that needs no device (series arguments as
    HeatBatch.march_series; species: the arguments of make_air_species, or None; loads, air, handlers: the terms whose air the
    species ride on, checked as their own checks do). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(**series)
    l, lkeep = make_zone_loads(**loads) if loads is not None else (None, None)
    a, akeep = make_air_paths(**air) if air is not None else (None, None)
    h, hkeep = make_air_handlers(**handlers) if handlers is not None else (None, None)
    sp, spkeep = make_air_species(**species) if species is not None else (None, None)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    rc = L.heat_air_species_check(C.byref(desc), C.byref(s), ref(l), ref(a), ref(h), ref(sp))
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


OPENING_STATS = ("sum_v", "max_v", "step_max")
_OPENING_ROWS = (("zone_a", np.int32, True), ("zone_b", np.int32, True), ("temp_chan", np.int32, False), ("wind_chan", np.int32, False),
                 ("frac_chan", np.int32, False), ("out_chan", np.int32, True), ("area", np.float64, True), ("cw", np.float64, False),
                 ("cs", np.float64, False), ("ca", np.float64, False), ("c0", np.float64, False))


def make_openings(zone_a=(), zone_b=(), out_chan=(), area=(), temp_chan=None, wind_chan=None, frac_chan=None, cw=None, cs=None, ca=None,
                  c0=None, stats=OPENING_STATS, resume=None, step_base=0):
    """Builds a heat_openings. Returns (openings, keepalive); the march updates the accumulators in place.
    zone_a, zone_b   [n] the zones an opening joins; zone_b -1: outside air at the temperature of temp_chan
    out_chan         [n] the DERIVED channel the opening writes its volume flow into, m3/s: name it as the volume_chan of an air
                     path, of a flow of the zone loads or of a handler's branch
    area             [n] m2, the discharge coefficient folded in
    temp_chan        [n] the outside-air temperature where zone_b is -1, -1 elsewhere; None: no opening to outside
    wind_chan        [n] the effective wind speed at the opening, m/s; None / -1: no wind term
    frac_chan        [n] the open fraction, clamped to [0, 1]; None / -1: fully open
    cw, cs, ca, c0   [n] the coefficients of u^2, |dT| / Tm, |dT| and 1 under the root, each None = 0 (openings.wind_and_stack,
                     single_sided and doorway give them for three published forms)
    stats            names out of OPENING_STATS: which accumulators are maintained (default: all)
    resume           a dict of arrays a previous series returned: the accumulators start from them
    step_base        the number the first step of this series has in step_max
    (openings.apply and accumulate are the rule in numpy and take the same dict)"""
    given = dict(zone_a=zone_a, zone_b=zone_b, out_chan=out_chan, area=area, temp_chan=temp_chan, wind_chan=wind_chan,
                 frac_chan=frac_chan, cw=cw, cs=cs, ca=ca, c0=c0)
    unknown = set(stats or ()) - set(OPENING_STATS)
    if unknown:
        raise ValueError("openings: unknown stats %s (known: %s)" % (sorted(unknown), ", ".join(OPENING_STATS)))
    op = Openings()
    keep = {}
    n = len(np.asarray(zone_a if zone_a is not None else ()).reshape(-1))
    op.n_openings, op.resume, op.step_base = n, 0 if resume is None else 1, int(step_base)
    for name, dtype, needed in _OPENING_ROWS:
        if given[name] is None and not needed:
            continue
        v = np.ascontiguousarray(given[name] if given[name] is not None else (), dtype=dtype).reshape(-1)
        if v.shape != (n,):
            raise ValueError("openings %s: %s for %d openings" % (name, v.shape, n))
        keep[name] = v
        setattr(op, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if n else None)
    for name in (stats or ()):
        dtype = np.int64 if name == "step_max" else np.float64
        if resume is not None:
            if name not in resume:
                raise ValueError("openings resume: %s is missing" % name)
            a = np.array(resume[name], dtype=dtype)  # (a copy: the march writes it)
            if a.shape != (n,):
                raise ValueError("openings resume: %s of shape %s, not %s" % (name, a.shape, (n,)))
        else:
            a = np.zeros(n, dtype)  # (the library initialises on the device)
        keep[name] = a
        setattr(op, name, a.ctypes.data_as(_i64p if dtype == np.int64 else _dp) if a.size else None)
    return op, keep


def openings_check(md, openings, lib=None, **series):
    """heat_openings_check: everything about the openings of a series that needs no device (series arguments as
    HeatBatch.march_series; openings: the arguments of make_openings, or None). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(**series)
    op, okeep = make_openings(**openings) if openings is not None else (None, None)
    rc = L.heat_openings_check(C.byref(desc), C.byref(s), C.byref(op) if op is not None else None)
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


CONTROLLER_STATE = ("integral", "tripped")
CONTROLLER_STATS = ("sum_u", "sum_out", "steps_on", "steps_sat", "trips")
_CONTROLLER_ROWS = (("sense_kind", np.int32, False), ("sense_index", np.int32, True), ("sense_node", np.int32, False),
                    ("set_chan", np.int32, True), ("action", np.int32, False), ("en_chan", np.int32, False), ("lim_kind", np.int32, False),
                    ("lim_index", np.int32, False), ("lim_node", np.int32, False), ("out_chan", np.int32, True), ("kp", np.float64, True),
                    ("ki", np.float64, False), ("bias", np.float64, False), ("out_lo", np.float64, False), ("out_hi", np.float64, True),
                    ("lim_hi", np.float64, False), ("lim_lo", np.float64, False))
_CONTROLLER_ACC_DTYPE = dict(integral=np.float64, tripped=np.uint8, sum_u=np.float64, sum_out=np.float64, steps_on=np.int64,
                             steps_sat=np.int64, trips=np.int64)


def make_controllers(sense_index=(), set_chan=(), out_chan=(), kp=(), out_hi=(), sense_kind=None, sense_node=None, action=None, en_chan=None,
                     lim_kind=None, lim_index=None, lim_node=None, ki=None, bias=None, out_lo=None, lim_hi=None, lim_lo=None,
                     state=CONTROLLER_STATE, stats=CONTROLLER_STATS, resume=None):
    """Builds a heat_controllers. Returns (controllers, keepalive); the march updates the state and the accumulators in place.
    sense_kind       [n] 0: a zone's air, 1: a node of a surface, 2: a channel; None: all 0
    sense_index      [n] the zone, the surface or the channel
    sense_node       [n] kind 1: the node, -1 the surface's last; None: all -1
    set_chan         [n] the setpoint's channel
    action           [n] > 0 heating (e = setpoint - sensed), else cooling; None: all +1
    en_chan          [n] enabled where its value is > 0; None / -1: always
    lim_kind, lim_index, lim_node, lim_hi, lim_lo
                     [n] a high-limit cut-out on a temperature named as the sensed one is: u = 0 from above lim_hi until below
                     lim_lo; lim_kind None / -1: none
    out_chan         [n] the DERIVED channel the controller writes out_lo + u (out_hi - out_lo) into: name it as the channel of a
                     gain of the zone loads, of the room radiation, of an opening's frac_chan, of an air path's volume, or of
                     a side's driven solar input (controllers.embed)
    kp, ki, bias     [n] u = clamp(kp e + I + bias), I = clamp(I + ki e), both to [0, 1]; ki per step; ki, bias None = 0
                     (controllers.proportional and pi give them)
    out_lo, out_hi   [n] the output at u = 0 (None: 0) and at u = 1
    state            names out of CONTROLLER_STATE that are returned (the device keeps both either way)
    stats            names out of CONTROLLER_STATS: which accumulators are maintained (default: all)
    resume           a dict of arrays a previous series returned: the state and the accumulators start from them
    (controllers.apply and accumulate are the rule in numpy and take the same dict)"""
    given = dict(sense_kind=sense_kind, sense_index=sense_index, sense_node=sense_node, set_chan=set_chan, action=action, en_chan=en_chan,
                 lim_kind=lim_kind, lim_index=lim_index, lim_node=lim_node, out_chan=out_chan, kp=kp, ki=ki, bias=bias, out_lo=out_lo,
                 out_hi=out_hi, lim_hi=lim_hi, lim_lo=lim_lo)
    unknown = set(stats or ()) - set(CONTROLLER_STATS) | set(state or ()) - set(CONTROLLER_STATE)
    if unknown:
        raise ValueError("controllers: unknown state or stats %s (known: %s)" % (sorted(unknown), ", ".join(CONTROLLER_STATE + CONTROLLER_STATS)))
    ct = Controllers()
    keep = {}
    n = len(np.asarray(sense_index if sense_index is not None else ()).reshape(-1))
    ct.n_controllers, ct.resume = n, 0 if resume is None else 1
    for name, dtype, needed in _CONTROLLER_ROWS:
        if given[name] is None and not needed:
            continue
        v = np.ascontiguousarray(given[name] if given[name] is not None else (), dtype=dtype).reshape(-1)
        if v.shape != (n,):
            raise ValueError("controllers %s: %s for %d controllers" % (name, v.shape, n))
        keep[name] = v
        setattr(ct, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if n else None)
    for name in tuple(state or ()) + tuple(stats or ()):
        dtype = _CONTROLLER_ACC_DTYPE[name]
        if resume is not None:
            if name not in resume:
                raise ValueError("controllers resume: %s is missing" % name)
            a = np.array(resume[name], dtype=dtype)  # (a copy: the march writes it)
            if a.shape != (n,):
                raise ValueError("controllers resume: %s of shape %s, not %s" % (name, a.shape, (n,)))
        else:
            a = np.zeros(n, dtype)  # (the library initialises on the device)
        keep[name] = a
        setattr(ct, name, a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if a.size else None)
    return ct, keep


def controllers_check(md, controllers, openings=None, lib=None, **series):
    """heat_controllers_check: everything about the controllers of a series, and about them beside its openings, that needs no
    device (series arguments as HeatBatch.march_series; controllers, openings: the arguments of make_controllers and
    make_openings, or None). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(**series)
    op, okeep = make_openings(**openings) if openings is not None else (None, None)
    ct, ckeep = make_controllers(**controllers) if controllers is not None else (None, None)
    rc = L.heat_controllers_check(C.byref(desc), C.byref(s), C.byref(op) if op is not None else None, C.byref(ct) if ct is not None else None)
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


NETWORK_STATE = ("pressure",)
NETWORK_STATS = ("sum_ab", "sum_ba", "iters_sum", "unconverged", "max_res")
# (name, dtype, needed, over): over 0 the networks, 1 the nodes, 2 the links
_NETWORK_ROWS = (("tol", np.float64, True, 0), ("max_iter", np.int32, True, 0), ("g_min", np.float64, True, 0),
                 ("node_zone", np.int32, True, 1), ("src_chan", np.int32, False, 1), ("src_gain", np.float64, False, 1),
                 ("zone_a", np.int32, True, 2), ("zone_b", np.int32, True, 2), ("temp_chan", np.int32, True, 2), ("wp_chan", np.int32, False, 2),
                 ("frac_chan", np.int32, False, 2), ("out_ab", np.int32, False, 2), ("out_ba", np.int32, False, 2), ("c", np.float64, True, 2),
                 ("gh", np.float64, False, 2), ("p_lin", np.float64, True, 2), ("wp_gain", np.float64, False, 2))
_NETWORK_ACC = dict(pressure=(np.float64, 1), sum_ab=(np.float64, 2), sum_ba=(np.float64, 2), iters_sum=(np.int64, 0), unconverged=(np.int64, 0),
                    max_res=(np.float64, 0))


def make_air_networks(net_offset=(0,), tol=(), max_iter=(), g_min=(), node_zone=(), zone_a=(), zone_b=(), temp_chan=(), c=(), p_lin=(),
                      src_chan=None, src_gain=None, wp_chan=None, frac_chan=None, out_ab=None, out_ba=None, gh=None, wp_gain=None,
                      state=NETWORK_STATE, stats=NETWORK_STATS, resume=None):
    """Builds a heat_air_networks. Returns (networks, keepalive); the march updates the state and the accumulators in place.
    net_offset       [n_networks + 1] network w owns the nodes net_offset[w] ... net_offset[w + 1] - 1; 1 to 64 nodes each
    tol, max_iter, g_min
                     [n_networks] the residual, kg/s, at which a solve stops; the most iterations, 1 ... 64; the conductance of
                     every node to the datum, kg/s per Pa, > 0
    node_zone        [n_nodes] the zone of every node; a zone is in at most one network
    src_chan, src_gain
                     [n_nodes] a net mechanical mass inflow src_gain * row[src_chan], kg/s (an extract fan is negative); None /
                     -1: none; src_gain None = 1
    zone_a, zone_b   [n_links] the link's zones; zone_b -1: outside
    temp_chan        [n_links] the outside temperature's channel where zone_b is -1, else -1
    wp_chan, wp_gain [n_links] outside links: the wind pressure at the link, wp_gain * row[wp_chan] Pa; None / -1: none
    frac_chan        [n_links] the open fraction, clamped to [0, 1] (it may be a controller's output); None / -1: 1
    out_ab, out_ba   [n_links] the DERIVED channels the link's volume flow a -> b and b -> a is written into; None / -1: none
                     (air_networks.paths names the air paths that read them)
    c, gh, p_lin     [n_links] the flow coefficient, m3/s per sqrt(Pa) (air_networks.orifice, tall_opening); 9.81 times the
                     link's height above the network's datum (None = 0); the pressure difference below which the law is linear
    state            names out of NETWORK_STATE that are returned (the device keeps the pressures either way)
    stats            names out of NETWORK_STATS: which accumulators are maintained (default: all)
    resume           a dict of arrays a previous series returned: the state and the accumulators start from them
    (air_networks.apply and accumulate are the rule in numpy and take the same dict)"""
    given = dict(tol=tol, max_iter=max_iter, g_min=g_min, node_zone=node_zone, src_chan=src_chan, src_gain=src_gain, zone_a=zone_a, zone_b=zone_b,
                 temp_chan=temp_chan, wp_chan=wp_chan, frac_chan=frac_chan, out_ab=out_ab, out_ba=out_ba, c=c, gh=gh, p_lin=p_lin, wp_gain=wp_gain)
    unknown = set(stats or ()) - set(NETWORK_STATS) | set(state or ()) - set(NETWORK_STATE)
    if unknown:
        raise ValueError("air networks: unknown state or stats %s (known: %s)" % (sorted(unknown), ", ".join(NETWORK_STATE + NETWORK_STATS)))
    nw = AirNetworks()
    keep = {}
    off = np.ascontiguousarray(net_offset if net_offset is not None else (0,), dtype=np.int32).reshape(-1)
    if off.size == 0:
        off = np.zeros(1, np.int32)
    n = (len(off) - 1, len(np.asarray(node_zone if node_zone is not None else ()).reshape(-1)),
         len(np.asarray(zone_a if zone_a is not None else ()).reshape(-1)))
    what = ("networks", "nodes", "links")
    nw.n_networks, nw.n_nodes, nw.n_links = n
    nw.resume = 0 if resume is None else 1
    keep["net_offset"] = off
    nw.net_offset = off.ctypes.data_as(_i32p)
    for name, dtype, needed, over in _NETWORK_ROWS:
        if given[name] is None and not needed:
            continue
        v = np.ascontiguousarray(given[name] if given[name] is not None else (), dtype=dtype).reshape(-1)
        if v.shape != (n[over],):
            raise ValueError("air networks %s: %s for %d %s" % (name, v.shape, n[over], what[over]))
        keep[name] = v
        setattr(nw, name, v.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if v.size else None)
    for name in tuple(state or ()) + tuple(stats or ()):
        dtype, over = _NETWORK_ACC[name]
        if resume is not None:
            if name not in resume:
                raise ValueError("air networks resume: %s is missing" % name)
            a = np.array(resume[name], dtype=dtype)  # (a copy: the march writes it)
            if a.shape != (n[over],):
                raise ValueError("air networks resume: %s of shape %s, not %s" % (name, a.shape, (n[over],)))
        else:
            a = np.zeros(n[over], dtype)  # (the library initialises on the device)
        keep[name] = a
        setattr(nw, name, a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))) if a.size else None)
    return nw, keep


def air_networks_check(md, networks, openings=None, controllers=None, lib=None, **series):
    """heat_air_networks_check: everything about the air networks of a series, and about them beside its openings and
    controllers, that needs no device (series arguments as HeatBatch.march_series; networks, openings, controllers: the
    arguments of make_air_networks, make_openings and make_controllers, or None). Host-only."""
    L = lib or load_library()
    desc, keep = make_desc(md)
    s, skeep = make_series(**series)
    op, okeep = make_openings(**openings) if openings is not None else (None, None)
    ct, ckeep = make_controllers(**controllers) if controllers is not None else (None, None)
    nw, nkeep = make_air_networks(**networks) if networks is not None else (None, None)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    rc = L.heat_air_networks_check(C.byref(desc), C.byref(s), ref(op), ref(ct), ref(nw))
    if rc != 0:
        raise HeatError(rc, L.heat_last_error().decode("utf-8", "replace"))


def comm_available():
    """Whether the library can load RCCL (no collective inside: vote on it before comm_init)."""
    return load_library().heat_comm_available() == 0


def comm_unique_id():
    """ncclGetUniqueId through the library (128 bytes). One rank calls it and hands the bytes to the others."""
    buf = (C.c_uint8 * 128)()
    _check(load_library().heat_comm_unique_id(buf))
    return bytes(buf)


def _zone_rows_fit(keep, n_zones):
    for k in ("zone_a0", "zone_b0"):
        if k in keep and keep[k].shape[1] != n_zones:
            raise ValueError("%s: rows of %d for %d zones" % (k, keep[k].shape[1], n_zones))


class HeatBatch:
    """Device-resident batch of surfaces + zones (≙ ThermalModel, src/model.rs:54-77)."""

    def __init__(self, md, device=-1, force_general=False, nodes_per_lane=0, use_graph=False, stream=None,
                 n_ranks=1, rank=0, no_palette=False, no_fusion=False, fuse_always=False, rank_of_surface=None,
                 sites=None, n_sites=None, ideal_resident=False):
        """rank_of_surface (heat_partition's result): the batch holds the surfaces of `rank` only, picked from the
        whole model's dict by the library (heat_batch_create_shard).
        sites (modeldict.concat's site_of_surface): a batch of weather sites (heat_batch_create_sites), n_sites of them
        (default: max(sites) + 1); its marches then take weather [n_sub, n_sites, 3].
        ideal_resident: set_ideal_resident(True) on the new batch (no option of the descriptor: a setting of the batch)."""
        self._L = load_library()
        self._h = _H()
        desc, keep = make_desc(md)
        opt = make_options(device, force_general, nodes_per_lane, use_graph, stream, n_ranks, rank, no_palette,
                           no_fusion, fuse_always)
        self.n_sites = 1
        if sites is not None:
            assert rank_of_surface is None, "a batch of weather sites cannot be sharded"
            sos = np.ascontiguousarray(sites, dtype=np.int32)
            if n_sites is None:
                n_sites = int(sos.max()) + 1 if len(sos) else 1
            _check(self._L.heat_batch_create_sites(C.byref(desc), C.byref(opt), int(n_sites), sos.ctypes.data_as(_i32p),
                                                   C.byref(self._h)))
            self.n_sites = int(self._L.heat_batch_n_sites(self._h))
        elif rank_of_surface is None:
            _check(self._L.heat_batch_create_ex(C.byref(desc), C.byref(opt), C.byref(self._h)))
        else:
            ros = np.ascontiguousarray(rank_of_surface, dtype=np.int32)
            assert len(ros) == int(md["n_surfaces"])
            _check(self._L.heat_batch_create_shard(C.byref(desc), C.byref(opt), ros.ctypes.data_as(_i32p),
                                                   C.byref(self._h)))
        self.n_state = int(md["n_state"])
        self.n_zones = int(md["n_zones"])
        self.n_surfaces = int(md["n_surfaces"])
        # (the default normals of a sky: the model's own; of a shard's batch they are the whole model's, like every array)
        self._normals = tuple(np.array(a, dtype=np.float64) for a in _model_normals(md))
        if ideal_resident:
            self.set_ideal_resident(True)

    def close(self):
        if getattr(self, "_h", None):
            self._L.heat_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def _state_ptr(state):
        assert state.dtype == np.float64 and state.flags.c_contiguous
        return state.ctypes.data_as(_dp)

    @staticmethod
    def _opt(a):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a, a.ctypes.data_as(_dp)

    def upload_state(self, state):
        _check(self._L.heat_batch_upload_state(self._h, self._state_ptr(state), state.size))

    def upload_inputs(self, state):
        _check(self._L.heat_batch_upload_inputs(self._h, self._state_ptr(state), state.size))

    def download_state(self, state):
        _check(self._L.heat_batch_download_state(self._h, self._state_ptr(state), state.size))

    OUT_NODES, OUT_SCALARS, OUT_ZONES, OUT_ALL = 1, 2, 4, 7

    def march(self, state, weather, zone_a0=None, zone_b0=None, outputs=None):
        """≙ ThermalModel::march: len(weather) sub-timesteps, in place on ``state``. ``outputs``: which of this
        path's outputs are written back (OUT_* bits; default all)."""
        w, n = as_weather(weather, self.n_sites)
        a0, pa = self._opt(zone_a0)
        b0, pb = self._opt(zone_b0)
        if outputs is None:
            _check(self._L.heat_batch_march(self._h, self._state_ptr(state), state.size, w, n, pa, pb))
        else:
            _check(self._L.heat_batch_march_ex(self._h, self._state_ptr(state), state.size, w, n, pa, pb, int(outputs)))

    def download_outputs(self, state, outputs):
        _check(self._L.heat_batch_download_outputs(self._h, self._state_ptr(state), state.size, int(outputs)))

    def march_resident(self, weather, zone_a0=None, zone_b0=None):
        w, n = as_weather(weather, self.n_sites)
        a0, pa = self._opt(zone_a0)
        b0, pb = self._opt(zone_b0)
        _check(self._L.heat_batch_march_resident(self._h, w, n, pa, pb))

    def synchronize(self):
        _check(self._L.heat_batch_synchronize(self._h))

    def march_series(self, weather, n_sub, loads=None, report=None, trace=True, applied=True, ideal=None, sky=None, gains=None,
                     air=None, path_q=True, shades=None, sunlit=True, radiation=None, irradiance=True, ambient=None, ambient_t=True,
                     blinds=None, position=True, blind_incident=True, aniso=None, comfort=None, operative=True, mrt=True,
                     handlers=None, supply_t=True, recovered=True, coil_q=True, branch_q=True, species=None, conc_rows=True,
                     vent_v=True, vent_q=True, openings=None, opening_v=True, controllers=None, control_u=True, control_out=True, networks=None,
                     link_q=True, node_p=True, net_iters=True, **series):
        """heat_batch_march_series: n_steps caller timesteps of n_sub sub-timesteps in one call, inputs driven from
        schedules on the device (make_series names the arguments). Returns (trace [n_steps, n_probes], failed_step);
        a numerical failure raises HeatError carrying ``failed_step`` and the ``trace`` so far.
        loads (a dict of make_zone_loads' arguments: gains, flows, thermostats): heat_batch_march_series_loads — the zones'
        gains, air flows and thermostats formed on the device at every step. Returns (trace, failed_step,
        applied [n_steps, n_thermostats], modes [n_thermostats]: pass them as thermostats["mode"] to the next series).
        report (a dict of make_report's arguments: groups, stats, limits, thermostat_stats, group_trace, resume, step_base):
        heat_batch_march_series_report — statistics and group sums maintained on the device. The report's arrays (a dict of
        numpy arrays: q_min, th_switches, group_trace, ...; pass it as resume to the next series) are returned as one more
        element. With a report, trace=False / applied=False record no trace / applied powers: an empty array comes back.
        ideal (a dict of make_ideal_loads' arguments: zone, heat_chan, cool_chan, heat_cap, cool_cap, stats, resume, step_base):
        heat_batch_march_series_ideal — zones held at their setpoints in every sub-timestep. Returns a dict: trace, failed_step,
        ideal_q [n_steps, n_loads] (the step's sum of the power over its sub-timesteps; / n_sub: the mean power in W),
        ideal (the accumulators: pass it as resume to the next series), and with loads applied and modes, with a report
        report.
        sky (a dict of make_sky's arguments: record [n_steps, n_sites, 8], mode, normals — default: the model's normal_x,
        normal_y, cos_tilt): heat_batch_march_series_sky — the solar and long-wave irradiance of the sides the mode bytes
        name, formed on the device from one record per site and step. Returns what the same call without sky returns.
        gains (a dict of make_solar_gains' arguments; sky carries the records, its mode may be left out):
        heat_batch_march_series_gains — the solar radiation the apertures transmit, onto the receiving sides. Returns what the
        same call without gains returns plus transmitted [n_steps, n_apertures] and ap_sum [n_apertures] (pass it as
        gains["ap_sum"] to the next series): two more elements of the tuple, or two more keys of the dict.
        air (a dict of make_air_paths' arguments: target, source, temp_chan, volume_chan, volume_gain, open_chan, sense, band,
        min_delta, state, sum_q, steps_open, switches, stats): heat_batch_march_series_air — air that moves between zones and
        controlled vents, formed on the device at every step from the zone temperatures it holds. Returns what the same call
        without air returns plus one dict: path_q [n_steps, n_paths] (empty with path_q=False), state, and of sum_q,
        steps_open, switches those in stats (pass state and them on to the next series) — one more element of the tuple, or
        the key "air" of the dict.
        shades (a dict of make_shades' arguments; sky carries the records and the mode bits of the shaded sides, gains the
        shaded apertures): heat_batch_march_series_shaded — the sunlit fraction of overhangs, fins and horizons, formed on the
        device at every step. Returns what the same call without shades returns plus sunlit [n_steps, n_shades] (empty with
        sunlit=False): one more element of the tuple, or the key "sunlit" of the dict.
        radiation (a dict of make_room_radiation's arguments): heat_batch_march_series_radiation — the long-wave irradiance of
        the faces of a room from the emission of the faces they see, formed on the device at every step from the temperatures
        it holds. Returns what the same call without radiation returns plus irradiance [n_steps, n_receivers] (empty with
        irradiance=False) and sum_irradiance [n_receivers] (pass it as radiation["sum_irradiance"] to the next series): two
        more elements of the tuple, or two more keys of the dict.
        ambient (a dict of make_ambient's arguments; an empty dict: a drive without sides): heat_batch_march_series_ambient —
        the temperature of Ambient sides from a channel, a gain and an offset, and optionally mixed with a zone temperature
        the device holds, formed on the device at every step. Returns what the same call without ambient returns plus
        ambient_t [n_steps, n_sides] (empty with ambient_t=False) and sum_temperature [n_sides] (pass it as
        ambient["sum_temperature"] to the next series): two more elements of the tuple, or two more keys of the dict.
        blinds (a dict of make_blinds' arguments; an empty dict: no blind; shades carries the shades they ride on):
        heat_batch_march_series_blinds — movable solar protection, closed by the irradiance on the shade's plane and a zone
        temperature the device holds, or following a position channel, formed on the device at every step. Returns what the
        same call without blinds returns plus one dict: position and incident [n_steps, n_blinds] (empty with position=False /
        blind_incident=False), state, and of steps_closed, switches, sum_position those in stats (pass state and them on to the
        next series) — one more element of the tuple, or the key "blinds" of the dict.
        aniso (a dict of make_sky_aniso's arguments: coef [n_steps, n_sites, 2], front_band, back_band, aperture_band,
        shade_band): an anisotropic sky — every sky-driven solar side, aperture and blind takes the diffuse radiation by the
        caller's circumsolar and horizon coefficients (heat_sky_aniso). The call then goes through
        heat_batch_march_series_call, the entry point that takes every term in one struct (an empty dict: that entry point
        without an anisotropic sky). Returns what the same call without aniso returns: anisotropy has no output of its own.
        comfort (a dict of make_comfort's arguments; an empty dict: no sensor): heat_batch_march_series_comfort — operative
        temperatures of rooms from the face and zone temperatures the device holds at the start of every step, accumulated
        against limits that are channels and, where a sensor has its control bit, sensed by thermostats, air paths and blinds in
        place of the zone temperature. Returns what the same call without comfort returns plus one dict: operative and mrt
        [n_steps, n_sensors] (empty with operative=False / mrt=False) and of COMFORT_STATS those in stats (pass them as
        comfort["resume"] to the next series) — one more element of the tuple, or the key "comfort" of the dict.
        handlers (a dict of make_air_handlers' arguments; an empty dict: no unit): heat_batch_march_series_handlers —
        ventilation units with heat recovery, a bypass and supply-air coils, formed on the device at every step from the zone
        air temperatures it holds. Returns what the same call without handlers returns plus one dict: supply_t, recovered,
        coil_q [n_steps, n_units] and branch_q [n_steps, n_branches] (each empty with its flag False), bypass, and of
        HANDLER_STATS those in stats (pass bypass and them on to the next series) — one more element of the tuple, or the key
        "handlers" of the dict.
        species (a dict of make_air_species' arguments; an empty dict: no species): heat_batch_march_series_species —
        concentrations per species and zone carried by every flow of air of the series (the loads' flows, the open air paths,
        the handlers' supply branches) and demand vents whose volume flow follows a concentration, stepped on the device.
        Returns what the same call without species returns plus one dict, appended last: conc_rows [n_steps, n_species,
        n_zones], vent_v, vent_q [n_steps, n_vents] (each empty with its flag False), conc (the concentrations after the last
        step) and of SPECIES_STATS those in stats (pass conc on, and the stats as species["resume"] with step_base, to the
        next series) — one more element of the tuple, or the key "species" of the dict.
        openings (a dict of make_openings' arguments; an empty dict: no opening): heat_batch_march_series_openings — the
        volume flows that wind and buoyancy drive through openings, formed on the device at the head of every step from the
        zone air temperatures it holds and written into DERIVED channels, which the air paths, the loads' flows, the handlers'
        branches and the species read as any channel. Returns what the same call without openings returns plus one dict,
        appended last: opening_v [n_steps, n_openings] (empty with opening_v=False) and of OPENING_STATS those in stats (pass
        them as openings["resume"] with step_base to the next series) — one more element of the tuple, or the key "openings"
        of the dict.
        controllers (a dict of make_controllers' arguments; an empty dict: no controller): heat_batch_march_series_controllers
        — modulating control loops, evaluated on the device as the first kernel of every step from the zone and node
        temperatures it holds and written into DERIVED channels, which the zone loads' gains, the room radiation, the
        openings' fractions, the air paths and the driven inputs of the sides read as any channel. Returns what the same call
        without controllers returns plus one dict, appended last: control_u, control_out [n_steps, n_controllers] (each empty
        with its flag False), of CONTROLLER_STATE those in state and of CONTROLLER_STATS those in stats (pass them as
        controllers["resume"] to the next series) — one more element of the tuple, or the key "controllers" of the dict.
        networks (a dict of make_air_networks' arguments; an empty dict: no network): heat_batch_march_series_networks — per step
        and per network the device solves the node pressures that balance the mass flows through all links, behind the
        openings, and writes every link's volume flow into DERIVED channels, which the air paths read as any channel
        (air_networks.paths). Returns what the same call without networks returns plus one dict, appended last: link_q
        [n_steps, n_links], node_p [n_steps, n_nodes], net_iters [n_steps, n_networks] (each empty with its flag False), of
        NETWORK_STATE those in state and of NETWORK_STATS those in stats (pass them as networks["resume"] to the next series)
        — one more element of the tuple, or the key "networks" of the dict."""
        given = dict(loads=loads, report=report, ideal=ideal, sky=sky, gains=gains, air=air, shades=shades, radiation=radiation,
                     ambient=ambient, blinds=blinds)
        # The gains read the sky's records, and so do shades whose sky names no side: such a call gets a sky without mode bits.
        # (One condition for every entry point: without shades it is "gains is not None", and with gains it holds whatever
        # the shades and the sky are — the spellings this had per entry point all reduce to it.)
        if gains is not None or (shades is not None and (sky is None or sky.get("mode") is None)):
            given["sky"] = _sky_for_gains(sky, self._normals, self.n_surfaces)
        return self._march_series(weather, n_sub, series, given, dict(trace=trace, applied=applied, path_q=path_q, sunlit=sunlit,
                                                                      irradiance=irradiance, ambient_t=ambient_t, position=position,
                                                                      blind_incident=blind_incident, operative=operative, mrt=mrt,
                                                                      supply_t=supply_t, recovered=recovered, coil_q=coil_q,
                                                                      branch_q=branch_q, conc_rows=conc_rows, vent_v=vent_v,
                                                                      vent_q=vent_q, opening_v=opening_v, control_u=control_u,
                                                                      control_out=control_out, link_q=link_q, node_p=node_p,
                                                                      net_iters=net_iters),
                                  aniso=aniso, comfort=comfort, handlers=handlers, species=species, openings=openings,
                                  controllers=controllers, networks=networks)

    # The eleven entry points, widest last: the symbol and the optional terms it carries. A call goes to the narrowest that carries
    # what was passed; its arguments are _SERIES_ORDER (the header's order) cut down to those terms and their arrays.
    _SERIES_ENTRY = (("heat_batch_march_series", ()),
                     ("heat_batch_march_series_loads", ("loads",)),
                     ("heat_batch_march_series_report", ("loads", "report")),
                     ("heat_batch_march_series_ideal", ("loads", "report", "ideal")),
                     ("heat_batch_march_series_sky", ("loads", "report", "ideal", "sky")),
                     ("heat_batch_march_series_gains", ("loads", "report", "ideal", "sky", "gains")),
                     ("heat_batch_march_series_air", ("loads", "report", "ideal", "sky", "gains", "air")),
                     ("heat_batch_march_series_shaded", ("loads", "report", "ideal", "sky", "gains", "air", "shades")),
                     ("heat_batch_march_series_radiation", ("loads", "report", "ideal", "sky", "gains", "air", "shades", "radiation")),
                     ("heat_batch_march_series_ambient", ("loads", "report", "ideal", "sky", "gains", "air", "shades", "radiation",
                                                          "ambient")),
                     ("heat_batch_march_series_blinds", ("loads", "report", "ideal", "sky", "gains", "air", "shades", "radiation",
                                                         "ambient", "blinds")))
    _SERIES_ORDER = ("sky", "shades", "gains", "loads", "air", "ideal", "report", "trace", "applied", "ideal_q", "transmitted", "path_q",
                     "sunlit", "radiation", "irradiance", "ambient", "ambient_t", "blinds", "position", "blind_incident")
    # term -> (its make_* function, the array of rows it returns, the count of that array's columns); the blinds return a
    # second array of rows of the same width, blind_incident
    _SERIES_TERMS = dict(loads=(make_zone_loads, "applied", "n_thermostats"), ideal=(make_ideal_loads, "ideal_q", "n_loads"),
                         gains=(make_solar_gains, "transmitted", "n_apertures"), air=(make_air_paths, "path_q", "n_paths"),
                         shades=(make_shades, "sunlit", "n_shades"), radiation=(make_room_radiation, "irradiance", "n_receivers"),
                         ambient=(make_ambient, "ambient_t", "n_sides"), blinds=(make_blinds, "position", "n_blinds"))

    def _march_series(self, weather, n_sub, series, given, want, aniso=None, comfort=None, handlers=None, species=None, openings=None,
                      controllers=None, networks=None):
        """march_series behind its arguments: given maps every optional term to its dict or None, want the arrays of rows to
        whether they are recorded; aniso: the dict of make_sky_aniso's arguments or None; comfort: the dict of make_comfort's
        arguments or None; handlers: the dict of make_air_handlers' arguments or None; species: the dict of make_air_species'
        arguments or None; openings: the dict of make_openings' arguments or None; controllers: the dict of make_controllers'
        arguments or None; networks: the dict of make_air_networks' arguments or None."""
        if given["report"] is None and given["ideal"] is None and not (want["trace"] and want["applied"]):
            raise ValueError("trace=False / applied=False need a report")
        s, keep = make_series(weather, n_sub, n_sites=self.n_sites, **series)
        _series_arrays_fit(keep, self.n_surfaces)
        _zone_rows_fit(keep, self.n_zones)
        made, kept = {}, {}
        if given["sky"] is not None:
            sky = dict(given["sky"])
            if sky.get("normals") is None:
                sky["normals"] = self._normals
            made["sky"], kept["sky"] = make_sky(**sky)
            _sky_fits(kept["sky"], s.n_steps, self.n_sites, self.n_surfaces)
        rows = dict(trace=np.zeros((s.n_steps if want["trace"] else 0, s.n_probes)))

        def build(term):
            make, key, count = self._SERIES_TERMS[term]
            if given[term] is not None or term == "loads":
                made[term], kept[term] = make(**(given[term] or {}))
                rows[key] = np.zeros((s.n_steps if want.get(key, True) else 0, getattr(made[term], count)))

        # Built in the order the methods this replaces built them, so that input wrong in two places raises what it raised:
        # sky, loads, ideal loads, report, gains, air paths, shades, room radiation, ambient drive. The loads and the report are
        # built for every call, also for heat_batch_march_series, which takes neither: not passed they are empty and cannot
        # raise, and the report is sized by the loads' thermostats.
        build("loads")
        build("ideal")
        made["report"], kept["report"] = make_report(n_probes=s.n_probes, n_thermostats=made["loads"].n_thermostats, n_steps=s.n_steps,
                                                     **(given["report"] or {}))
        build("gains")
        build("air")
        build("shades")
        if given["shades"] is not None:
            _shades_fit(kept["shades"], self.n_surfaces, made["gains"].n_apertures if "gains" in made else None)
        build("radiation")
        build("ambient")
        build("blinds")
        if "position" in rows:
            rows["blind_incident"] = np.zeros((s.n_steps if want["blind_incident"] else 0, made["blinds"].n_blinds))
        symbol, carried = next(e for e in self._SERIES_ENTRY if all(v is None or k in e[1] for k, v in given.items()))
        # The symbol's arguments: of _SERIES_ORDER the names of the terms it carries (a struct, NULL where the term was not
        # passed), the arrays of rows of those terms and the trace, which every symbol has (an array, NULL where it is empty).
        term_of = {key: term for term, (_, key, _) in self._SERIES_TERMS.items()}       # the term an array of rows belongs to
        term_of["blind_incident"] = "blinds"
        args = []
        for name in self._SERIES_ORDER:
            is_struct = name in given
            if is_struct and name in carried:
                args.append(C.byref(made[name]) if given[name] is not None else None)
            elif not is_struct and (name == "trace" or term_of[name] in carried):
                args.append(rows[name].ctypes.data_as(_dp) if name in rows and rows[name].size else None)
        failed = C.c_int32(-1)
        if aniso is not None or comfort is not None or handlers is not None or species is not None or openings is not None or controllers is not None or networks is not None:
            # One struct, filled by name: the terms that were passed (the fields' names are the header's), the arrays of rows
            # that are recorded, and the anisotropic sky.
            call = SeriesCall(size=C.sizeof(SeriesCall), s=C.pointer(s), failed_step=C.pointer(failed))
            if aniso:
                an, akeep = make_sky_aniso(**aniso)
                _aniso_fits(akeep, s.n_steps, self.n_sites, self.n_surfaces, made["gains"].n_apertures if "gains" in made else None,
                            made["shades"].n_shades if "shades" in made else None)
                call.aniso = C.pointer(an)
            field = dict(loads="l", ideal="il", report="r")
            for term, v in given.items():
                if v is not None:
                    setattr(call, field.get(term, term), C.pointer(made[term]))
            for name, a in rows.items():
                if a.size:
                    setattr(call, name, a.ctypes.data_as(_dp))
            ptr = lambda a: a.ctypes.data_as(_dp) if a.size else None  # noqa: E731
            cf = None
            if comfort is not None:
                cf, ckeep = make_comfort(**comfort)
                top_rows = np.zeros((s.n_steps if want["operative"] else 0, cf.n_sensors))
                mrt_rows = np.zeros((s.n_steps if want["mrt"] else 0, cf.n_sensors))
            ah = None
            if handlers is not None:
                ah, hkeep = make_air_handlers(**handlers)
                hrows = {k: np.zeros((s.n_steps if want[k] else 0, ah.n_branches if k == "branch_q" else ah.n_units))
                         for k in ("supply_t", "recovered", "coil_q", "branch_q")}
            sp = None
            if species is not None:
                sp, spkeep = make_air_species(**species)
                if sp.n_species and spkeep["outdoor_chan"].shape[1] != self.n_zones:
                    raise ValueError("air species outdoor_chan: %d zones, the batch has %d" % (spkeep["outdoor_chan"].shape[1], self.n_zones))
                sprows = dict(conc_rows=np.zeros((s.n_steps if want["conc_rows"] else 0, sp.n_species, self.n_zones if sp.n_species else 0)),
                              vent_v=np.zeros((s.n_steps if want["vent_v"] else 0, sp.n_vents)),
                              vent_q=np.zeros((s.n_steps if want["vent_q"] else 0, sp.n_vents)))
            hp = [ptr(hrows[k]) for k in ("supply_t", "recovered", "coil_q", "branch_q")] if ah is not None else [None] * 4
            op = None
            if openings is not None:
                op, opkeep = make_openings(**openings)
                oprows = np.zeros((s.n_steps if want["opening_v"] else 0, op.n_openings))
            spp = [ptr(sprows[k]) for k in ("conc_rows", "vent_v", "vent_q")] if sp is not None else [None] * 3
            ct = None
            if controllers is not None:
                ct, ctkeep = make_controllers(**controllers)
                ctrows = {k: np.zeros((s.n_steps if want[k] else 0, ct.n_controllers)) for k in ("control_u", "control_out")}
            if networks is not None:
                nw, nwkeep = make_air_networks(**networks)
                nwrows = dict(link_q=np.zeros((s.n_steps if want["link_q"] else 0, nw.n_links)),
                              node_p=np.zeros((s.n_steps if want["node_p"] else 0, nw.n_nodes)),
                              net_iters=np.zeros((s.n_steps if want["net_iters"] else 0, nw.n_networks), np.int32))
                rc = self._L.heat_batch_march_series_networks(self._h, C.byref(call), C.byref(cf) if cf is not None else None,
                                                              ptr(top_rows) if cf is not None else None, ptr(mrt_rows) if cf is not None else None,
                                                              C.byref(ah) if ah is not None else None, *hp,
                                                              C.byref(sp) if sp is not None else None, *spp,
                                                              C.byref(op) if op is not None else None, ptr(oprows) if op is not None else None,
                                                              C.byref(ct) if ct is not None else None,
                                                              ptr(ctrows["control_u"]) if ct is not None else None,
                                                              ptr(ctrows["control_out"]) if ct is not None else None,
                                                              C.byref(nw), ptr(nwrows["link_q"]), ptr(nwrows["node_p"]),
                                                              nwrows["net_iters"].ctypes.data_as(_i32p) if nwrows["net_iters"].size else None)
            elif controllers is not None:
                rc = self._L.heat_batch_march_series_controllers(self._h, C.byref(call), C.byref(cf) if cf is not None else None,
                                                                 ptr(top_rows) if cf is not None else None, ptr(mrt_rows) if cf is not None else None,
                                                                 C.byref(ah) if ah is not None else None, *hp,
                                                                 C.byref(sp) if sp is not None else None, *spp,
                                                                 C.byref(op) if op is not None else None, ptr(oprows) if op is not None else None,
                                                                 C.byref(ct), ptr(ctrows["control_u"]), ptr(ctrows["control_out"]))
            elif openings is not None:
                rc = self._L.heat_batch_march_series_openings(self._h, C.byref(call), C.byref(cf) if cf is not None else None,
                                                              ptr(top_rows) if cf is not None else None, ptr(mrt_rows) if cf is not None else None,
                                                              C.byref(ah) if ah is not None else None, *hp,
                                                              C.byref(sp) if sp is not None else None, *spp, C.byref(op), ptr(oprows))
            elif species is not None:
                rc = self._L.heat_batch_march_series_species(self._h, C.byref(call), C.byref(cf) if cf is not None else None,
                                                             ptr(top_rows) if cf is not None else None, ptr(mrt_rows) if cf is not None else None,
                                                             C.byref(ah) if ah is not None else None, *hp, C.byref(sp), ptr(sprows["conc_rows"]),
                                                             ptr(sprows["vent_v"]), ptr(sprows["vent_q"]))
            elif handlers is not None:
                rc = self._L.heat_batch_march_series_handlers(self._h, C.byref(call), C.byref(cf) if cf is not None else None,
                                                              ptr(top_rows) if cf is not None else None, ptr(mrt_rows) if cf is not None else None,
                                                              C.byref(ah), ptr(hrows["supply_t"]), ptr(hrows["recovered"]), ptr(hrows["coil_q"]),
                                                              ptr(hrows["branch_q"]))
            elif comfort is not None:
                rc = self._L.heat_batch_march_series_comfort(self._h, C.byref(call), C.byref(cf), top_rows.ctypes.data_as(_dp) if top_rows.size else None,
                                                             mrt_rows.ctypes.data_as(_dp) if mrt_rows.size else None)
            else:
                rc = self._L.heat_batch_march_series_call(self._h, C.byref(call))
        else:
            rc = getattr(self._L, symbol)(self._h, C.byref(s), *args, C.byref(failed))
        if rc != 0:
            e = HeatError(rc, self._L.heat_last_error().decode("utf-8", "replace"))
            e.failed_step, e.trace = int(failed.value), rows["trace"]
            raise e
        # what is returned, in the order the terms were added to the call: a dict with ideal loads, else a tuple of the values
        out = [("trace", rows["trace"]), ("failed_step", int(failed.value))]
        if given["ideal"] is not None:
            out += [("ideal_q", rows["ideal_q"]), ("ideal", {k: kept["ideal"][k] for k in IDEAL_STATS if k in kept["ideal"]})]
        if given["loads"] is not None:
            out += [("applied", rows["applied"]), ("modes", kept["loads"].get("th_mode", np.zeros(0, np.uint8)))]
        if given["report"] is not None:
            out += [("report", {k: v for k, v in kept["report"].items() if not k.startswith("group_") or k == "group_trace"})]
        if given["gains"] is not None:
            out += [("transmitted", rows["transmitted"]), ("ap_sum", kept["gains"]["ap_sum"])]
        if given["air"] is not None:
            out += [("air", dict(path_q=rows["path_q"], **{k: kept["air"][k] for k in ("state",) + AIR_STATS if k in kept["air"]}))]
        if given["shades"] is not None:
            out += [("sunlit", rows["sunlit"])]
        if given["radiation"] is not None:
            out += [("irradiance", rows["irradiance"]), ("sum_irradiance", kept["radiation"]["sum_irradiance"])]
        if given["ambient"] is not None:
            out += [("ambient_t", rows["ambient_t"]), ("sum_temperature", kept["ambient"]["sum_temperature"])]
        if given["blinds"] is not None:
            out += [("blinds", dict(position=rows["position"], incident=rows["blind_incident"],
                                    **{k: kept["blinds"][k] for k in ("state",) + BLIND_STATS if k in kept["blinds"]}))]
        if comfort is not None:
            out += [("comfort", dict(operative=top_rows, mrt=mrt_rows, **{k: ckeep[k] for k in COMFORT_STATS if k in ckeep}))]
        if handlers is not None:
            out += [("handlers", dict(hrows, **{k: hkeep[k] for k in ("bypass",) + HANDLER_STATS if k in hkeep}))]
        if species is not None:
            out += [("species", dict(sprows, **{k: spkeep[k] for k in ("conc",) + SPECIES_STATS if k in spkeep}))]
        if openings is not None:
            out += [("openings", dict(opening_v=oprows, **{k: opkeep[k] for k in OPENING_STATS if k in opkeep}))]
        if controllers is not None:
            out += [("controllers", dict(ctrows, **{k: ctkeep[k] for k in CONTROLLER_STATE + CONTROLLER_STATS if k in ctkeep}))]
        if networks is not None:
            out += [("networks", dict(nwrows, **{k: nwkeep[k] for k in NETWORK_STATE + NETWORK_STATS if k in nwkeep}))]
        return dict(out) if given["ideal"] is not None else tuple(v for _, v in out)

    def set_ambient(self, surfaces, sides, temperatures):
        """heat_batch_set_ambient: the temperature (C) of the listed Ambient sides (surface of the model, 0 front / 1 back)
        from the next march on; durable until set again."""
        q = np.ascontiguousarray(surfaces, dtype=np.int64).reshape(-1)
        sd = np.ascontiguousarray(sides, dtype=np.uint8).reshape(-1)
        v = np.ascontiguousarray(temperatures, dtype=np.float64).reshape(-1)
        if not (q.shape == sd.shape == v.shape):
            raise ValueError("set_ambient: %d surfaces, %d sides, %d temperatures" % (q.size, sd.size, v.size))
        _check(self._L.heat_batch_set_ambient(self._h, q.size, q.ctypes.data_as(_i64p) if q.size else None,
                                              sd.ctypes.data_as(C.POINTER(C.c_uint8)) if q.size else None,
                                              v.ctypes.data_as(_dp) if q.size else None))

    def failed_surface(self):
        """(index, kind) of the first place the last reported numerical failure was seen; (-1, 0) if none."""
        i, k = C.c_int64(-1), C.c_int32(0)
        _check(self._L.heat_batch_failed_surface(self._h, C.byref(i), C.byref(k)))
        return int(i.value), int(k.value)

    def set_weather(self, weather, zone_a0=None, zone_b0=None):
        w, n = as_weather(weather, self.n_sites)
        a0, pa = self._opt(zone_a0)
        b0, pb = self._opt(zone_b0)
        _check(self._L.heat_batch_set_weather(self._h, w, n, pa, pb))

    def step_surfaces(self, sub_step):
        _check(self._L.heat_batch_step_surfaces(self._h, sub_step))

    def step_zones(self, gathered_ptr, n_blocks):
        _check(self._L.heat_batch_step_zones(self._h, gathered_ptr, n_blocks))

    def zone_partials_ptr(self):
        return self._L.heat_batch_zone_partials(self._h)

    def use_partials(self, dev_ptr):
        _check(self._L.heat_batch_use_partials(self._h, dev_ptr))

    def touched_zones(self):
        m = np.zeros(self.n_zones, dtype=np.uint8)
        _check(self._L.heat_batch_touched_zones(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8))))
        return m

    def set_shared_zones(self, shared_zone):
        sz = np.ascontiguousarray(shared_zone, dtype=np.int32)
        _check(self._L.heat_batch_set_shared_zones(self._h, sz.ctypes.data_as(_i32p), len(sz)))

    def comm_init(self, unique_id, extra_shared=None):
        """ncclCommInitRank with the 128-byte id of comm_unique_id() (collective: every rank calls it), then the
        ranks agree on the shared zones (plus ``extra_shared``, tests). After it the batch marches like a
        single-GPU one."""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        if extra_shared is None or len(extra_shared) == 0:
            _check(self._L.heat_batch_comm_init(self._h, buf))
        else:
            ex = np.ascontiguousarray(extra_shared, dtype=np.int32)
            _check(self._L.heat_batch_comm_init_ex(self._h, buf, ex.ctypes.data_as(_i32p), len(ex)))

    def set_owned_zones(self, owned):
        m = np.ascontiguousarray(owned, dtype=np.uint8)
        assert len(m) == self.n_zones
        _check(self._L.heat_batch_set_owned_zones(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8))))

    @property
    def n_shared_zones(self):
        return int(self._L.heat_batch_n_shared_zones(self._h))

    @property
    def comm_ranks(self):
        """Ranks of the batch's own RCCL communicator (0: none)."""
        return int(self._L.heat_batch_comm_ranks(self._h))

    def comm_destroy(self):
        _check(self._L.heat_batch_comm_destroy(self._h))

    def set_fusion(self, enabled):
        """Cluster-resident march on/off (off: every surface is streamed one sub-timestep per launch)."""
        _check(self._L.heat_batch_set_fusion(self._h, 1 if enabled else 0))

    def set_ideal_resident(self, enabled):
        """Opt-in, durable: ideal series of this batch keep its resident clusters resident (heat_ideal_loads, RESIDENT
        FORM) where the batch is eligible; otherwise, and by default, they march streamed."""
        _check(self._L.heat_batch_set_ideal_resident(self._h, 1 if enabled else 0))

    @property
    def ideal_resident(self):
        """1 when the next ideal series would march the resident clusters resident: the opt-in, fusion on, an eligible batch."""
        return int(self._L.heat_batch_ideal_resident(self._h))

    @property
    def n_fused_surfaces(self):
        return int(self._L.heat_batch_n_fused_surfaces(self._h))

    @property
    def n_fused_launches(self):
        return int(self._L.heat_batch_n_fused_launches(self._h))

    def set_timing(self, enabled):
        _check(self._L.heat_batch_set_timing(self._h, int(enabled)))  # (k > 1: every k-th streamed march call)

    def get_timing(self):
        a, b, n = _d(0), _d(0), C.c_int64(0)
        _check(self._L.heat_batch_get_timing(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    @property
    def n_surfaces_in_batch(self):
        """Surfaces this batch holds (a shard of the model when created with rank_of_surface)."""
        return int(self._L.heat_batch_n_surfaces(self._h))

    @property
    def algorithmic_bytes(self):
        return self._L.heat_batch_algorithmic_bytes(self._h)

    @property
    def n_nodes(self):
        return self._L.heat_batch_n_nodes(self._h)

    def nomass_iterations(self):
        return self._L.heat_batch_nomass_iterations(self._h)

    def class_counts(self):
        c = (C.c_int64 * 5)()
        _check(self._L.heat_batch_class_counts(self._h, c))
        return list(c)


# ---------------------------------------------------------------------------------------------------
# Setup-time half (include/heat_amd_setup.h)
def make_layers(layers):
    """list of dicts -> ctypes array of heat_layer. Keys: thickness, and either is_gas/gas or k, rho, cp;
    optional front_thermal_abs, back_thermal_abs (0.84), tau (0), front_solar_abs, back_solar_abs (0.84) —
    the defaults the reference applies when the substance does not define the property."""
    arr = (Layer * len(layers))()
    for i, L in enumerate(layers):
        arr[i].is_gas = 1 if L.get("is_gas") else 0
        arr[i].gas = int(L.get("gas", 0))
        arr[i].thickness = float(L["thickness"])
        arr[i].conductivity = float(L.get("k", 0.0))
        arr[i].density = float(L.get("rho", 0.0))
        arr[i].specific_heat = float(L.get("cp", 0.0))
        arr[i].front_thermal_absorbtance = float(L.get("front_thermal_abs", 0.84))
        arr[i].back_thermal_absorbtance = float(L.get("back_thermal_abs", 0.84))
        arr[i].solar_transmittance = float(L.get("tau", 0.0))
        arr[i].front_solar_absorbtance = float(L.get("front_solar_abs", 0.84))
        arr[i].back_solar_absorbtance = float(L.get("back_solar_abs", 0.84))
    return arr


def discretize(layers, model_dt, max_dx, min_dt, height=1.0, angle=0.0):
    """Discretization::new (reference src/discretization.rs:95-114) through the C ABI."""
    L = load_library()
    arr = make_layers(layers)
    n_layers = len(layers)
    n_el = (C.c_int32 * n_layers)()
    sub = L.heat_discretize_construction(n_layers, arr, model_dt, max_dx, min_dt, n_el)
    if sub < 0:
        raise HeatError(sub, "heat_discretize_construction failed")
    return build_segments(layers, list(n_el), height, angle, tstep_subdivision=sub)


def build_segments(layers, n_elements, height=1.0, angle=0.0, tstep_subdivision=1):
    L = load_library()
    arr = make_layers(layers)
    n_layers = len(layers)
    n_el = (C.c_int32 * n_layers)(*n_elements)
    n_nodes = L.heat_count_nodes(n_layers, n_el)
    mass = np.zeros(n_nodes)
    uval = np.zeros(n_nodes)
    segc = np.zeros(n_nodes, dtype=np.int32)
    cav = np.zeros(max(n_layers, 1), dtype=CAVITY_DTYPE)
    nc = L.heat_build_segments(n_layers, arr, n_el, height, angle, mass.ctypes.data_as(_dp), uval.ctypes.data_as(_dp),
                               segc.ctypes.data_as(_i32p), cav.ctypes.data_as(C.POINTER(Cavity)), 0)
    if nc < 0:
        raise HeatError(nc, "heat_build_segments failed")
    fa = np.zeros(n_nodes)
    ba = np.zeros(n_nodes)
    rc = L.heat_node_alphas(n_layers, arr, n_el, n_nodes, fa.ctypes.data_as(_dp), ba.ctypes.data_as(_dp))
    return dict(tstep_subdivision=tstep_subdivision, n_elements=list(n_elements), n_nodes=n_nodes, mass=mass,
                uvalue=uval, seg_cavity=segc, cavities=cav[:nc].copy(), front_alpha=fa, back_alpha=ba, alpha_rc=rc)


def get_chunks(mass):
    L = load_library()
    mass = np.ascontiguousarray(mass, dtype=np.float64)
    n = len(mass)
    nm, nn = C.c_int32(0), C.c_int32(0)
    mc = (C.c_int32 * (2 * n + 2))()
    nc = (C.c_int32 * (2 * n + 2))()
    _check(L.heat_get_chunks(n, mass.ctypes.data_as(_dp), C.byref(nm), mc, C.byref(nn), nc))
    return ([(mc[2 * i], mc[2 * i + 1]) for i in range(nm.value)],
            [(nc[2 * i], nc[2 * i + 1]) for i in range(nn.value)])


class ModelBuilder:
    """ThermalModel::new (reference src/model.rs:215-354) through the C ABI: zones + surfaces with their
    constructions in, the flattened model dict (heat_amd.modeldict) + initial SimulationState out."""

    def __init__(self, n_per_hour, terrain=-1):
        self._L = load_library()
        self._h = self._L.heat_model_builder_create(n_per_hour, terrain)
        if not self._h:
            raise HeatError(-1, "heat_model_builder_create failed")
        self._keep = []

    def close(self):
        if getattr(self, "_h", None):
            self._L.heat_model_builder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_zone(self, volume):
        return self._L.heat_model_builder_add_zone(self._h, float(volume))

    def add_surface(self, layers, area, perimeter, normal, centroid_z, front_kind, back_kind, front_zone=0,
                    back_zone=0, front_ambient=0.0, back_ambient=0.0, is_fenestration=False):
        arr = make_layers(layers)
        s = SurfaceIn()
        s.layers = arr
        s.n_layers = len(layers)
        s.is_fenestration = 1 if is_fenestration else 0
        s.area, s.perimeter, s.centroid_z = float(area), float(perimeter), float(centroid_z)
        for i in range(3):
            s.normal[i] = float(normal[i])
        s.front_kind, s.back_kind, s.front_zone, s.back_zone = int(front_kind), int(back_kind), int(front_zone), int(back_zone)
        s.front_ambient, s.back_ambient = float(front_ambient), float(back_ambient)
        rc = self._L.heat_model_builder_add_surface(self._h, C.byref(s))
        if rc < 0:
            raise HeatError(rc, "heat_model_builder_add_surface failed")
        return rc

    def finish(self):
        """Returns (model dict, initial state, dt_subdivisions)."""
        pd = C.POINTER(Desc)()
        ps = _dp()
        nsub = C.c_int32(0)
        rc = self._L.heat_model_builder_finish(self._h, C.byref(pd), C.byref(ps), C.byref(nsub))
        if rc != 0:
            raise HeatError(rc, "heat_model_builder_finish failed (the reference would panic or return Err here)")
        d = pd.contents
        S, Z, N = d.n_surfaces, d.n_zones, 0
        off = np.ctypeslib.as_array(d.node_offset, shape=(S + 1,)).copy()
        N = int(off[-1])

        def arr(p, n):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0)

        md = dict(n_surfaces=int(S), n_zones=int(Z), n_state=int(d.n_state), dt=float(d.dt), node_offset=off,
                  front_hs_fix=None, back_hs_fix=None, seg_cavity=None, cavities=None)
        for k in ("mass", "uvalue", "front_alpha", "back_alpha"):
            md[k] = arr(getattr(d, k), N)
        for k in _I32:
            md[k] = arr(getattr(d, k), S).astype(np.int32)
        for k in [x for x in _F64 if x not in ("mass", "uvalue", "front_alpha", "back_alpha", "zone_volume")]:
            md[k] = arr(getattr(d, k), S)
        for k in [x for x in _I64 if x not in ("node_offset", "zone_slot")]:
            md[k] = arr(getattr(d, k), S).astype(np.int64)
        md["zone_volume"] = arr(d.zone_volume, Z)
        md["zone_slot"] = arr(d.zone_slot, Z).astype(np.int64)
        if d.n_cavities:
            md["seg_cavity"] = arr(d.seg_cavity, N).astype(np.int32)
            cv = np.zeros(d.n_cavities, dtype=CAVITY_DTYPE)
            C.memmove(cv.ctypes.data, d.cavities, cv.nbytes)
            md["cavities"] = cv
        state = np.ctypeslib.as_array(ps, shape=(int(d.n_state),)).copy() if int(d.n_state) > 0 else np.zeros(0)
        return md, state, int(nsub.value)

    def surface_info(self, i):
        sub, nn = C.c_int32(0), C.c_int32(0)
        el = (C.c_int32 * 64)()
        n = self._L.heat_model_builder_surface_info(self._h, i, C.byref(sub), C.byref(nn), el, 64)
        return dict(tstep_subdivision=sub.value, n_nodes=nn.value, n_elements=list(el[:n]))
