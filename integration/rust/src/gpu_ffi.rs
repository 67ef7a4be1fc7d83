//! FFI declarations of include/heat_amd.h (ABI version 1) — `src/gpu_ffi.rs` of the `heat` crate, feature `gpu`.
//! Unverified: not compiled in this repository. Struct layouts are checked against the C header by
//! tests/test_abi_symbols.py (ctypes mirrors of the same structs vs gcc's offsetof).
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] pub struct HeatCavity { pub thickness: f64, pub height: f64, pub angle: f64,
                                   pub eout: f64, pub ein: f64, pub gas: i32, pub reserved: i32 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct HeatWeather { pub dry_bulb: f64, pub wind_direction: f64, pub wind_speed: f64 }
#[repr(C)] pub struct HeatBatchDesc {
    pub abi_version: i32, pub reserved: i32,
    pub n_surfaces: i64, pub n_zones: i64, pub n_cavities: i64, pub n_state: i64, pub dt: f64,
    pub node_offset: *const i64, pub mass: *const f64, pub uvalue: *const f64, pub seg_cavity: *const i32,
    pub front_alpha: *const f64, pub back_alpha: *const f64, pub cavities: *const HeatCavity,
    pub front_kind: *const i32, pub back_kind: *const i32, pub front_zone: *const i32, pub back_zone: *const i32,
    pub front_ambient: *const f64, pub back_ambient: *const f64,
    pub front_emissivity: *const f64, pub back_emissivity: *const f64,
    pub area: *const f64, pub perimeter: *const f64, pub cos_tilt: *const f64,
    pub normal_x: *const f64, pub normal_y: *const f64, pub wind_modifier: *const f64,
    pub front_hs_fix: *const f64, pub back_hs_fix: *const f64,
    pub first_node_slot: *const i64, pub hs_front_slot: *const i64, pub hs_back_slot: *const i64,
    pub flow_front_slot: *const i64, pub flow_back_slot: *const i64,
    pub solar_front_slot: *const i64, pub solar_back_slot: *const i64,
    pub ir_front_slot: *const i64, pub ir_back_slot: *const i64,
    pub zone_volume: *const f64, pub zone_slot: *const i64,
}
#[repr(C)] pub struct HeatBatchOptions {
    pub device: i32, pub force_general: i32, pub nodes_per_lane: i32, pub use_graph: i32,
    pub stream: *mut c_void, pub n_ranks: i32, pub rank: i32, pub no_palette: i32, pub no_fusion: i32,
}
#[repr(C)] pub struct HeatBatch { _private: [u8; 0] }
// The series structs this file does not spell out (include/heat_amd.h: heat_series, heat_zone_loads, heat_ideal_loads,
// heat_series_report): passed by pointer only.
#[repr(C)] pub struct HeatSeries { _private: [u8; 0] }
#[repr(C)] pub struct HeatZoneLoads { _private: [u8; 0] }
#[repr(C)] pub struct HeatIdealLoads { _private: [u8; 0] }
#[repr(C)] pub struct HeatSeriesReport { _private: [u8; 0] }
#[repr(C)] #[derive(Clone, Copy)]
pub struct HeatSkyRecord { pub sun_x: f64, pub sun_y: f64, pub sun_z: f64, pub beam: f64, pub diffuse: f64, pub ground: f64,
                           pub ir_sky: f64, pub ir_ground: f64 }
#[repr(C)] pub struct HeatSky {
    pub record: *const HeatSkyRecord, pub normal_x: *const f64, pub normal_y: *const f64, pub normal_z: *const f64,
    pub mode: *const u8,
}
// heat_solar_gains: apertures (windows seen from the sky) and entries (the shares of an aperture's power a side receives)
#[repr(C)] pub struct HeatSolarGains {
    pub n_apertures: i64, pub ap_surface: *const i64,
    pub ap_normal_x: *const f64, pub ap_normal_y: *const f64, pub ap_normal_z: *const f64,
    pub ap_tau_coef: *const f64, pub ap_tau_diffuse: *const f64, pub ap_scale: *const f64, pub ap_sum: *mut f64,
    pub n_entries: i64, pub en_surface: *const i64, pub en_side: *const u8, pub en_aperture: *const i32,
    pub en_beam: *const f64, pub en_diffuse: *const f64,
}
// heat_air_paths: air that moves between zones, and vents controlled on the state of both of their ends
#[repr(C)] pub struct HeatAirPaths {
    pub n_paths: i64, pub target: *const i32, pub source: *const i32, pub temp_chan: *const i32, pub volume_chan: *const i32,
    pub volume_gain: *const f64, pub open_chan: *const i32, pub sense: *const i8, pub band: *const f64, pub min_delta: *const f64,
    pub state: *mut u8, pub sum_q: *mut f64, pub steps_open: *mut i64, pub switches: *mut i64,
}
// heat_shades: overhangs, side fins and horizon profiles, and the sides and apertures they shade
#[repr(C)] pub struct HeatShades {
    pub n_shades: i64, pub sh_surface: *const i64,
    pub sh_normal_x: *const f64, pub sh_normal_y: *const f64, pub sh_normal_z: *const f64,
    pub sh_right_x: *const f64, pub sh_right_y: *const f64, pub sh_right_z: *const f64,
    pub sh_up_x: *const f64, pub sh_up_y: *const f64, pub sh_up_z: *const f64,
    pub sh_width: *const f64, pub sh_height: *const f64, pub overhang_depth: *const f64, pub overhang_gap: *const f64,
    pub fin_pos_depth: *const f64, pub fin_pos_gap: *const f64, pub fin_neg_depth: *const f64, pub fin_neg_gap: *const f64,
    pub diffuse_factor: *const f64, pub ground_factor: *const f64, pub sh_horizon: *const i32,
    pub n_horizons: i64, pub horizon_tan2: *const f64,
    pub front_shade: *const i32, pub back_shade: *const i32, pub aperture_shade: *const i32,
}
// heat_room_radiation: long-wave exchange among the faces of a room
#[repr(C)] pub struct HeatRoomRadiation {
    pub n_receivers: i64, pub rc_surface: *const i64, pub rc_side: *const u8, pub sum_irradiance: *mut f64,
    pub n_entries: i64, pub en_receiver: *const i64, pub en_surface: *const i64, pub en_side: *const u8,
    pub en_chan: *const i32, pub en_factor: *const f64,
}
// heat_ambient_drive: ambient-side temperatures of a series, per step
#[repr(C)] pub struct HeatAmbientDrive {
    pub n_sides: i64, pub surface: *const i64, pub side: *const u8, pub chan: *const i32, pub gain: *const f64,
    pub offset: *const f64, pub mix_zone: *const i32, pub mix: *const f64, pub sum_temperature: *mut f64,
}
// heat_blinds: movable solar protection that rides on shades, controlled or scheduled
#[repr(C)] pub struct HeatBlinds {
    pub n_blinds: i64, pub shade: *const i32,
    pub beam_closed: *const f64, pub diffuse_closed: *const f64, pub ground_closed: *const f64,
    pub pos_chan: *const i32, pub irr_close: *const f64, pub irr_open: *const f64,
    pub zone: *const i32, pub set_chan: *const i32, pub band: *const f64, pub enable_chan: *const i32,
    pub state: *mut u8, pub steps_closed: *mut i64, pub switches: *mut i64, pub sum_position: *mut f64,
}
// heat_sky_coef / heat_sky_aniso: an anisotropic sky — (F1, F2) per site and step beside the records, a band per consumer
#[repr(C)] #[derive(Clone, Copy)]
pub struct HeatSkyCoef { pub circ: f64, pub horiz: f64 }
#[repr(C)] pub struct HeatSkyAniso {
    pub coef: *const HeatSkyCoef, pub front_band: *const f64, pub back_band: *const f64,
    pub aperture_band: *const f64, pub shade_band: *const f64,
}
// heat_series_call: every term of a series by name; zero it (std::mem::zeroed), set size = size_of::<HeatSeriesCall>(), fill
#[repr(C)] pub struct HeatSeriesCall {
    pub size: usize, pub s: *const HeatSeries, pub sky: *const HeatSky, pub aniso: *const HeatSkyAniso,
    pub shades: *const HeatShades, pub gains: *const HeatSolarGains, pub l: *const HeatZoneLoads, pub air: *mut HeatAirPaths,
    pub il: *mut HeatIdealLoads, pub r: *mut HeatSeriesReport, pub radiation: *mut HeatRoomRadiation,
    pub ambient: *mut HeatAmbientDrive, pub blinds: *mut HeatBlinds,
    pub trace: *mut f64, pub applied: *mut f64, pub ideal_q: *mut f64, pub transmitted: *mut f64, pub path_q: *mut f64,
    pub sunlit: *mut f64, pub irradiance: *mut f64, pub ambient_t: *mut f64, pub position: *mut f64,
    pub blind_incident: *mut f64, pub failed_step: *mut i32,
}
// heat_comfort: operative-temperature sensors of a series — faces and weights, limits as channels, in/out accumulators
#[repr(C)] pub struct HeatComfort {
    pub n_sensors: i64, pub zone: *const i32, pub air_weight: *const f64, pub control: *const u8,
    pub n_entries: i64, pub en_sensor: *const i32, pub en_surface: *const i64, pub en_side: *const u8, pub en_weight: *const f64,
    pub occ_chan: *const i32, pub lo_chan: *const i32, pub hi_chan: *const i32,
    pub resume: i32, pub step_base: i64,
    pub n_occupied: *mut i64, pub sum_operative: *mut f64, pub min_operative: *mut f64, pub step_min: *mut i64,
    pub max_operative: *mut f64, pub step_max: *mut i64, pub n_below: *mut i64, pub deg_below: *mut f64,
    pub n_above: *mut i64, pub deg_above: *mut f64, pub max_above: *mut f64, pub step_max_above: *mut i64,
}
// heat_air_handlers: ventilation units with heat recovery, a bypass and supply-air coils, and their branches into the zones
#[repr(C)] pub struct HeatAirHandlers {
    pub n_units: i64, pub outdoor_chan: *const i32, pub eff_chan: *const i32, pub eff_gain: *const f64,
    pub bypass_chan: *const i32, pub bypass_band: *const f64, pub bypass_min_delta: *const f64,
    pub heat_chan: *const i32, pub cool_chan: *const i32, pub heat_cap: *const f64, pub cool_cap: *const f64,
    pub n_branches: i64, pub br_unit: *const i32, pub br_zone: *const i32, pub br_volume_chan: *const i32,
    pub br_volume_gain: *const f64, pub br_kind: *const u8,
    pub bypass: *mut u8, pub sum_recovered: *mut f64, pub sum_heating: *mut f64, pub sum_cooling: *mut f64,
    pub steps_bypass: *mut i64, pub switches: *mut i64, pub steps_heat_saturated: *mut i64, pub steps_cool_saturated: *mut i64,
    pub sum_branch_q: *mut f64,
}
// heat_air_species: concentrations per species and zone carried by the air a series moves, and demand vents that follow them
#[repr(C)] pub struct HeatAirSpecies {
    pub n_species: i64, pub outdoor_chan: *const i32,
    pub n_sources: i64, pub src_zone: *const i32, pub src_species: *const i32, pub src_chan: *const i32, pub src_factor: *const f64,
    pub n_vents: i64, pub vent_zone: *const i32, pub vent_species: *const i32, pub vent_temp_chan: *const i32,
    pub vent_enable_chan: *const i32, pub vent_v_min: *const f64, pub vent_v_max: *const f64, pub vent_c_lo: *const f64,
    pub vent_c_hi: *const f64, pub limit_chan: *const i32, pub occ_chan: *const i32, pub resume: i64, pub step_base: i64,
    pub conc: *mut f64, pub n_occupied: *mut i64, pub sum_conc: *mut f64, pub max_conc: *mut f64, pub step_max: *mut i64,
    pub n_above: *mut i64, pub excess_above: *mut f64, pub sum_volume: *mut f64, pub sum_q: *mut f64, pub steps_saturated: *mut i64,
}
// heat_openings: wind- and stack-driven volume flows through openings, written into derived channels of the device's table
#[repr(C)] pub struct HeatOpenings {
    pub n_openings: i64, pub zone_a: *const i32, pub zone_b: *const i32, pub temp_chan: *const i32, pub wind_chan: *const i32,
    pub frac_chan: *const i32, pub out_chan: *const i32, pub area: *const f64, pub cw: *const f64, pub cs: *const f64,
    pub ca: *const f64, pub c0: *const f64, pub resume: i64, pub step_base: i64,
    pub sum_v: *mut f64, pub max_v: *mut f64, pub step_max: *mut i64,
}
// heat_controllers: modulating control loops whose outputs are written into derived channels of the device's table
#[repr(C)] pub struct HeatControllers {
    pub n_controllers: i64, pub sense_kind: *const i32, pub sense_index: *const i32, pub sense_node: *const i32, pub set_chan: *const i32,
    pub action: *const i32, pub en_chan: *const i32, pub lim_kind: *const i32, pub lim_index: *const i32, pub lim_node: *const i32,
    pub out_chan: *const i32, pub kp: *const f64, pub ki: *const f64, pub bias: *const f64, pub out_lo: *const f64, pub out_hi: *const f64,
    pub lim_hi: *const f64, pub lim_lo: *const f64, pub resume: i64, pub integral: *mut f64, pub tripped: *mut u8,
    pub sum_u: *mut f64, pub sum_out: *mut f64, pub steps_on: *mut i64, pub steps_sat: *mut i64, pub trips: *mut i64,
}
// heat_air_networks: pressure-balanced flows through the links of zone networks, written into derived channels
#[repr(C)] pub struct HeatAirNetworks {
    pub n_networks: i64, pub n_nodes: i64, pub n_links: i64, pub net_offset: *const i32, pub tol: *const f64, pub max_iter: *const i32,
    pub g_min: *const f64, pub node_zone: *const i32, pub src_chan: *const i32, pub src_gain: *const f64, pub zone_a: *const i32,
    pub zone_b: *const i32, pub temp_chan: *const i32, pub wp_chan: *const i32, pub frac_chan: *const i32, pub out_ab: *const i32,
    pub out_ba: *const i32, pub c: *const f64, pub gh: *const f64, pub p_lin: *const f64, pub wp_gain: *const f64, pub resume: i64,
    pub pressure: *mut f64, pub sum_ab: *mut f64, pub sum_ba: *mut f64, pub iters_sum: *mut i64, pub unconverged: *mut i64,
    pub max_res: *mut f64,
}

pub const HEAT_COMM_ID_BYTES: usize = 128;

extern "C" {
    pub fn heat_batch_create(desc: *const HeatBatchDesc, out: *mut *mut HeatBatch) -> c_int;
    pub fn heat_batch_create_ex(desc: *const HeatBatchDesc, opt: *const HeatBatchOptions,
                                out: *mut *mut HeatBatch) -> c_int;
    pub fn heat_batch_destroy(b: *mut HeatBatch);
    pub fn heat_batch_upload_state(b: *mut HeatBatch, state: *const f64, n_state: usize) -> c_int;
    pub fn heat_batch_upload_inputs(b: *mut HeatBatch, state: *const f64, n_state: usize) -> c_int;
    pub fn heat_batch_download_state(b: *mut HeatBatch, state: *mut f64, n_state: usize) -> c_int;
    pub fn heat_batch_march(b: *mut HeatBatch, state: *mut f64, n_state: usize,
                            weather: *const HeatWeather, n_sub: i32,
                            zone_a0: *const f64, zone_b0: *const f64) -> c_int;
    pub fn heat_batch_march_resident(b: *mut HeatBatch, weather: *const HeatWeather, n_sub: i32,
                                     zone_a0: *const f64, zone_b0: *const f64) -> c_int;
    pub fn heat_batch_synchronize(b: *mut HeatBatch) -> c_int;
    // multi-GPU: one process per GPU, the library owns the RCCL communicator
    pub fn heat_comm_unique_id(id: *mut u8) -> c_int;
    pub fn heat_batch_comm_init(b: *mut HeatBatch, id: *const u8) -> c_int;
    pub fn heat_comm_available() -> c_int;
    // a model cut along its zone-connected clusters: no zone shared, no communicator needed
    pub fn heat_partition(desc: *const HeatBatchDesc, n_ranks: i32, rank_of_surface: *mut i32,
                          n_shared_zones: *mut i64) -> c_int;
    pub fn heat_batch_create_shard(desc: *const HeatBatchDesc, opt: *const HeatBatchOptions,
                                   rank_of_surface: *const i32, out: *mut *mut HeatBatch) -> c_int;
    // which outputs travel back with every march (HEAT_OUT_*), and the rest on demand
    pub fn heat_batch_march_ex(b: *mut HeatBatch, state: *mut f64, n_state: usize, weather: *const HeatWeather,
                               n_sub: i32, zone_a0: *const f64, zone_b0: *const f64, what: i32) -> c_int;
    pub fn heat_batch_download_outputs(b: *mut HeatBatch, state: *mut f64, n_state: usize, what: i32) -> c_int;
    pub fn heat_batch_failed_surface(b: *const HeatBatch, index: *mut i64, kind: *mut i32) -> c_int;
    pub fn heat_batch_set_fusion(b: *mut HeatBatch, enabled: i32) -> c_int;
    // ideal loads in the cluster-resident march: opt-in per batch, what the batch would do, and the planner's answer
    // (host-only; reason: heat_ideal_resident_reason, 0 eligible .. 4)
    pub fn heat_batch_set_ideal_resident(b: *mut HeatBatch, enabled: i32) -> c_int;
    pub fn heat_batch_ideal_resident(b: *const HeatBatch) -> i32;
    pub fn heat_plan_ideal_resident(desc: *const HeatBatchDesc, opt: *const HeatBatchOptions, n_sites: i32,
                                    site_of_surface: *const i32, reason: *mut i32) -> c_int;
    // solar gains of a series: window-transmitted solar onto the room's faces, formed on the device at every step
    pub fn heat_solar_gains_check(desc: *const HeatBatchDesc, n_sites: i32, s: *const HeatSeries, sky: *const HeatSky,
                                  gains: *const HeatSolarGains) -> c_int;
    pub fn heat_batch_march_series_gains(b: *mut HeatBatch, s: *const HeatSeries, sky: *const HeatSky,
                                         gains: *const HeatSolarGains, l: *const HeatZoneLoads, il: *mut HeatIdealLoads,
                                         r: *mut HeatSeriesReport, trace: *mut f64, applied: *mut f64, ideal_q: *mut f64,
                                         transmitted: *mut f64, failed_step: *mut i32) -> c_int;
    // air paths of a series: zone-to-zone mixing and controlled vents, formed on the device at every step
    pub fn heat_air_paths_check(desc: *const HeatBatchDesc, n_sites: i32, s: *const HeatSeries, air: *const HeatAirPaths) -> c_int;
    pub fn heat_batch_march_series_air(b: *mut HeatBatch, s: *const HeatSeries, sky: *const HeatSky,
                                       gains: *const HeatSolarGains, l: *const HeatZoneLoads, air: *mut HeatAirPaths,
                                       il: *mut HeatIdealLoads, r: *mut HeatSeriesReport, trace: *mut f64, applied: *mut f64,
                                       ideal_q: *mut f64, transmitted: *mut f64, path_q: *mut f64, failed_step: *mut i32) -> c_int;
    // shades of a series: sunlit fractions of overhangs, fins and horizons, formed on the device at every step
    pub fn heat_shades_check(desc: *const HeatBatchDesc, n_sites: i32, s: *const HeatSeries, sky: *const HeatSky,
                             gains: *const HeatSolarGains, shades: *const HeatShades) -> c_int;
    pub fn heat_batch_march_series_shaded(b: *mut HeatBatch, s: *const HeatSeries, sky: *const HeatSky, shades: *const HeatShades,
                                          gains: *const HeatSolarGains, l: *const HeatZoneLoads, air: *mut HeatAirPaths,
                                          il: *mut HeatIdealLoads, r: *mut HeatSeriesReport, trace: *mut f64, applied: *mut f64,
                                          ideal_q: *mut f64, transmitted: *mut f64, path_q: *mut f64, sunlit: *mut f64,
                                          failed_step: *mut i32) -> c_int;
    // room radiation of a series: the long-wave irradiance of a room's faces from the emission of the faces they see
    pub fn heat_room_radiation_check(desc: *const HeatBatchDesc, n_sites: i32, s: *const HeatSeries, sky: *const HeatSky,
                                     radiation: *const HeatRoomRadiation) -> c_int;
    pub fn heat_batch_march_series_radiation(b: *mut HeatBatch, s: *const HeatSeries, sky: *const HeatSky, shades: *const HeatShades,
                                             gains: *const HeatSolarGains, l: *const HeatZoneLoads, air: *mut HeatAirPaths,
                                             il: *mut HeatIdealLoads, r: *mut HeatSeriesReport, trace: *mut f64, applied: *mut f64,
                                             ideal_q: *mut f64, transmitted: *mut f64, path_q: *mut f64, sunlit: *mut f64,
                                             radiation: *mut HeatRoomRadiation, irradiance: *mut f64, failed_step: *mut i32) -> c_int;
    // ambient temperatures after creation: per call, and per step of a series from a channel and a zone temperature
    pub fn heat_batch_set_ambient(b: *mut HeatBatch, n: i64, surface: *const i64, side: *const u8, temperature: *const f64) -> c_int;
    pub fn heat_ambient_check(desc: *const HeatBatchDesc, n_sites: i32, s: *const HeatSeries, a: *const HeatAmbientDrive) -> c_int;
    pub fn heat_batch_march_series_ambient(b: *mut HeatBatch, s: *const HeatSeries, sky: *const HeatSky, shades: *const HeatShades,
                                           gains: *const HeatSolarGains, l: *const HeatZoneLoads, air: *mut HeatAirPaths,
                                           il: *mut HeatIdealLoads, r: *mut HeatSeriesReport, trace: *mut f64, applied: *mut f64,
                                           ideal_q: *mut f64, transmitted: *mut f64, path_q: *mut f64, sunlit: *mut f64,
                                           radiation: *mut HeatRoomRadiation, irradiance: *mut f64, ambient: *mut HeatAmbientDrive,
                                           ambient_t: *mut f64, failed_step: *mut i32) -> c_int;
    // blinds of a series: movable shades driven by the sun on the window, a zone temperature and schedules, at every step
    pub fn heat_blinds_check(desc: *const HeatBatchDesc, n_sites: i32, s: *const HeatSeries, sky: *const HeatSky,
                             gains: *const HeatSolarGains, shades: *const HeatShades, blinds: *const HeatBlinds) -> c_int;
    pub fn heat_batch_march_series_blinds(b: *mut HeatBatch, s: *const HeatSeries, sky: *const HeatSky, shades: *const HeatShades,
                                          gains: *const HeatSolarGains, l: *const HeatZoneLoads, air: *mut HeatAirPaths,
                                          il: *mut HeatIdealLoads, r: *mut HeatSeriesReport, trace: *mut f64, applied: *mut f64,
                                          ideal_q: *mut f64, transmitted: *mut f64, path_q: *mut f64, sunlit: *mut f64,
                                          radiation: *mut HeatRoomRadiation, irradiance: *mut f64, ambient: *mut HeatAmbientDrive,
                                          ambient_t: *mut f64, blinds: *mut HeatBlinds, position: *mut f64,
                                          blind_incident: *mut f64, failed_step: *mut i32) -> c_int;
    // anisotropic sky of a series, and the entry point that takes every term of a series in one struct
    pub fn heat_sky_aniso_check(desc: *const HeatBatchDesc, n_sites: i32, s: *const HeatSeries, sky: *const HeatSky,
                                gains: *const HeatSolarGains, shades: *const HeatShades, aniso: *const HeatSkyAniso) -> c_int;
    pub fn heat_batch_march_series_call(b: *mut HeatBatch, call: *const HeatSeriesCall) -> c_int;
    // comfort of a series: operative temperatures per room, reported, accumulated and sensed by the controls
    pub fn heat_comfort_check(desc: *const HeatBatchDesc, s: *const HeatSeries, c: *const HeatComfort) -> c_int;
    pub fn heat_batch_march_series_comfort(b: *mut HeatBatch, call: *const HeatSeriesCall, c: *mut HeatComfort,
                                           operative: *mut f64, mrt: *mut f64) -> c_int;
    // air handlers of a series: heat recovery, bypass and supply coils from the zone temperatures the device holds
    pub fn heat_air_handlers_check(desc: *const HeatBatchDesc, s: *const HeatSeries, h: *const HeatAirHandlers) -> c_int;
    pub fn heat_batch_march_series_handlers(b: *mut HeatBatch, call: *const HeatSeriesCall, c: *mut HeatComfort,
                                            operative: *mut f64, mrt: *mut f64, h: *mut HeatAirHandlers, supply_t: *mut f64,
                                            recovered: *mut f64, coil_q: *mut f64, branch_q: *mut f64) -> c_int;
    // air species of a series: concentrations carried by every flow of air, demand vents that follow them
    pub fn heat_air_species_check(desc: *const HeatBatchDesc, s: *const HeatSeries, l: *const HeatZoneLoads, air: *const HeatAirPaths,
                                  h: *const HeatAirHandlers, sp: *const HeatAirSpecies) -> c_int;
    pub fn heat_batch_march_series_species(b: *mut HeatBatch, call: *const HeatSeriesCall, c: *mut HeatComfort,
                                           operative: *mut f64, mrt: *mut f64, h: *mut HeatAirHandlers, supply_t: *mut f64,
                                           recovered: *mut f64, coil_q: *mut f64, branch_q: *mut f64, sp: *mut HeatAirSpecies,
                                           conc_rows: *mut f64, vent_v: *mut f64, vent_q: *mut f64) -> c_int;
    // openings of a series: volume flows from the zone temperatures the device holds, read by every consumer as a channel
    pub fn heat_openings_check(desc: *const HeatBatchDesc, s: *const HeatSeries, op: *const HeatOpenings) -> c_int;
    pub fn heat_batch_march_series_openings(b: *mut HeatBatch, call: *const HeatSeriesCall, c: *mut HeatComfort,
                                            operative: *mut f64, mrt: *mut f64, h: *mut HeatAirHandlers, supply_t: *mut f64,
                                            recovered: *mut f64, coil_q: *mut f64, branch_q: *mut f64, sp: *mut HeatAirSpecies,
                                            conc_rows: *mut f64, vent_v: *mut f64, vent_q: *mut f64, op: *mut HeatOpenings,
                                            opening_v: *mut f64) -> c_int;
    // controllers of a series: modulating loops on the temperatures the device holds, read by every consumer as a channel
    pub fn heat_controllers_check(desc: *const HeatBatchDesc, s: *const HeatSeries, op: *const HeatOpenings,
                                  ct: *const HeatControllers) -> c_int;
    pub fn heat_batch_march_series_controllers(b: *mut HeatBatch, call: *const HeatSeriesCall, c: *mut HeatComfort,
                                               operative: *mut f64, mrt: *mut f64, h: *mut HeatAirHandlers, supply_t: *mut f64,
                                               recovered: *mut f64, coil_q: *mut f64, branch_q: *mut f64, sp: *mut HeatAirSpecies,
                                               conc_rows: *mut f64, vent_v: *mut f64, vent_q: *mut f64, op: *mut HeatOpenings,
                                               opening_v: *mut f64, ct: *mut HeatControllers, control_u: *mut f64,
                                               control_out: *mut f64) -> c_int;
    // air networks of a series: node pressures that balance the links' mass flows, the flows read by the air paths as channels
    pub fn heat_air_networks_check(desc: *const HeatBatchDesc, s: *const HeatSeries, op: *const HeatOpenings,
                                   ct: *const HeatControllers, nw: *const HeatAirNetworks) -> c_int;
    pub fn heat_batch_march_series_networks(b: *mut HeatBatch, call: *const HeatSeriesCall, c: *mut HeatComfort,
                                            operative: *mut f64, mrt: *mut f64, h: *mut HeatAirHandlers, supply_t: *mut f64,
                                            recovered: *mut f64, coil_q: *mut f64, branch_q: *mut f64, sp: *mut HeatAirSpecies,
                                            conc_rows: *mut f64, vent_v: *mut f64, vent_q: *mut f64, op: *mut HeatOpenings,
                                            opening_v: *mut f64, ct: *mut HeatControllers, control_u: *mut f64,
                                            control_out: *mut f64, nw: *mut HeatAirNetworks, link_q: *mut f64, node_p: *mut f64,
                                            net_iters: *mut i32) -> c_int;
    pub fn heat_last_error() -> *const c_char;
}

pub const HEAT_OUT_NODE_TEMPERATURES: i32 = 1;
pub const HEAT_OUT_SURFACE_SCALARS: i32 = 2;
pub const HEAT_OUT_ZONE_TEMPERATURES: i32 = 4;
pub const HEAT_OUT_ALL: i32 = 7;

pub fn check(rc: c_int) -> Result<(), String> {
    if rc == 0 { Ok(()) } else {
        Err(unsafe { std::ffi::CStr::from_ptr(heat_last_error()) }.to_string_lossy().into_owned())
    }
}
