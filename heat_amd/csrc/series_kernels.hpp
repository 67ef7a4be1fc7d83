// series_kernels.hpp — host-callable launchers of the kernels in series_kernels.hip and the device views they take.
#pragma once
#include "kernels.hpp"

namespace heat {

// Series march (heat_batch_march_series): the driven inputs of a step and its probes. The head of a step is
// launch_begin_march with device-resident sources.
struct SeriesInputs {
    const int32_t *chan;      // [4][S] in device surface order: solar front, solar back, long-wave front, long-wave back;
                              // a channel of the step's row, or -1: the input is not driven
    const double *gain[4];    // [S] each, same order; nullptr: 1
    const uint8_t *own_face;  // [S]: bit 0 / 1 = add sigma T^4 of the own first / last node to the front / back long-wave
                              // input; nullptr: nowhere
    const uint32_t *face;     // [2][S]: index into the T buffer of the first / last node (read only where own_face asks)
};
void launch_series_inputs(int n_surf, const double *row, const SeriesInputs &in, const double *T, const double *side_alpha,
                          SideDyn *dyn, const SlotArrays &sl, double *mirror, hipStream_t st);
// Sky of a series step (heat_sky, include/heat_amd.h): launched behind launch_series_inputs and before the body, one lane per
// device surface; only when some mode byte is set.
struct alignas(16) SkyRecord {  // heat_sky_record
    double sun_x, sun_y, sun_z, beam, diffuse, ground, ir_sky, ir_ground;
};
// Anisotropic sky (heat_sky_aniso, include/heat_amd.h): one pair per site and step beside the record. The three consumers of
// the record — launch_series_blinds, launch_series_sky, launch_series_apertures — take the step's row of pairs, [n_sites], and
// their bands (sides [2][S] in device order, shades [n_shades], apertures [n]); coef == nullptr launches the isotropic kernels.
struct alignas(16) SkyCoef {  // heat_sky_coef
    double circ, horiz;
};
// What a shaded consumer gathers (heat_shades): the step's sunlit fraction k_series_shading has just stored and the two
// constant factors, rows of the shade table.
struct ShadeFactors {
    const double *f;        // [n_shades] the step's sunlit fraction of the beam
    const double *diffuse;  // [n_shades] (ones where the caller gave none)
    const double *ground;   // [n_shades]
};
struct SeriesSky {
    const uint8_t *mode;     // [S] in device surface order: bit 0 solar front, 1 solar back, 2 long-wave front, 3 long-wave back
    const double *normal;    // [3][S]: x, y, z of the front face's outward normal
    const int32_t *site;     // [S] (SideArrays::site); nullptr: site 0
    const double *gain[4];   // the series' gain arrays (SeriesInputs::gain); nullptr: 1
    const int32_t *shade;    // [2][S] the shade of the front / back solar input, -1: none; nullptr: no side is shaded
    ShadeFactors sf;
};
// Shades of a series step (heat_shades, include/heat_amd.h; table: plan.hpp, ShadeTables): launched behind
// launch_series_inputs and before launch_series_sky, one lane per shade; only when there are shades.
struct SeriesShades {
    int n;
    const int32_t *site;     // [n] the site whose record the shade reads
    const int32_t *horizon;  // [n] horizon profile, -1: none
    const double *tab;       // [kShadeRows][n]
    const double *tan2;      // [n_horizons][16]
    double *f;               // [n] out: the step's sunlit fraction
};
// records: the step's row of the record table, [n_sites]; sunlit_row: the step's row of sunlit, [n], or nullptr
void launch_series_shading(const SkyRecord *records, const SeriesShades &sh, double *sunlit_row, hipStream_t st);
// Blinds of a series step (heat_blinds, include/heat_amd.h; tables: plan.hpp, BlindTables): one launch behind
// launch_series_shading and before launch_series_sky, only when there are blinds — one lane per SHADE. A lane reads its
// shade's normal and constant factors from the shade table's rows and the f launch_series_shading has just stored, and writes
// the three EFFECTIVE factors the shaded consumers gather (ShadeFactors) in place of (f, the table's rows): plain copies where
// the shade carries no blind. The blind table is a structure of arrays in the caller's blind order; a blind has one shade, so
// its state byte, accumulators and output elements have one writer.
struct SeriesBlinds {
    int n_shades, n_blinds;
    const int32_t *blind_of_shade;  // [n_shades] -1: the shade carries no blind
    const int32_t *site;            // [n_shades] (SeriesShades::site)
    const double *tab;              // [kShadeRows][n_shades] (SeriesShades::tab)
    const double *f;                // [n_shades] (SeriesShades::f)
    const int32_t *pos_chan, *zone, *set_chan, *enable_chan;  // [n_blinds] each, -1: none
    const double *beam_closed, *diffuse_closed, *ground_closed, *irr_close, *irr_open, *half_band;  // [n_blinds] each
    uint8_t *state;                 // [n_blinds]
    double *sum_position;           // [n_blinds] each; nullptr: not maintained
    int64_t *steps_closed, *switches;
    double *eff_f, *eff_diffuse, *eff_ground;  // [n_shades] each, out: what ShadeFactors hands the consumers
};
// records: the step's row of the record table, [n_sites]; row: the step's row of the channel table; position_row /
// incident_row: the step's rows of position / blind_incident, [n_blinds] (caller's order), or nullptr
void launch_series_blinds(const SkyRecord *records, const SeriesBlinds &bl, const double *row, const double *zone_T,
                          double *position_row, double *incident_row, const SkyCoef *coef, const double *band, hipStream_t st);
// records: the step's row of the record table, [n_sites]
void launch_series_sky(int n_surf, const SkyRecord *records, const SeriesSky &sky, const double *side_alpha, SideDyn *dyn,
                       const SlotArrays &sl, double *mirror, const SkyCoef *coef, const double *band, hipStream_t st);
// Solar gains of a series step (heat_solar_gains, include/heat_amd.h; tables: plan.hpp, SolarGainTables): two launches
// behind launch_series_sky and before the body, only when there are apertures — one lane per aperture, then (only when there
// are entries) one lane per receiver.
struct SeriesApertures {
    int n;
    const int32_t *dev;       // [n] the aperture's device surface (for its site)
    const int32_t *site;      // [S] (SideArrays::site); nullptr: site 0
    const double *normal;     // [3][n]
    const double *coef;       // [6][n]: coefficient j of all apertures contiguous
    const double *tau_scale;  // [2][n]: tau_diffuse, scale
    double2 *power;           // [n] (Pb, Pd) of the step, W
    double *sum;              // [n] ap_sum; nullptr: not kept
    const int32_t *shade;     // [n] the aperture's shade, -1: none; nullptr: no aperture is shaded
    ShadeFactors sf;
};
struct SeriesGains {
    int n_receivers;
    const uint32_t *rec;       // [n_receivers] side * S + device surface
    const int64_t *slice_off;  // [n_slices + 1]
    const int32_t *ap;         // sliced ELL, -1: padding
    const double2 *share;      // (en_beam, en_diffuse) beside ap
    const double2 *power;      // SeriesApertures::power
    const double *gain[2];     // the series' solar gain arrays, front and back (SeriesInputs::gain); nullptr: 1
};
// records: the step's row of the record table, [n_sites]; transmitted: the step's row, [n], or nullptr
void launch_series_apertures(const SkyRecord *records, const SeriesApertures &ap, double *transmitted, const SkyCoef *coef,
                             const double *band, hipStream_t st);
void launch_series_solar_gains(int n_surf, const SeriesGains &g, const double *side_alpha, SideDyn *dyn, const SlotArrays &sl,
                               double *mirror, hipStream_t st);
// Room radiation of a series step (heat_room_radiation, include/heat_amd.h; tables: plan.hpp, RoomRadiationTables): two
// launches behind launch_series_solar_gains and before the body, only when there are receivers — one lane per distinct
// emitter side (only when there are emitters), then one lane per receiver.
struct SeriesRoomRadiation {
    int n_emitters, n_receivers;
    const uint32_t *face;    // [n_emitters] index into the T buffer of the emitter's face node
    double *emission;        // [n_emitters] E of the step
    const uint32_t *rec;     // [n_receivers] side * S + device surface
    const int32_t *off;      // [n_receivers + 1] CSR ranges of the entries
    const int32_t *src;      // [n_entries] >= 0: emitter number; < 0: ~channel of the step's row
    const double *factor;    // [n_entries]
    const double *gain[2];   // the series' long-wave gain arrays, front and back (SeriesInputs::gain[2], [3]); nullptr: 1
    double *sum;             // [n_receivers] sum_irradiance; nullptr: not kept
};
void launch_series_emission(const SeriesRoomRadiation &rr, const double *T, hipStream_t st);
// row: the step's row of the channel table; irradiance_row: the step's row of irradiance, [n_receivers], or nullptr
void launch_series_room_radiation(int n_surf, const SeriesRoomRadiation &rr, const double *row, SideDyn *dyn, const SlotArrays &sl,
                                  double *mirror, double *irradiance_row, hipStream_t st);
// Ambient temperatures of a series step (heat_ambient_drive, include/heat_amd.h; tables: plan.hpp, AmbientTables) and of
// heat_batch_set_ambient: one launch between the step's head and its body, only when there are driven sides — one lane per
// side. It rewrites SideConst::ambient of the side's record, and SideConst::forced of the back record that carries a front's
// ambient temperature (layout.hpp); every kernel family reads both from global memory at the start of its launch.
struct SeriesAmbient {
    int n_sides;
    const uint32_t *rec;       // [n_sides] side * S + device surface
    const uint32_t *peer;      // [n_sides] the back record whose `forced` follows, or kNoAmbientPeer
    const int32_t *chan;       // [n_sides] channel of the step's row; nullptr: lane i reads row[i] (the setter)
    const double *gain;        // [n_sides]; nullptr: 1
    const double *offset;      // [n_sides]; nullptr: 0
    const int32_t *mix_zone;   // [n_sides] -1: none; nullptr: none anywhere
    const double *mix;         // [n_sides] read where mix_zone >= 0
    double *sum;               // [n_sides] sum_temperature; nullptr: not kept
};
// row: the step's row of the channel table (the setter: the temperatures); ambient_row: the step's row of ambient_t,
// [n_sides], or nullptr
void launch_series_ambient(const SeriesAmbient &a, const double *row, const double *zone_T, SideConst *sc, double *ambient_row,
                           hipStream_t st);
// Zone loads of a series step (heat_zone_loads, include/heat_amd.h; tables: plan.hpp, ZoneLoadTables): launched between the
// step's head and its driven inputs, one lane per zone.
struct ZoneLoadsDev {
    const int32_t *off;  // [3][n_zones + 1]: CSR offsets of the zone's gains, flows, thermostats
    const int32_t *gain_chan;
    const double *gain_factor;
    const int32_t *flow_volume_chan, *flow_temp_chan;
    const double *flow_volume_gain;
    const int32_t *th_sensor, *th_heat_chan, *th_cool_chan, *th_orig;
    const double *th_heat_power, *th_cool_power, *th_half_band;
    uint8_t *th_mode;  // [n_thermostats], the caller's order
};
// row: the step's row of the channel table; applied_row: the step's row of `applied` (caller's order), or nullptr;
// flags: the batch's failure flags (a term that makes a zone's a0 / b0 NaN is reported as that zone's failure)
void launch_series_zone_loads(int n_zones, const ZoneLoadsDev &zl, const double *row, const double *zone_T, double *a0, double *b0,
                              double *applied_row, int *flags, hipStream_t st);
// buf / idx: where probe p reads — kProbeBufT: T[idx]; kProbeBufOut: the SideOut records as doubles (2 * record + 0 hs,
// + 1 flow); kProbeBufZone: zone_T[idx]
// fail_step: 5 ints, [0] = -1 until lane 0 finds the failure flags set; then the step and flags[0..3] as of that step
constexpr int kProbeBufT = 0, kProbeBufOut = 1, kProbeBufZone = 2;
void launch_series_probe(int64_t n_probes, const uint8_t *buf, const uint32_t *idx, const double *T, const SideOut *out,
                         const double *zone_T, double *trace_row, const int *flags, int *fail_step, int step, hipStream_t st);

// Report of a series (heat_series_report, include/heat_amd.h; tables: plan.hpp, GroupTables): on the step's tail, beside
// launch_series_probe. launch_series_groups reduces every segment of every group to its partial sum (nothing to do without
// entries); launch_series_stats — one lane per quantity — takes a probe's value as the probe kernel does and a group's as
// its partial sums added in segment order, writes the group's element of the step's group_trace row and updates the
// accumulators that exist (a nullptr array costs no load or store).
struct SeriesGroupsDev {
    const uint8_t *buf;        // [n_entries]: kProbeBuf* of the entry
    const uint32_t *idx;       // [n_entries]: index into that buffer
    const double *weight;      // [n_entries], nullptr: all ones
    const uint32_t *wave_seg;  // [n_wave][3]: first entry, end entry, partial sum
    const uint32_t *row_seg;   // [n_row][3]
    int n_wave, n_row;
    double *part;              // the segments' partial sums
};
void launch_series_groups(const SeriesGroupsDev &g, const double *T, const SideOut *out, const double *zone_T, hipStream_t st);
struct SeriesStatsDev {
    int64_t n_probes, n_groups;
    const uint8_t *buf;        // probes, as launch_series_probe takes them
    const uint32_t *idx;
    const double *part;        // groups: partial sums part[part_off[g] .. part_off[g + 1])
    const uint32_t *part_off;
    double *q_min, *q_max, *q_sum, *q_deg_below, *q_deg_above;  // [n_probes + n_groups] each, nullptr: not maintained
    int64_t *q_step_min, *q_step_max, *q_n_below, *q_n_above;
    const double *q_lo, *q_hi;
};
// group_row: the step's row of group_trace, or nullptr; step: K = step_base + k
void launch_series_stats(const SeriesStatsDev &s, const double *T, const SideOut *out, const double *zone_T, double *group_row,
                         int64_t step, hipStream_t st);
// Thermostat statistics, one lane per thermostat, behind launch_series_zone_loads: mode = the bytes it has just written,
// prev = the modes before this step (kept here), applied_row = the step's applied powers (caller's order).
struct SeriesThStatsDev {
    int64_t *steps_heating, *steps_cooling, *switches;  // [n_thermostats] each, nullptr: not maintained
    double *sum_heating, *sum_cooling;
    uint8_t *prev;
};
void launch_series_th_stats(int n_thermostats, const SeriesThStatsDev &t, const uint8_t *mode, const double *applied_row, hipStream_t st);
// Air paths of a series step (heat_air_paths, include/heat_amd.h; tables: plan.hpp, AirPathTables): launched behind
// launch_series_zone_loads / launch_series_th_stats and before launch_series_inputs, one lane per zone; only when there are
// paths.
struct AirPathsDev {
    const int32_t *off;  // [n_zones + 1]: CSR offsets of the paths whose target the zone is
    const int32_t *source, *temp_chan, *volume_chan, *open_chan, *orig;
    const double *volume_gain, *sense, *half_band, *min_delta;
    uint8_t *state;      // [n_paths], the caller's order (as every array below)
    double *sum_q;       // nullptr: not maintained
    int64_t *steps_open, *switches;
};
// row: the step's row of the channel table; q_row: the step's row of path_q (caller's order), or nullptr; flags: the batch's
// failure flags (a path that makes a zone's a0 / b0 NaN is reported as that zone's failure); control_T: what a controlled
// path senses for e — zone_T itself, or the step's control temperatures (heat_comfort); the air that moves stays zone_T
void launch_series_air_paths(int n_zones, const AirPathsDev &ap, const double *row, const double *zone_T, const double *control_T,
                             double *a0, double *b0, double *q_row, int *flags, hipStream_t st);
// Comfort of a series step (heat_comfort, include/heat_amd.h; tables: plan.hpp, ComfortTables): launched behind the step's
// head and before launch_series_zone_loads, only when there are sensors. launch_series_comfort — one lane per sensor — walks
// the sensor's CSR range of entries, gathers each face node from T, forms the mean radiant and the operative temperature,
// stores them into `top` (always) and the step's rows (where asked) and updates the accumulators that exist.
// launch_series_control_T — one lane per zone, only with a control sensor — writes control_T[z] = top[ctl_sensor[z]], or
// zone_T[z] where the zone has none: what the thermostats, the air paths' e and the blinds then read in place of zone_T.
struct SeriesComfort {
    int n_sensors;
    const int32_t *off;        // [n_sensors + 1]
    const uint32_t *face;      // [n_entries]: index into T
    const double *weight;      // [n_entries]
    const int32_t *zone, *occ_chan, *lo_chan, *hi_chan;  // [n_sensors] each; channels -1: none
    const double *air_weight;  // [n_sensors]
    double *top;               // [n_sensors]: the step's operative temperatures
    int64_t *n_occupied, *step_min, *step_max, *n_below, *n_above, *step_max_above;  // [n_sensors] each, nullptr: not maintained
    double *sum_operative, *min_operative, *max_operative, *deg_below, *deg_above, *max_above;
};
// row: the step's row of the channel table; operative_row / mrt_row: the step's rows, [n_sensors], or nullptr; step: K
void launch_series_comfort(const SeriesComfort &cf, const double *row, const double *T, const double *zone_T, double *operative_row,
                           double *mrt_row, int64_t step, hipStream_t st);
void launch_series_control_T(int n_zones, const int32_t *ctl_sensor, const double *top, const double *zone_T, double *control_T,
                             hipStream_t st);
// Air handlers of a series step (heat_air_handlers, include/heat_amd.h; tables: plan.hpp, HandlerTables): launched behind
// launch_series_air_paths and before launch_series_ambient, only when there are units. launch_series_handler_units — one lane
// per unit — walks the unit's CSR range of branches twice (extract, then supply), forms Te, the bypass, Tr, the mass flows and
// the coil, stores Ts[u] and m[j] into the call's scratch and updates the unit's rows, state byte and accumulators.
// launch_series_handler_supply — one lane per zone, behind it — adds the zone's supply branches to its a0 / b0 and writes
// their branch_q.
struct HandlersDev {
    int n_units;
    const int32_t *unit_off;                       // [n_units + 1]: CSR offsets of all branches of the unit
    const int32_t *u_zone, *u_chan, *u_orig;       // [n_branches], sorted by unit
    const uint8_t *u_kind;
    const double *u_gain;
    const int32_t *zone_off;                       // [n_zones + 1]: CSR offsets of the supply branches into the zone
    const int32_t *z_unit, *z_orig;                // [n_supply], sorted by zone
    const int32_t *outdoor_chan, *eff_chan, *bypass_chan, *heat_chan, *cool_chan;   // [n_units] each; -1: none
    const double *eff_gain, *half_band, *min_delta, *heat_cap, *cool_cap;           // [n_units] each
    double *ts, *m;                                // [n_units], [n_branches] (caller's order): the step's scratch
    uint8_t *bypass;                               // [n_units]
    double *sum_recovered, *sum_heating, *sum_cooling;   // [n_units] each, nullptr: not maintained
    int64_t *steps_bypass, *switches, *steps_heat_saturated, *steps_cool_saturated;
    double *sum_branch_q;                          // [n_branches], the caller's order; nullptr: not maintained
};
// row: the step's row of the channel table; the four rows of the step's outputs (caller's order), or nullptr each
void launch_series_handler_units(const HandlersDev &h, const double *row, const double *zone_T, double *supply_row, double *recovered_row,
                                 double *coil_row, double *branch_row, hipStream_t st);
// flags: the batch's failure flags (a branch that makes a zone's a0 / b0 NaN is reported as that zone's failure)
void launch_series_handler_supply(int n_zones, const HandlersDev &h, const double *zone_T, double *a0, double *b0, double *branch_row,
                                  int *flags, hipStream_t st);
// Air species of a series step (heat_air_species, include/heat_amd.h; tables: plan.hpp, SpeciesTables): launched behind
// launch_series_handler_supply and before launch_series_ambient, only when there are species. launch_series_vents — one lane
// per zone, only when there are vents — forms the volume flow of each of the zone's demand vents from the concentrations the
// step starts with, adds the enabled ones to the zone's a0 / b0, stores V into the call's scratch and updates the vent's rows
// and accumulators. launch_series_species — one lane per (species, zone), behind it — sums the sources and every inflow of
// the step (the loads' flows, the open air paths, the handlers' supply branches and the vents, read through those terms' own
// views), steps the concentration into conc_next and updates the lane's row and accumulators. conc is never written in a
// step: no lane sees another's new value; the driver swaps the two buffers between the steps.
struct SpeciesDev {
    int n_species, n_vents;
    const int32_t *outdoor_chan;                   // [n_species][n_zones]; -1: 0.0
    const int32_t *src_off, *src_chan;             // [n_species * n_zones + 1], [n_sources] by lane
    const double *src_factor;
    const int32_t *vent_off;                       // [n_zones + 1]; nullptr: no vent
    const int32_t *v_species, *v_temp_chan, *v_enable_chan, *v_orig;   // [n_vents] by zone
    const double *v_min, *v_max, *c_lo, *c_hi;
    const int32_t *limit_chan, *occ_chan;          // [n_species], [n_zones]; -1: none
    const int32_t *br_chan;                        // [n_branches] of the handlers, the caller's order; nullptr: none
    const double *br_gain;
    double *vent_V;                                // [n_vents], the caller's order: the step's scratch
    int64_t *n_occupied, *step_max, *n_above;      // [n_species][n_zones] each, nullptr: not maintained
    double *sum_conc, *max_conc, *excess_above;
    double *sum_volume, *sum_q;                    // [n_vents], the caller's order; nullptr: not maintained
    int64_t *steps_saturated;
};
// row: the step's row of the channel table; conc: the concentrations at the start of the step; v_row / q_row: the step's rows
// of vent_v / vent_q (caller's order), or nullptr; flags: the batch's failure flags (a vent that makes a zone's a0 / b0 NaN is
// reported as that zone's failure)
void launch_series_vents(int n_zones, const SpeciesDev &sp, const double *row, const double *zone_T, const double *conc, double *a0,
                         double *b0, double *v_row, double *q_row, int *flags, hipStream_t st);
// zl / ap / hd: the views of the step's zone loads, air paths and handlers, or nullptr each (the term is absent); h: n_sub * dt;
// conc_row: the step's row of conc_rows, or nullptr; step: K
void launch_series_species(int n_zones, const SpeciesDev &sp, const ZoneLoadsDev *zl, const AirPathsDev *ap, const HandlersDev *hd,
                           const double *row, const double *zone_vol, double h, const double *conc, double *conc_next, double *conc_row,
                           int64_t step, hipStream_t st);
// Openings of a series step (heat_openings, include/heat_amd.h; tables: plan.hpp, OpeningTables): the first launch of a step
// behind the controllers, ahead of launch_series_comfort, only when there are openings, one lane per opening in the caller's
// order. With the controllers it is one of the two launches that WRITE the step's row of the device's channel table: every
// later launch of the step reads the derived columns as it reads any channel.
struct OpeningsDev {
    int n_openings;
    const int32_t *zone_a, *zone_b, *temp_chan, *wind_chan, *frac_chan, *out_chan;   // [n] each; channels -1: none
    const double *area, *cw, *cs, *ca, *c0;                                           // [n] each
    double *sum_v, *max_v;                                                            // [n] each, nullptr: not maintained
    int64_t *step_max;
};
// row: the step's row of the channel table, written at out_chan; v_row: the step's row of opening_v, or nullptr; step: K
void launch_series_openings(const OpeningsDev &op, double *row, const double *zone_T, double *v_row, int64_t step, hipStream_t st);
// Controllers of a series step (heat_controllers, include/heat_amd.h; tables: plan.hpp, ControllerTables): the FIRST launch
// of a step, ahead of launch_series_openings, only when there are controllers, one lane per controller in the caller's
// order. It writes the step's row of the device's channel table at the controllers' derived columns.
struct ControllersDev {
    int n_controllers;
    const int32_t *sense_kind, *set_chan, *action, *en_chan, *lim_kind, *out_chan;   // [n] each; en_chan, lim_kind -1: none
    const uint32_t *sense_at, *lim_at;     // [n] each: the zone, the channel, or the node's index in T
    const double *kp, *ki, *bias, *out_lo, *out_hi, *lim_hi, *lim_lo;                 // [n] each
    double *integral;                      // [n] the state: always present
    uint8_t *tripped;
    double *sum_u, *sum_out;               // [n] each, nullptr: not maintained
    int64_t *steps_on, *steps_sat, *trips;
};
// row: the step's row of the channel table, written at out_chan; T: the node temperatures; u_row, out_row: the step's rows of
// control_u and control_out, or nullptr
void launch_series_controllers(const ControllersDev &ct, double *row, const double *T, const double *zone_T, double *u_row, double *out_row,
                               hipStream_t st);
// Air networks of a series step (heat_air_networks, include/heat_amd.h; tables: plan.hpp, NetworkTables): launched behind the
// openings, ahead of launch_series_comfort, only when there are networks: one launch of k_series_networks<W> per width class
// present, a workgroup of ONE wavefront holding 64 / W networks, lane = node. With the controllers and the openings it is one
// of the three launches that WRITE the step's row of the device's channel table, at the links' derived columns.
struct NetworksDev {
    int class_start[5];                    // the sorted networks of class c (W = 8 << c): [class_start[c], class_start[c + 1])
    int n_nodes, n_links;
    const int32_t *net_id, *net_n, *net_node0, *net_max_iter;                       // [n_networks], sorted
    const double *net_tol, *net_g_min;
    const int32_t *node_id, *node_zone, *node_src_chan, *node_inc0, *node_inc_n;    // [n_nodes], sorted
    const double *node_src_gain;
    const int32_t *inc;                    // the incident links of every sorted node, ascending
    const int32_t *zone_a, *zone_b, *la, *lb, *temp_chan, *wp_chan, *frac_chan, *out_ab, *out_ba;   // [n_links], the caller's order
    const double *c, *gh, *p_lin, *s_lin, *wp_gain;
    double *pressure;                      // [n_nodes], the caller's order: the state, always present
    double *sum_ab, *sum_ba;               // [n_links], nullptr: not maintained
    int64_t *iters_sum, *unconverged;      // [n_networks], the caller's order
    double *max_res;
};
// row: the step's row of the channel table, written at out_ab and out_ba; q_row, p_row, it_row: the step's rows of link_q,
// node_p and net_iters (the caller's order), or nullptr
void launch_series_networks(const NetworksDev &nw, double *row, const double *zone_T, double *q_row, double *p_row, int32_t *it_row,
                            hipStream_t st);
void launch_fill_f64(double *dst, int64_t n, double value, hipStream_t st);
// Ideal loads of a series: the step's begin and end (the sequence and the view: kernels.hpp, IdealLoadsDev)
void launch_series_ideal_begin(const IdealLoadsDev &il, const double *row, hipStream_t st);
// q_row: the step's row of ideal_q, or nullptr; step: K = step_base + k
void launch_series_ideal_end(const IdealLoadsDev &il, double *q_row, int64_t step, hipStream_t st);

}  // namespace heat
