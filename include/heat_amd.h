/*
 * heat_amd.h — C ABI of the MI355X-native wall heat-conduction path.
 *
 * This is the drop-in boundary for the hot path of SIMPLE-BuildingSimulation/heat
 * (reference paths below are relative to the reference repository root):
 *
 *   ThermalModel::new + allocate_memory   src/model.rs:193-354   -> heat_batch_create
 *   ThermalModel::march (sub-dt loop)      src/model.rs:359-427   -> heat_batch_march
 *   iterate_surfaces                       src/model.rs:102-180   -> (inside march) heat_batch_step_surfaces
 *   calculate_zones_abc + estimate_zones_future_temperatures
 *                                          src/model.rs:489-597,650-674 -> heat_batch_step_zones
 *   SurfaceTrait::{get,set}_node_temperatures & the scalar slot accessors
 *                                          src/surface_trait.rs:81-164 -> heat_batch_upload_state / _download_state
 *
 * The caller (a Rust shim implementing `SimulationModel for GpuThermalModel`,
 * see INTEGRATION.md) keeps owning the flat `SimulationState` array; this
 * library owns a device-resident mirror of the slots the path touches, laid out
 * as a lane-blocked structure of arrays in HBM.
 *
 * Plain C types only. Every function returns 0 on success, a negative
 * HEAT_E_* code for an invalid call/descriptor, or a positive HEAT_N_* code
 * for a numerical failure detected on the device (the reference panics there).
 * heat_last_error() returns a human-readable message for the last failure on
 * the calling thread. The library never aborts the process.
 */
#ifndef HEAT_AMD_H
#define HEAT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HEAT_AMD_ABI_VERSION 1

/* simple_model::Boundary as consumed at src/surface.rs:611-702 */
enum heat_boundary_kind {
    HEAT_BOUNDARY_SPACE = 0,
    HEAT_BOUNDARY_AMBIENT = 1, /* Boundary::AmbientTemperature { temperature } */
    HEAT_BOUNDARY_OUTDOOR = 2,
    HEAT_BOUNDARY_GROUND = 3   /* rejected: the reference panics (surface.rs:642,687; model.rs:92) */
};

/* src/gas.rs:45-74 */
enum heat_gas { HEAT_GAS_AIR = 0, HEAT_GAS_ARGON = 1, HEAT_GAS_KRYPTON = 2, HEAT_GAS_XENON = 3 };

enum heat_status {
    HEAT_OK = 0,
    /* invalid call / descriptor (reference: Err(String) or a setup-time panic) */
    HEAT_E_INVALID_ARG = -1,
    HEAT_E_GROUND_BOUNDARY = -2, /* surface.rs:642,687 */
    HEAT_E_UVALUE_NONE = -3,     /* discretization.rs:53 */
    HEAT_E_SIZE = -4,            /* slot or index out of range */
    HEAT_E_DEVICE = -5,          /* HIP runtime failure (message has the HIP error string) */
    HEAT_E_TOO_MANY_NODES = -6,
    HEAT_E_COMM = -7,            /* RCCL not loadable, or a collective failed (message has RCCL's error string) */
    /* numerical failure on the device (reference: assert!/unreachable! panics) */
    HEAT_N_NAN_HS = 1,           /* surface.rs:704-707 */
    HEAT_N_NAN_NOMASS = 2,       /* surface.rs:850 */
    HEAT_N_NAN_ZONE = 3,         /* model.rs:417-420 */
    HEAT_N_UNREACHABLE = 4       /* convection.rs:104, gas.rs:219,296 */
};

/* src/cavity.rs:28-50 */
typedef struct heat_cavity {
    double thickness;
    double height;
    double angle; /* radians; 0 horizontal, pi/2 vertical */
    double eout;
    double ein;
    int32_t gas;  /* enum heat_gas */
    int32_t reserved;
} heat_cavity;

/* Weather of one sub-timestep (model.rs:371-382). The shim converts degrees to radians
 * (`wind_direction.to_radians()`, model.rs:373). */
typedef struct heat_weather {
    double dry_bulb;       /* C */
    double wind_direction; /* radians */
    double wind_speed;     /* m/s */
} heat_weather;

/*
 * Everything ThermalModel::new derives and the hot path reads, flattened.
 * Surfaces first, then fenestrations (the reference iterates them in that
 * order, model.rs:388-408). All arrays are host memory, copied by
 * heat_batch_create; they need not outlive the call.
 */
typedef struct heat_batch_desc {
    int32_t abi_version; /* HEAT_AMD_ABI_VERSION */
    int32_t reserved;
    int64_t n_surfaces;
    int64_t n_zones;
    int64_t n_cavities;
    int64_t n_state; /* length of the caller's SimulationState array */
    double dt;       /* ThermalModel::dt, model.rs:76,326-330 */

    /* Discretization::segments, CSR over surfaces (discretization.rs:73) */
    const int64_t *node_offset; /* [n_surfaces+1] */
    const double *mass;         /* segments[i].0 ; a node is massive iff mass >= 1e-5 (discretization.rs:149) */
    const double *uvalue;       /* UValue::Solid(u) -> u ; UValue::Back -> 0 ; NaN = UValue::None (rejected) */
    const int32_t *seg_cavity;  /* UValue::Cavity -> index into cavities, else -1 ; NULL when n_cavities == 0 */
    const double *front_alpha;  /* ThermalSurfaceData::front_alphas, surface.rs:366 */
    const double *back_alpha;   /* ThermalSurfaceData::back_alphas, surface.rs:370 */
    const heat_cavity *cavities;

    /* ThermalSurfaceData fields, surface.rs:315-381 */
    const int32_t *front_kind, *back_kind; /* enum heat_boundary_kind */
    const int32_t *front_zone, *back_zone; /* front/back_space_index (used when kind == SPACE) */
    const double *front_ambient, *back_ambient; /* used when kind == AMBIENT */
    const double *front_emissivity, *back_emissivity;
    const double *area, *perimeter;
    const double *cos_tilt;
    const double *normal_x, *normal_y;
    const double *wind_modifier;
    const double *front_hs_fix, *back_hs_fix; /* debug-only overrides, surface.rs:374-380; NULL or NaN = none */

    /* SimulationState slots (surface.rs:428-442; surface_trait.rs:223-378) */
    const int64_t *first_node_slot; /* node slots of a surface are contiguous */
    const int64_t *hs_front_slot, *hs_back_slot;
    const int64_t *flow_front_slot, *flow_back_slot;
    const int64_t *solar_front_slot, *solar_back_slot;
    const int64_t *ir_front_slot, *ir_back_slot;

    /* ThermalZone (zone.rs:28-56) */
    const double *zone_volume;
    const int64_t *zone_slot; /* Space dry-bulb temperature slot */
} heat_batch_desc;

typedef struct heat_batch heat_batch;

/* Options for heat_batch_create_ex. Zero-initialise for defaults. */
typedef struct heat_batch_options {
    int32_t device;          /* HIP device ordinal; -1 = current device */
    int32_t force_general;   /* 1: route every surface through the general (catch-all) kernel */
    int32_t nodes_per_lane;  /* 0 = auto; else 4, 8 or 16 (fast-path blocking factor) */
    int32_t use_graph;       /* 1: replay the sub-timestep as a hipGraph inside heat_batch_march */
    void *stream;            /* hipStream_t to run on; NULL = a stream owned by the batch */
    /* Multi-GPU (one process per GPU): this rank holds a shard of the surfaces but all zones.
     * With n_ranks > 1 the caller either gives the batch a communicator (heat_batch_comm_init, below) and
     * marches as on one GPU, or brings its own collective and alternates
     * heat_batch_step_surfaces -> all-gather of heat_batch_zone_partials -> heat_batch_step_zones. */
    int32_t n_ranks;
    int32_t rank;
    int32_t no_palette;      /* 1: keep dt/mass and U as per-node arrays even where a palette would do */
    int32_t no_fusion;       /* cluster-resident march (see heat_batch_set_fusion): 0 = plan it for the clusters the cost
                              * model expects to gain, 1 = never, 2 = for every cluster that structurally can (tests) */
} heat_batch_options;

/* ≙ ThermalModel::new + allocate_memory: validates, packs and uploads the constants. */
int heat_batch_create(const heat_batch_desc *desc, heat_batch **out);
int heat_batch_create_ex(const heat_batch_desc *desc, const heat_batch_options *opt, heat_batch **out);
void heat_batch_destroy(heat_batch *b);

/*
 * Weather sites: one batch of buildings from several climates, each site with its own weather. A batch of K sites is K
 * reference models marched in lockstep (model.rs:369-382 reads the weather once per sub-timestep; it reaches only the
 * Outdoor sides: t_out, model.rs:79-96; wind speed, convection.rs:157-167; wind direction, surface.rs:37-46).
 *   site_of_surface[n_surfaces]  the site of every surface, in [0, n_sites); 1 <= n_sites <= 65536
 * A count outside that range is refused with HEAT_E_INVALID_ARG, a site out of range with HEAT_E_SIZE (the message
 * names the surface), both before any device work; so is a sharded batch (opt->n_ranks > 1: HEAT_E_INVALID_ARG).
 * n_sites == 1 gives exactly the batch heat_batch_create_ex gives. On a batch of n_sites > 1 the `weather` argument of
 * heat_batch_march, heat_batch_march_ex, heat_batch_march_resident and heat_batch_set_weather holds n_sub * n_sites
 * records, sub-timestep-major: record [k * n_sites + s] is site s at sub-timestep k; a call of more than 2^24 records
 * (n_sub * n_sites) is refused with HEAT_E_INVALID_ARG. A batch has one dt (and each call
 * one n_sub) for all its sites: buildings whose models chose different time steps go to separate batches.
 * The planner gives every tile, cluster-resident workgroup and team surfaces of one site; a zone-connected cluster whose
 * surfaces belong to several sites is legal and is streamed.
 */
int heat_batch_create_sites(const heat_batch_desc *desc, const heat_batch_options *opt, int32_t n_sites,
                            const int32_t *site_of_surface, heat_batch **out);
int32_t heat_batch_n_sites(const heat_batch *b); /* 1 for a batch made without sites */

/* Copies every slot the path touches (node temperatures, hs, flows, irradiances, zone
 * dry-bulb) from / to the caller's SimulationState. */
int heat_batch_upload_state(heat_batch *b, const double *state, size_t n_state);
int heat_batch_download_state(heat_batch *b, double *state, size_t n_state);
/* Only what other modules write between two march calls: solar + IR irradiance slots
 * and zone dry-bulb temperatures. The zone slots are taken only while `state` holds what this path last computed
 * for them: after a march whose outputs left HEAT_OUT_ZONE_TEMPERATURES out (or a resident march without a download)
 * the caller's zone slots are older than the device's and are NOT read — heat_batch_upload_state takes everything. */
int heat_batch_upload_inputs(heat_batch *b, const double *state, size_t n_state);

/*
 * ≙ ThermalModel::march (model.rs:359-427): n_sub sub-timesteps. weather: n_sub records, or n_sub * n_sites records
 * [k * n_sites + s] on a batch of weather sites (heat_batch_create_sites).
 * zone_a0 / zone_b0 (nullable, [n_zones]) are the terms of calculate_zones_abc that do
 * not come from surfaces (HVAC, luminaires, infiltration, ventilation; model.rs:500-544),
 * evaluated by the caller.
 * Uploads the inputs from `state`, marches, downloads the outputs into `state`.
 */
int heat_batch_march(heat_batch *b, double *state, size_t n_state, const heat_weather *weather,
                     int32_t n_sub, const double *zone_a0, const double *zone_b0);
/* Data at this boundary: the call uploads only the slots other modules write between two marches
 * — the 4 S irradiance slots and the zones' dry-bulb slots, gathered on the host into pinned memory, one 32 MB copy
 * per million surfaces — and downloads only the outputs of this module, through two pinned staging halves with the
 * host scatter on a thread pool (HEAT_AMD_HOST_THREADS, default min(16, cores)) overlapping the copies.
 * heat_batch_march_ex chooses which outputs come back every call: a caller that reads the node temperatures only
 * now and then (they are 8 n of every surface's 8 n + 32 output bytes) leaves HEAT_OUT_NODE_TEMPERATURES out and
 * fetches them with heat_batch_download_outputs when needed; the device-resident state is always complete. */
enum heat_outputs {
    HEAT_OUT_NODE_TEMPERATURES = 1, /* SurfaceTrait::set_node_temperatures, surface_trait.rs:107-125 */
    HEAT_OUT_SURFACE_SCALARS = 2,   /* hs front / back, convective heat flow front / back (model.rs:154-169) */
    HEAT_OUT_ZONE_TEMPERATURES = 4, /* dry-bulb temperature of the zones this batch owns (model.rs:410-423) */
    HEAT_OUT_ALL = 7
};
/* (weather: as heat_batch_march — n_sub * n_sites records [k * n_sites + s] on a batch of weather sites) */
int heat_batch_march_ex(heat_batch *b, double *state, size_t n_state, const heat_weather *weather, int32_t n_sub,
                        const double *zone_a0, const double *zone_b0, int32_t what);
int heat_batch_download_outputs(heat_batch *b, double *state, size_t n_state, int32_t what);

/* Same, but on the device-resident state only (no host traffic; asynchronous on the batch's
 * stream until heat_batch_synchronize / a download). weather: as heat_batch_march (n_sub * n_sites records with sites). */
int heat_batch_march_resident(heat_batch *b, const heat_weather *weather, int32_t n_sub,
                              const double *zone_a0, const double *zone_b0);
int heat_batch_synchronize(heat_batch *b); /* waits, then reports device-side numerical flags */

/*
 * Series march: n_steps caller timesteps of n_sub sub-timesteps each in ONE call (model.rs:359-427 repeated, as the
 * reference's validation harness repeats it: validate_wall_heat_transfer.rs:615-711). Between two ThermalModel::march calls
 * only the weather, the irradiance slots and the zones' a0 / b0 terms change; for a free-running building all three are
 * known before the run starts. They are uploaded once as schedules; before step k the device sets that step's driven
 * inputs, after step k it records the probed slots into row k of a trace. The host enqueues every step without waiting
 * and synchronises once at the end.
 * Contract: the device state after the call and row k of the trace are what n_steps successive heat_batch_march_ex calls
 * give when the caller writes step k's inputs into its state before call k and reads the probed slots after it (inputs as
 * validate_wall_heat_transfer.rs:675-705 sets them). Without the own-face term the two are equal bit for bit: a step runs
 * the kernels of a call of n_sub on the same inputs (one multiplication per driven value).
 *   weather        n_steps * n_sub * n_sites records: [(k * n_sub + i) * n_sites + s] is site s at sub-timestep i of step k
 *                  (n_sites = 1 on a batch made without sites). More than 2^24 records PER STEP (n_sub * n_sites, on a
 *                  batch of several sites) are refused as in heat_batch_march.
 *   zone terms     n_zone_term_steps = 0: a0 = b0 = 0 in every step; 1: one row [n_zones] for every step; n_steps: row k
 *                  for step k (model.rs:500-544). With rows, a NULL zone_a0 or zone_b0 stands for zeros.
 *   driven inputs  surfaces are numbered as in the descriptor. The value of an input of surface s at step k is
 *                  gain[s] * channel[k * n_channels + chan[s]]; a NULL gain array is all ones. With chan[s] == -1, or a
 *                  NULL chan array, the input keeps the value the last upload or series put on the device: the matching
 *                  field of the side's device record (solar, or radiant temperature) is not written, also when the side's
 *                  other field is. The values pass through the clamps of surface.rs:916-923 and the long-wave conversion of
 *                  surface.rs:647,692 exactly as an uploaded slot does (the same device functions). Zone temperatures are
 *                  never driven: they are the path's own output.
 *   ir_own_face    (nullable) the long-wave feedback of the reference's harness (validate_wall_heat_transfer.rs:689-699):
 *                  with bit 0 / bit 1 of ir_own_face[s] set, SIGMA * (T + 273.15)^4 of the surface's own first / last node
 *                  temperature AT THE START OF THE STEP is added to its driven front / back long-wave irradiance. A bit on
 *                  a side whose long-wave channel is -1 is refused (HEAT_E_SIZE, naming the surface).
 *   probes         slots of the caller's SimulationState this path owns: node temperatures, hs and convective flow front /
 *                  back, zone dry-bulb. trace[k * n_probes + p] is slot probe_slot[p] after step k.
 * heat_series_check validates everything that needs no device, and heat_batch_march_series calls the same checks first,
 * before any device work: a NULL series, a negative count, a NULL array that a positive count needs ->
 * HEAT_E_INVALID_ARG; n_zone_term_steps other than 0, 1, n_steps -> HEAT_E_INVALID_ARG; a channel index outside
 * [-1, n_channels) -> HEAT_E_SIZE naming the surface; a probe slot that is not a node-temperature, hs, flow or zone slot of
 * the descriptor (an irradiance slot, a slot of another module) -> HEAT_E_SIZE naming the probe. A sharded batch
 * (n_ranks > 1) is refused with HEAT_E_INVALID_ARG, as heat_batch_create_sites refuses one; weather sites are supported.
 * n_steps == 0 marches nothing and sets nothing. n_sub == 0 with n_steps > 0 still sets the inputs and records the probes
 * of every step (model.rs:369: the loop body never runs). n_probes == 0 and n_channels == 0 are legal (trace may be NULL
 * when it has no element).
 * A numerical failure is reported as heat_batch_synchronize reports it (same codes; heat_batch_failed_surface works);
 * *failed_step (nullable) is the first step after which the failure flags were set, -1 when there was none. Trace rows from
 * that step on are unspecified. The call returns after one synchronisation, with the trace on the host; the device state is
 * complete (heat_batch_download_state / _outputs fetch anything else) and the caller's zone slots are older than the
 * device's, as after a resident march without a download (heat_batch_upload_inputs). The schedules live on the device for
 * the duration of the call; one too large for it fails with HEAT_E_DEVICE before anything is marched — cut the run into
 * several series: a series of k steps followed by one of n - k gives the same bits as one of n.
 */
typedef struct heat_series {
    int32_t n_steps;            /* caller timesteps (march calls) in this series, >= 0 */
    int32_t n_sub;              /* sub-timesteps per step (ThermalModel::dt_subdivisions), >= 0 */
    const heat_weather *weather;/* n_steps * n_sub * n_sites records, [(k * n_sub + i) * n_sites + s] */
    int32_t n_zone_term_steps;  /* 0 (none), 1 (one row for every step) or n_steps */
    const double *zone_a0, *zone_b0;      /* [n_zone_term_steps][n_zones] */
    int32_t n_channels;
    const double *channel;                /* [n_steps][n_channels] */
    const int32_t *solar_front_chan, *solar_back_chan, *ir_front_chan, *ir_back_chan;   /* [n_surfaces]; -1 / NULL: not driven */
    const double *solar_front_gain, *solar_back_gain, *ir_front_gain, *ir_back_gain;    /* [n_surfaces]; NULL = 1 */
    const uint8_t *ir_own_face;           /* [n_surfaces], nullable */
    int64_t n_probes;
    const int64_t *probe_slot;            /* [n_probes] */
} heat_series;

int heat_series_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s); /* host-only */
int heat_batch_march_series(heat_batch *b, const heat_series *s, double *trace /* [n_steps][n_probes] */,
                            int32_t *failed_step);

/*
 * Zone loads of a series: the terms of calculate_zones_abc that do not come from surfaces (model.rs:500-544), formed ON THE
 * DEVICE at every step from the series' channel table and a few constants per term, instead of [n_steps][n_zones] rows of
 * zone_a0 / zone_b0 the caller computes in advance — and thermostats, which need the zone temperatures the device holds at
 * the start of the step and so cannot be a schedule at all. The reference forms the heater, luminaire, infiltration and
 * ventilation terms (model.rs:500-544, air properties gas.rs:49,165-179); it has NO controller (its IdealHeaterCooler is
 * a todo!(), heating_cooling.rs:66-119): the control law below is this library's own contract, defined — as the series is —
 * against the per-call loop with the same rule applied by the host between the calls.
 * Step k, after the step's head (weather, zone-term row) and before its sub-timesteps; T = the zone temperatures the device
 * holds at that moment (what step k - 1 left; for step 0 the state as it is); row = channel[k]:
 *   1. a0[z], b0[z] start from the series' own zone-term row (zeros without rows).
 *   2. gains of zone z, in the caller's order:       a0[z] += gain_factor[i] * row[gain_chan[i]]
 *   3. air flows of zone z, in the caller's order:   V = flow_volume_gain[i] * row[flow_volume_chan[i]]  (m3/s)
 *                                                    Tin = row[flow_temp_chan[i]]  (C),  Tk = Tin + 273.15
 *                                                    rho = 101325 * 28.97 / (8314.46261815324 * Tk)       (gas.rs:175-179)
 *                                                    cp = 1002.7370 + 1.2324e-2 * Tk                      (gas.rs:49,165-167)
 *                                                    m = (rho * V) * cp;   a0[z] += m * Tin;   b0[z] += m
 *   4. thermostats whose TARGET is zone z, in the caller's order, with Ts = T[th_sensor_zone[t]], d = th_band[t] / 2, mode
 *      the thermostat's mode byte, h / c = row[th_heat_chan[t]] / row[th_cool_chan[t]]:
 *        heating (only if th_heat_chan[t] >= 0):  Ts < h - d -> mode = 1;  else if mode == 1 and Ts > h + d -> mode = 0
 *        cooling (only if mode != 1 now and th_cool_chan[t] >= 0):
 *                                                 Ts > c + d -> mode = 2;  else if mode == 2 and Ts < c - d -> mode = 0
 *        power = +th_heat_power[t] in mode 1, -th_cool_power[t] in mode 2, 0 otherwise;
 *        a0[z] += power;  applied[k * n_thermostats + t] = power.
 *      A NaN setpoint makes every comparison false: the mode stays.
 *   5. The terms hold for all n_sub sub-timesteps of the step, as the zone_a0 / zone_b0 of a march call do.
 * Every product and sum above is ONE rounded f64 operation in the order written (no fused multiply-add): a host that applies
 * the same rule between heat_batch_march_ex calls gets the same bits. A NULL gain_factor / flow_volume_gain is all ones.
 * th_mode (in / out, nullable) carries the modes over a cut: a series of k steps followed by one of n - k with the returned
 * modes gives the bits of the series of n. NULL: every thermostat starts off and the modes are not returned.
 * heat_zone_loads_check (host-only) and heat_batch_march_series_loads run the same checks, all before any device work:
 * a negative count, a NULL array that a positive count needs (gain_factor, flow_volume_gain and th_mode may be NULL) ->
 * HEAT_E_INVALID_ARG; a zone outside [0, n_zones) or a channel outside [0, n_channels) (a setpoint channel may be -1, but
 * not both of a thermostat) -> HEAT_E_SIZE; a power or band that is negative or not finite, a mode byte above 2 ->
 * HEAT_E_INVALID_ARG. The message names "gain i", "flow i" or "thermostat i". A sharded batch is refused, as by
 * heat_batch_march_series. Weather sites need nothing: a site's outdoor temperature is a channel the caller fills.
 * l == NULL, or all three counts 0, is heat_batch_march_series(b, s, trace, failed_step) exactly. applied is nullable;
 * n_sub == 0 still evaluates the loads of every step. A term that turns a zone's a0 or b0 into NaN (a NaN channel value) is
 * a numerical failure of that step: HEAT_N_NAN_ZONE, heat_batch_failed_surface names the zone. (Here the series is stricter
 * than the per-call path: the zone update keeps the temperature of a zone whose b is NaN, model.rs:662-668, and a caller
 * that passes such terms to heat_batch_march_ex is told nothing.) After a numerical failure applied rows and modes from the
 * failed step on are unspecified, as the trace's are.
 */
typedef struct heat_zone_loads {
    /* gains (heaters, luminaires, people; model.rs:500-516): a0[zone] += factor * channel[k][chan] */
    int64_t n_gains;
    const int32_t *gain_zone, *gain_chan;
    const double *gain_factor; /* NULL = 1 */
    /* air flows (infiltration, ventilation; model.rs:522-544) */
    int64_t n_flows;
    const int32_t *flow_zone, *flow_volume_chan, *flow_temp_chan;
    const double *flow_volume_gain; /* NULL = 1 */
    /* thermostats: one sensor zone, one target zone */
    int64_t n_thermostats;
    const int32_t *th_sensor_zone, *th_target_zone, *th_heat_chan, *th_cool_chan; /* setpoint channels, -1: none */
    const double *th_heat_power, *th_cool_power, *th_band;                        /* W >= 0, W >= 0, K >= 0 */
    uint8_t *th_mode; /* in/out, nullable: 0 off, 1 heating, 2 cooling */
} heat_zone_loads;

int heat_zone_loads_check(const heat_batch_desc *desc, const heat_series *s, const heat_zone_loads *l); /* host-only */
int heat_batch_march_series_loads(heat_batch *b, const heat_series *s, const heat_zone_loads *l,
                                  double *trace /* [n_steps][n_probes] */,
                                  double *applied /* [n_steps][n_thermostats], nullable */, int32_t *failed_step);

/*
 * Report of a series: statistics and weighted group sums maintained ON THE DEVICE at every step, instead of a
 * [n_steps][n_probes] trace the caller reduces afterwards. Everything here is O(1) state per quantity, independent of
 * n_steps in memory and in transfer: a year of quarter-hour steps (35 040) reports on a million quantities without a trace.
 * heat_batch_march_series_report is the series with loads plus a report; r == NULL is heat_batch_march_series_loads exactly
 * (and l == NULL then heat_batch_march_series), with ONE difference: trace == NULL means "record no trace" — no
 * [n_steps][n_probes] buffer exists on the device, the probes still define quantities. Likewise applied == NULL keeps no
 * [n_steps][n_thermostats] buffer (one row of scratch where thermostat statistics need the powers).
 * Quantities: Q = n_probes + n_groups. Quantity q < n_probes is probe q of the series; quantity n_probes + g is group g.
 * Groups: group g is the entries [group_offset[g], group_offset[g + 1]) (CSR) of group_slot / group_weight; a slot is
 *   anything a probe may be (node temperature, hs, convective flow front / back, zone dry-bulb). The value of group g after
 *   step k is the sum of weight[i] * slot_i over its entries (group_weight == NULL: all ones); an empty group is 0.0.
 *   group_trace (nullable): group_trace[k * n_groups + g] is that value. The order of the summation is the library's: it is
 *   fixed by the group's own entries alone (sorted into device order, cut into segments of a fixed number of entries, a fixed
 *   tree inside a segment, the segments added in order) — never by launch geometry, timing, or the other groups and probes
 *   of the report. The same report on the same state gives the same bits, and with n entries
 *   |value - exact| <= n * 2^-52 * sum |weight[i] * slot_i|.
 * Statistics: every array is in/out and nullable; a NULL array is not maintained (and costs no traffic). With v the value of
 *   quantity q after step k and K = step_base + k, applied at every step in step order:
 *     q_min, q_step_min     if (v < min) { min = v; step_min = K; }      (strict: the first occurrence; a NaN never enters)
 *     q_max, q_step_max     if (v > max) { max = v; step_max = K; }
 *     q_sum                 sum = sum + v                                 (one rounded addition per step)
 *     q_n_below, q_deg_below, limit q_lo (input)   if (v < lo) { n += 1; deg = deg + (lo - v); }
 *     q_n_above, q_deg_above, limit q_hi (input)   if (v > hi) { n += 1; deg = deg + (v - hi); }
 *   A NaN limit never counts. q_step_min / q_step_max without q_min / q_max are refused (HEAT_E_INVALID_ARG), as is a count
 *   or degree array without its limit array. resume == 0: the library initialises on the device (min = +inf, max = -inf,
 *   steps = -1, sums and counts 0); resume != 0: the accumulators start from the caller's arrays. No fused multiply-add: a
 *   host applying the rules in a plain loop over the full trace gets the same bits, and a series of k steps followed by one
 *   of n - k with resume = 1 and step_base + k gives the bits of the series of n.
 * Thermostat statistics (only with loads and n_thermostats > 0; caller's thermostat order; same resume rule):
 *     th_steps_heating / th_steps_cooling   steps whose mode after the evaluation of the step is 1 / 2
 *     th_switches                           steps whose mode after the evaluation differs from the mode before it (before
 *                                           step 0: the incoming th_mode byte, 0 when th_mode is NULL)
 *     th_sum_heating / th_sum_cooling       sum = sum + applied over the steps with applied > 0 / applied < 0
 *   They equal the same loop over the returned applied rows and modes bit for bit.
 * heat_series_report_check (host-only; it also builds the group tables — ordered by kind, surface or zone and node, since
 * without a batch there is no device layout to order them by) and the march run the same checks before any device work: a
 * negative count, a NULL array a positive count needs, group_offset not starting at 0 or decreasing, a non-finite weight,
 * a count / degree array without its limit, a step array without its extremum, thermostat arrays without thermostats ->
 * HEAT_E_INVALID_ARG; a group slot that is none of this path's output slots -> HEAT_E_SIZE. The message names
 * "group g" or "group entry i". Sharded batches are refused as by the series.
 * n_steps == 0 touches nothing, not even with resume == 0. n_sub == 0 still evaluates every step's report, on the unchanged
 * state. failed_step, the return code and heat_batch_failed_surface behave as in the series, also with trace == NULL; after
 * a numerical failure every report output is unspecified from the failed step on, as the trace is.
 */
typedef struct heat_series_report {
    int32_t resume;             /* 0: accumulators initialised by the library; else: they start from the arrays below */
    int64_t step_base;          /* K = step_base + k is what q_step_min / q_step_max record */
    int64_t n_groups;
    const int64_t *group_offset;/* [n_groups + 1], CSR */
    const int64_t *group_slot;  /* [group_offset[n_groups]] */
    const double *group_weight; /* same length; NULL = 1 */
    double *group_trace;        /* [n_steps][n_groups], nullable */
    /* statistics, [n_probes + n_groups] each, in/out, nullable */
    double *q_min;
    int64_t *q_step_min;
    double *q_max;
    int64_t *q_step_max;
    double *q_sum;
    const double *q_lo;         /* input */
    int64_t *q_n_below;
    double *q_deg_below;
    const double *q_hi;         /* input */
    int64_t *q_n_above;
    double *q_deg_above;
    /* thermostat statistics, [n_thermostats] each, in/out, nullable */
    int64_t *th_steps_heating, *th_steps_cooling, *th_switches;
    double *th_sum_heating, *th_sum_cooling;
} heat_series_report;

int heat_series_report_check(const heat_batch_desc *desc, const heat_series *s, const heat_zone_loads *l /* nullable */,
                             const heat_series_report *r); /* host-only */
int heat_batch_march_series_report(heat_batch *b, const heat_series *s, const heat_zone_loads *l /* nullable */,
                                   heat_series_report *r /* nullable */, double *trace /* [n_steps][n_probes], nullable */,
                                   double *applied /* [n_steps][n_thermostats], nullable */, int32_t *failed_step);

/*
 * Ideal loads of a series: in EVERY SUB-TIMESTEP a zone with an ideal load receives exactly the power that brings it to its
 * setpoint, limited by a capacity, and that power is the result of the run — the heating and cooling demand of the zone and
 * its peak, which the dead-band thermostat of heat_zone_loads (a plant of fixed size switched once per step) cannot give.
 * The reference leaves this controller as a todo!() (IdealHeaterCooler, heating_cooling.rs:66-119): the rule below is this
 * library's own contract, defined against a host loop that runs iterate_surfaces, calculate_zones_abc and the rule in every
 * sub-timestep. It cannot be formed by the caller: it needs the surface sums of the sub-timestep it acts in.
 * Setpoints: h = channel[k][heat_chan[i]] and c = channel[k][cool_chan[i]] hold for all n_sub sub-timesteps of step k.
 * In each sub-timestep, after the surfaces, for the zone of load i (every other zone is updated as ever, model.rs:650-674):
 *   tc        the zone's temperature before the update
 *   s_a, s_b  the zone's surface sums (sum of h A T_face, sum of h A; model.rs:562-585) exactly as the streamed zone balance
 *             forms them: same lanes, same tree
 *   a0, b0    the step's zone terms, INCLUDING the gains, flows and thermostat powers of heat_zone_loads (evaluated first)
 * Every line is one rounded f64 operation in the order written, no fused multiply-add (zone_mcp: zone.rs:59-65):
 *   a = s_a + a0;  b = s_b + b0;  cz = zone_mcp(volume, tc);  q = 0;  ft = tc
 *   if (fabs(b) > 1e-9) {                        (model.rs:662-668: otherwise the zone keeps its temperature)
 *       r = a / b;  E = exp(((-b) * dt) / cz);  free = r + (tc - r) * E;  ft = free;  D = 1 - E
 *       if (D > 0) {
 *           if (heat_chan >= 0 && free < h) {
 *               need = (b * (h - tc * E)) / D - a
 *               q = need > heat_cap ? heat_cap : need;  if (!(q > 0)) q = 0
 *               if (q > 0) { if (q == need) ft = h;      (unsaturated: the zone IS at the setpoint, bit for bit)
 *                            else { a2 = a + q;  r2 = a2 / b;  ft = r2 + (tc - r2) * E;  n_sat_heating += 1 } }
 *           } else if (cool_chan >= 0 && free > c) {     (heating is looked at first; the mirror image)
 *               need = (b * (c - tc * E)) / D - a
 *               q = need < -cool_cap ? -cool_cap : need;  if (!(q < 0)) q = 0
 *               if (q < 0) { if (q == need) ft = c;
 *                            else { a2 = a + q;  r2 = a2 / b;  ft = r2 + (tc - r2) * E;  n_sat_cooling += 1 } }
 *           }
 *       }
 *   }
 *   zone_T = ft;  qsum[i] = qsum[i] + q          (qsum starts at 0.0 in every step)
 * A NaN setpoint makes every comparison false: the zone floats. A NaN ft is HEAT_N_NAN_ZONE with the zone's number, as in
 * the zone balance. After the step's last sub-timestep, with v = qsum[i] and K = step_base + k:
 *   ideal_q[k * n_loads + i] = v                 (divide by n_sub for the step's mean power in W)
 *   sum_heating += v where v > 0;  sum_cooling += v where v < 0            (one rounded addition per step)
 *   if (v > peak_heating) { peak_heating = v; step_peak_heating = K; }     (strict: the first occurrence)
 *   if (v < peak_cooling) { peak_cooling = v; step_peak_cooling = K; }
 * Every accumulator is in/out and nullable. resume == 0: the library initialises on the device (sums and counts 0,
 * peak_heating = -inf, peak_cooling = +inf, steps = -1); resume != 0: they start from the caller's arrays. n_sub == 0 gives
 * qsum = 0 in every step. The controller has no memory: a series of k steps followed by one of n - k with resume = 1 and
 * step_base + k gives the bits of the series of n (ideal_q, accumulators, trace and state).
 * heat_cap / cool_cap: W, >= 0, +inf = unlimited; a NULL array = all unlimited. A capacity of 0 never acts.
 * The zone of an ideal load may also be a thermostat's target or sensor, a gain or flow zone, a probe or a group entry.
 * Weather sites are supported. By default a series with ideal loads marches every sub-timestep streamed (surfaces, zone
 * sums, this rule): the cluster-resident march is not used for it, and the batch's fusion setting is left as it is for
 * later calls.
 * RESIDENT FORM, opt-in per batch (heat_batch_set_ideal_resident, below): the clusters the batch marches resident stay
 * resident in an ideal series, and the lane that finishes a zone in the cluster-resident march applies the rule above. The
 * rule is unchanged with ONE substitution: for the zones a workgroup owns, s_a, s_b (and the surfaces' march) are the
 * cluster-resident march's — its lanes, its tree — instead of the streamed zone balance's; the streamed remainder of the
 * batch keeps the streamed sums. Everything the rule makes exact stays exact (an unsaturated zone is at its setpoint bit for
 * bit, qsum is the sequential sum over the step's sub-timesteps from 0.0, the accumulators, cut and resume, run-to-run
 * identity), but the resident form is NOT bit-equal to the streamed form: the two differ by the rounding of the sums. A zone
 * without a load has, from the same inputs, the bits of the plain resident march. Without the opt-in nothing changes: the
 * same kernels, the same bits.
 * LIMIT: residency is decided for the WHOLE batch, once, from its plan — every resident launch the batch would make needs an
 * ideal instantiation of its kernel, so a batch with clusters marched by teams, with resident workgroups of walls only in a
 * class with gas cavities, or in a class with no-mass chunks other than facings marches its ideal series streamed as before, batch-wide
 * (heat_plan_ideal_resident names the reason; with HEAT_AMD_TRACE set the series says so once). Routing only those classes
 * to the streamed leg for one call is not done: what is streamed and what is resident is fixed when the batch is created.
 * The call-length rule of the plain march applies: n_sub = 1 on a batch of more than 8 192 surfaces streams.
 * heat_ideal_loads_check (host-only) and heat_batch_march_series_ideal run the same checks before any device work; every
 * message names "ideal load i": a negative count, a NULL array a positive count needs (zone, heat_chan, cool_chan), a step
 * array without its peak array, a capacity that is negative or NaN, a second load on a zone -> HEAT_E_INVALID_ARG; a zone
 * outside [0, n_zones), a channel outside [-1, n_channels), a load with neither setpoint channel -> HEAT_E_SIZE. Sharded
 * batches are refused as by the series.
 * heat_batch_march_series_ideal with il == NULL or n_loads == 0 is heat_batch_march_series_report exactly (same kernels,
 * same bits); ideal_q is nullable. After a numerical failure ideal_q rows and accumulators from the failed step on are
 * unspecified, as the trace is.
 */
typedef struct heat_ideal_loads {
    int64_t n_loads;
    const int32_t *zone;                   /* [n_loads], at most one load per zone */
    const int32_t *heat_chan, *cool_chan;  /* setpoint channels of the series, -1: none (not both) */
    const double *heat_cap, *cool_cap;     /* W, >= 0, +inf = unlimited; NULL = unlimited */
    int32_t resume;                        /* as heat_series_report::resume, for the arrays below */
    int64_t step_base;
    /* accumulators, [n_loads] each, in/out, nullable */
    double *sum_heating, *sum_cooling;     /* sum over steps of the step's q-sum, by sign */
    double *peak_heating; int64_t *step_peak_heating;   /* largest step q-sum, first occurrence */
    double *peak_cooling; int64_t *step_peak_cooling;   /* most negative step q-sum */
    int64_t *n_sat_heating, *n_sat_cooling;             /* SUB-timesteps that ended at the capacity */
} heat_ideal_loads;

int heat_ideal_loads_check(const heat_batch_desc *desc, const heat_series *s, const heat_ideal_loads *il); /* host-only */
int heat_batch_march_series_ideal(heat_batch *b, const heat_series *s, const heat_zone_loads *l /* nullable */,
                                  heat_ideal_loads *il /* nullable */, heat_series_report *r /* nullable */,
                                  double *trace /* [n_steps][n_probes], nullable */,
                                  double *applied /* [n_steps][n_thermostats], nullable */,
                                  double *ideal_q /* [n_steps][n_loads], nullable */, int32_t *failed_step);

/*
 * Sky of a series: the incident solar and long-wave irradiance of sky-facing sides, formed ON THE DEVICE at every step from
 * one 64-byte record per site and step (the sun's direction, three short-wave and two long-wave irradiances) and the
 * surface's normal, instead of one channel column per distinct (site, orientation) the caller computes in advance: with a
 * random azimuth per wall that is one column per wall. The reference has no counterpart — solar geometry lives in another
 * SIMPLE crate and its harness reads EnergyPlus' incident irradiance from CSV (validate_wall_heat_transfer.rs:675-705): the
 * rule below is this library's own contract, defined — as the thermostat and the ideal load are — against the per-call loop
 * with the same rule written on the host (heat_amd/sky.py, incident()).
 * For a side whose mode bit is set, with n = the front normal (its component-wise negation for the back side) and r = the
 * record of the surface's site at step k; every line is one rounded f64 operation in the order written, no fused
 * multiply-add:
 *   c   = (n.x * r.sun_x + n.y * r.sun_y) + n.z * r.sun_z
 *   fs  = 0.5 + 0.5 * n.z          fg = 0.5 - 0.5 * n.z
 *   solar:      bm = c > 0 ? r.beam * c : 0.0
 *               v  = (bm + r.diffuse * fs) + r.ground * fg
 *   long-wave:  v  = r.ir_sky * fs + r.ir_ground * fg
 *   if the series carries the gain array of that input:  v = v * gain[s]
 * From v on the value is the raw value of a driven input of the series: into the state mirror where the batch keeps one,
 * through the clamps of surface.rs:916-923 and the side's absorptance factor or the long-wave conversion of
 * surface.rs:647,692 (the same device functions), into the side's device record. A field that is neither sky-driven nor
 * channel-driven is not written. The model is an isotropic sky with a ground view of 1 - fs; anisotropic skies, shading and
 * sun-position formulas are the caller's (it supplies the sun vector, which keeps the rule free of transcendental functions:
 * the host reproduces the bits). A NaN in a record is treated as a NaN channel value is. The sky has no memory: a series of k
 * steps followed by one of n - k gives the bits of the series of n. n_sub == 0 still sets the inputs of every step.
 * heat_sky_check (host-only) and heat_batch_march_series_sky run the same checks before any device work; every message names
 * "surface s": a NULL mode, NULL normals while some mode byte is not 0, a NULL record while some mode byte is not 0 and
 * n_steps > 0, a normal component that is not finite on a surface whose mode is not 0, a mode byte above 15 ->
 * HEAT_E_INVALID_ARG; a mode bit on an input whose channel in the series is >= 0 (an input has one source) -> HEAT_E_SIZE.
 * An ir_own_face bit on a sky-driven side is refused by the series (it needs a channel). Sharded batches are refused as by
 * the series; weather sites are supported (n_sites is the batch's).
 * heat_batch_march_series_sky with sky == NULL, or with every mode byte 0, is heat_batch_march_series_ideal exactly (same
 * kernels, same bits).
 */
typedef struct heat_sky_record {   /* one site at one step; 64 bytes */
    double sun_x, sun_y, sun_z;    /* vector towards the sun, in the axes of the surfaces' normals (z up) */
    double beam;                   /* direct normal irradiance, W/m2 */
    double diffuse;                /* diffuse horizontal irradiance, W/m2 */
    double ground;                 /* short-wave irradiance leaving the ground (albedo x global horizontal), W/m2 */
    double ir_sky;                 /* horizontal infrared irradiance from the sky, W/m2 */
    double ir_ground;              /* long-wave irradiance leaving the ground, W/m2 */
} heat_sky_record;

typedef struct heat_sky {
    const heat_sky_record *record;                 /* [n_steps][n_sites]: [k * n_sites + site] */
    const double *normal_x, *normal_y, *normal_z;  /* [n_surfaces] outward normal of the FRONT face; the back face sees its negation */
    const uint8_t *mode;                           /* [n_surfaces] bit 0 solar front, 1 solar back, 2 long-wave front, 3 long-wave back */
} heat_sky;

int heat_sky_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky); /* host-only */
int heat_batch_march_series_sky(heat_batch *b, const heat_series *s, const heat_sky *sky /* nullable */,
                                const heat_zone_loads *l /* nullable */, heat_ideal_loads *il /* nullable */,
                                heat_series_report *r /* nullable */, double *trace, double *applied, double *ideal_q,
                                int32_t *failed_step);

/*
 * Solar gains of a series: the solar radiation that enters a room THROUGH ITS WINDOWS and lands on the room's inside faces,
 * formed on the device at every step from the sky's per-site records — instead of one channel column per inside face the
 * caller computes in advance. The reference computes this term in another SIMPLE crate; the rule below is this library's own
 * contract, defined — as the sky is — against the per-call loop with the same rule written on the host
 * (heat_amd/solar_gains.py, transmitted() and received()).
 * An APERTURE a is a window seen from the sky: ap_surface (used only for its weather site), the outward normal n of the
 * side that sees the sky, a beam transmittance as a polynomial of degree 5 in the cosine of incidence
 * (ap_tau_coef[a][0..5], constant term first), a hemispherical transmittance and a scale in m2 (area x frame or shading
 * factor). With r = sky->record[k][site of ap_surface[a]]; every line is ONE rounded f64 operation in the order written, no
 * fused multiply-add:
 *   c  = (n.x * r.sun_x + n.y * r.sun_y) + n.z * r.sun_z
 *   fs = 0.5 + 0.5 * n.z          fg = 0.5 - 0.5 * n.z
 *   t  = coef[5];  for j = 4 .. 0:  t = t * c;  t = t + coef[j]
 *   ib = r.beam * c
 *   Pb = c > 0 ? (ib * t) * scale : 0.0                  (W, beam; a NaN cosine is no beam, as in the sky)
 *   id = r.diffuse * fs + r.ground * fg
 *   Pd = (id * tau_diffuse) * scale                      (W, diffuse + ground-reflected)
 *   P  = Pb + Pd;  transmitted[k][a] = P;  ap_sum[a] = ap_sum[a] + P
 * t is not clamped: the polynomial is the caller's. ap_sum (in/out, nullable) is added onto what the caller passes in: a
 * series of k steps followed by one of n - k with the returned array gives the bits of the series of n.
 * An ENTRY i gives a receiver — the side en_side[i] (0 front, 1 back) of surface en_surface[i] — the shares en_beam[i] and
 * en_diffuse[i] (1/m2: the share of the aperture's beam or diffuse power that lands on the receiver, divided by the
 * receiver's area) of aperture en_aperture[i]. Entries come in any order; the raw solar value of a receiver is formed over
 * ITS entries in the caller's order:
 *   v = 0.0;   per entry:  v = v + en_beam[i] * Pb[a_i];   v = v + en_diffuse[i] * Pd[a_i]
 *   if the series carries that input's gain array:  v = v * gain[s]
 * From v on the value is the raw value of a driven solar input of the series: into the state mirror where the batch keeps
 * one, through the clamps of surface.rs:916-923, times the side's absorptance factor, into the solar field of the side's
 * device record. The side's long-wave field is never written here, and a side without entries is not written at all.
 * An input has ONE source: the solar input of a receiver has channel -1 in the series and no solar mode bit in the sky.
 * The rule has no memory beyond ap_sum; n_sub == 0 still sets the inputs of every step; a NaN in a record or table
 * propagates as a NaN channel value does.
 * heat_solar_gains_check (host-only; it also lays out and verifies the tables the march uploads) and
 * heat_batch_march_series_gains run the same checks before any device work; every message names "aperture a" or "entry i":
 * a negative count, a NULL array a positive count needs (ap_sum may be NULL), n_apertures > 0 with n_steps > 0 and no sky or
 * no sky->record, a normal, coefficient, scale, transmittance or share that is not finite, a side byte above 1 ->
 * HEAT_E_INVALID_ARG; a surface or aperture index out of range, a receiver whose solar input already has a channel or a sky
 * bit -> HEAT_E_SIZE. Sharded batches are refused as by the series; weather sites are supported.
 * heat_batch_march_series_gains with gains == NULL, or with n_apertures == 0 and n_entries == 0, is
 * heat_batch_march_series_sky exactly (same kernels, same bits).
 */
typedef struct heat_solar_gains {
    int64_t n_apertures;
    const int64_t *ap_surface;                              /* [n_apertures] the window's surface: its site's record is read */
    const double *ap_normal_x, *ap_normal_y, *ap_normal_z;  /* [n_apertures] outward normal of the side that sees the sky */
    const double *ap_tau_coef;                              /* [n_apertures][6] beam transmittance, constant term first */
    const double *ap_tau_diffuse;                           /* [n_apertures] hemispherical transmittance */
    const double *ap_scale;                                 /* [n_apertures] m2 */
    double *ap_sum;                                         /* [n_apertures] in/out, nullable: sum of P over the steps, W */
    int64_t n_entries;
    const int64_t *en_surface;                              /* [n_entries] the receiver's surface */
    const uint8_t *en_side;                                 /* [n_entries] 0 front, 1 back */
    const int32_t *en_aperture;                             /* [n_entries] */
    const double *en_beam, *en_diffuse;                     /* [n_entries] 1/m2 */
} heat_solar_gains;

int heat_solar_gains_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky,
                           const heat_solar_gains *gains); /* host-only */
int heat_batch_march_series_gains(heat_batch *b, const heat_series *s, const heat_sky *sky /* nullable */,
                                  const heat_solar_gains *gains /* nullable */, const heat_zone_loads *l /* nullable */,
                                  heat_ideal_loads *il /* nullable */, heat_series_report *r /* nullable */, double *trace,
                                  double *applied, double *ideal_q,
                                  double *transmitted /* [n_steps][n_apertures], nullable */, int32_t *failed_step);

/*
 * Air paths of a series: air that moves BETWEEN ZONES — a doorway, a transfer grille, the vent of a Trombe wall — and vents
 * that open and close on the state of both of their ends: night ventilation, a window that opens when the room is too warm
 * and the air outside is cooler. It is the one term of calculate_zones_abc the reference marks and leaves empty
 * ("Mixing with other zones", "AIR MIXTURE WITH OTHER ZONES ... unimplemented()", model.rs:546,592-593): the rule below is
 * this library's own contract, defined — as the thermostat is — against the per-call loop with the same rule applied by the
 * host between the calls (heat_amd/air_paths.py, apply()). Like a thermostat it cannot be a schedule: what the target
 * receives is m * T of the source zone, a temperature the device holds; the flows of heat_zone_loads read volume and
 * temperature from channels and can express none of it.
 * A PATH i carries air from source[i] — a zone, or -1: supply air at row[temp_chan[i]] — into target[i]. Balanced exchange
 * between two zones is TWO paths; that is the caller's business. Step k, after step 4 of the zone loads (thermostats) and
 * before the driven inputs and the sub-timesteps; T = the zone temperatures the device holds then (what step k - 1 left;
 * nothing on the step's head writes them), row = channel[k]. Per target zone the paths are taken in the caller's order.
 * Every line is ONE rounded f64 operation in the order written, no fused multiply-add:
 *   Tt = T[target];  Ts = source >= 0 ? T[source] : row[temp_chan]
 *   controlled (open_chan non-NULL and open_chan[i] >= 0):  set = row[open_chan];  d = band / 2;  s = sense (+1.0 / -1.0)
 *       e = s * (Tt - set)                        how far the target is beyond its setpoint
 *       g = s * (Tt - Ts)                         how much the source helps
 *       if      e > d  and g > min_delta           state = 1
 *       else if state == 1 and (e < -d or g <= 0)  state = 0
 *     (a NaN makes every comparison false: the state stays)
 *   uncontrolled: open, whatever the state byte says; the byte is left as it is
 *   closed:  q = 0.0, nothing is added to a0 / b0
 *   open:    V = volume_gain * row[volume_chan]  (m3/s);  Tk = Ts + 273.15
 *            rho = 101325 * 28.97 / (8314.46261815324 * Tk);  cp = 1002.7370 + 1.2324e-2 * Tk;  m = (rho * V) * cp
 *                                                 (exactly the expressions and grouping of step 3 of heat_zone_loads)
 *            mt = m * Ts;  a0[target] = a0[target] + mt;  b0[target] = b0[target] + m
 *            dT = Ts - Tt;  q = m * dT            (W: what the path brings the target at the start of the step)
 *   path_q[k * n_paths + i] = q;  sum_q[i] = sum_q[i] + q;  steps_open[i] += open;  switches[i] += (state after != before)
 * sense = +1 is a cooling vent (it wants a source colder than the target, which is above its setpoint), -1 a heating vent.
 * path_q, the accumulators and state are in the caller's path order. The terms hold for all n_sub sub-timesteps of the step,
 * as every other a0 / b0 term does: ideal loads see them. EVERY source is read as it was at the START of the step, whatever
 * the order of the zones: a chain A -> B -> C does not propagate within a step. An uncontrolled path counts as open in
 * steps_open and never switches. The accumulators add onto what the caller passes in, as ap_sum does, and state carries the
 * controllers over a cut: a series of k steps followed by one of n - k with the returned arrays gives the bits of the series
 * of n. state == NULL: every controlled path starts closed and the states are not returned. n_sub == 0 still evaluates the
 * paths of every step. A term that turns a zone's a0 or b0 into NaN (a NaN volume on an open path) is a numerical failure of
 * that step: HEAT_N_NAN_ZONE, heat_batch_failed_surface names the zone, as for the zone loads; path_q rows, accumulators and
 * states from the failed step on are unspecified, as the trace is.
 * heat_air_paths_check (host-only; it also builds and verifies the tables the march uploads) and
 * heat_batch_march_series_air run the same checks before any device work; every message names "air path i": a negative
 * count, a NULL array a positive count needs (target, source, volume_chan; sense, band and min_delta where some path is
 * controlled), source == target, a band, min_delta or volume_gain that is not finite, a negative band or min_delta, a sense
 * other than +1 / -1 on a controlled path, a state byte above 1 -> HEAT_E_INVALID_ARG; a zone outside [0, n_zones) (a source
 * outside [-1, n_zones)), a volume channel outside [0, n_channels), an open channel outside [-1, n_channels), a source of -1
 * without a temperature channel in [0, n_channels), a temperature channel other than -1 on a path whose source is a zone (an
 * input has ONE source) -> HEAT_E_SIZE. Sharded batches are refused as by the series; weather sites need nothing.
 * heat_batch_march_series_air with air == NULL or n_paths == 0 is heat_batch_march_series_gains exactly (same launches, same
 * bits); path_q is nullable, and an array that is not asked for costs no traffic and changes no bit of the others.
 */
typedef struct heat_air_paths {
    int64_t n_paths;
    const int32_t *target;        /* [n_paths] zone that receives the air */
    const int32_t *source;        /* [n_paths] zone the air comes from, or -1: supply air at row[temp_chan] */
    const int32_t *temp_chan;     /* [n_paths] nullable when no source is -1; must be -1 where source >= 0 */
    const int32_t *volume_chan;   /* [n_paths] m3/s */
    const double  *volume_gain;   /* [n_paths] nullable = 1 */
    const int32_t *open_chan;     /* [n_paths] nullable / -1: uncontrolled, always open; else the target's setpoint, C */
    const int8_t  *sense;         /* [n_paths] +1 cooling (wants a colder source), -1 heating; read only where controlled */
    const double  *band;          /* [n_paths] K, >= 0; read only where controlled */
    const double  *min_delta;     /* [n_paths] K, >= 0; read only where controlled */
    uint8_t *state;               /* [n_paths] in/out, nullable (= all closed): 0 closed, 1 open */
    double  *sum_q;               /* [n_paths] in/out, nullable: sum over the steps of q, W */
    int64_t *steps_open;          /* [n_paths] in/out, nullable */
    int64_t *switches;            /* [n_paths] in/out, nullable */
} heat_air_paths;

int heat_air_paths_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_air_paths *air); /* host-only */
int heat_batch_march_series_air(heat_batch *b, const heat_series *s, const heat_sky *sky /* nullable */,
                                const heat_solar_gains *gains /* nullable */, const heat_zone_loads *l /* nullable */,
                                heat_air_paths *air /* nullable */, heat_ideal_loads *il /* nullable */,
                                heat_series_report *r /* nullable */, double *trace, double *applied, double *ideal_q,
                                double *transmitted, double *path_q /* [n_steps][n_paths], nullable */, int32_t *failed_step);

/*
 * Shades of a series: the SUNLIT FRACTION of the beam on a rectangle under an overhang, between side fins and behind a site's
 * horizon, formed on the device at every step from the sun vector of the sky's per-site record — instead of one channel column
 * per shaded side the caller computes in advance (an aperture cannot express it at all: its ap_scale is constant over the
 * series). The reference has no counterpart; the rule below is this library's own contract, defined — as the sky is — against
 * the per-call loop with the same rule written on the host (heat_amd/shading.py, sunlit()).
 * A SHADE j is a self-contained geometric device: the plane of a rectangle W wide and H high with outward normal n, the
 * in-plane horizontal axis u (to the right seen from outside) and the in-plane upward axis v (u = v x n; the caller supplies
 * all three, heat_amd/shading.py frame_of() builds u and v); a horizontal plate of overhang_depth, overhang_gap above the
 * rectangle's top edge and unbounded along u; a fin of fin_pos_depth, fin_pos_gap beside the +u edge and one of fin_neg_depth,
 * fin_neg_gap beside the -u edge, both unbounded along v (a depth of 0: the device is absent); optionally a horizon profile
 * p = sh_horizon[j]: tan^2 of the obstruction's elevation in 16 sectors of 22.5 degrees, counter-clockwise from east
 * (horizon_tan2[p][0] covers azimuths [0, 22.5) degrees from the x axis towards y). sh_surface[j] is used only for its
 * weather site, as ap_surface is. With (sx, sy, sz) = the sun vector of sky->record[k][site of sh_surface[j]]; every line is
 * ONE rounded f64 operation in the order written, no fused multiply-add, no square root, no transcendental function;
 * max(a, b) is (b > a ? b : a) and min(a, b) is (b < a ? b : a) — the FIRST operand where the comparison is false, so a NaN
 * first operand stays:
 *   c  = (n.x * sx + n.y * sy) + n.z * sz;   us = (u.x * sx + u.y * sy) + u.z * sz;   vs = (v.x * sx + v.y * sy) + v.z * sz
 *   overhang:  drop = (overhang_depth * vs) / c;  sh = drop - overhang_gap;  sh = max(sh, 0.0);  sh = min(sh, H)
 *              fv = vs > 0 ? (H - sh) / H : 1.0
 *   fins:      ap = (fin_pos_depth * us) / c;  wp = ap - fin_pos_gap;  wp = max(wp, 0.0);  wp = min(wp, W)
 *              nu = -us;  an = (fin_neg_depth * nu) / c;  wn = an - fin_neg_gap;  wn = max(wn, 0.0);  wn = min(wn, W)
 *              sw = us > 0 ? wp : (us < 0 ? wn : 0.0);  fh = (W - sw) / W
 *   f = fv * fh
 *   horizon (p >= 0):
 *              ax = |sx|;  ay = |sy|;  T = 0.41421356237309503   (tan 22.5 degrees)
 *              m = (ay > T * ax) + (ay > ax) + (T * ay > ax)
 *              sector = sx >= 0 ? (sy >= 0 ? m : 15 - m) : (sy >= 0 ? 7 - m : 8 + m)
 *              h2 = sx * sx + sy * sy;  lit = sz > 0 and sz * sz > horizon_tan2[p][sector] * h2;  if not lit: f = 0.0
 *   if not (c > 0): f = 0.0                  (the sun behind the plane, or a NaN: no beam, as in the sky)
 *   sunlit[k * n_shades + j] = f
 * A sun exactly on a sector boundary belongs to the sector the comparisons give (sy == 0, sx > 0: sector 0; sx == sy > 0:
 * sector 1; sx == 0, sy > 0: sector 3). Whatever the sun vector holds, the sector is in [0, 16).
 * The consumers refer to shades by number; one shade may serve several of them, and the cosine of a consumer stays its own,
 * from its own normal:
 *   a sky-driven solar side (heat_sky, mode bit 0 / 1) with front_shade[s] / back_shade[s] = j:
 *       bm = c > 0 ? r.beam * c : 0.0;  bm = bm * f;  dv = (r.diffuse * fs) * diffuse_factor[j]
 *       gv = (r.ground * fg) * ground_factor[j];  v = (bm + dv) + gv          (then the gain, mirror, clamp, absorptance)
 *   an aperture (heat_solar_gains) with aperture_shade[a] = j:
 *       Pb = c > 0 ? ((ib * t) * scale) * f : 0.0
 *       id = (r.diffuse * fs) * diffuse_factor[j] + (r.ground * fg) * ground_factor[j]      (Pd, P, transmitted, ap_sum as before)
 *   a side or aperture without a shade (-1, or a NULL array) follows the rule of heat_sky / heat_solar_gains: today's bits.
 * diffuse_factor / ground_factor are constant factors on the diffuse and the ground-reflected part (the sky and ground view
 * the devices leave); NULL = 1. A shade has no memory: a series of k steps followed by one of n - k gives the bits of the
 * series of n. n_sub == 0 still evaluates the shades of every step. A shade reads ITS OWN site's record — that of
 * sh_surface[j] — whatever the site of the side or aperture that refers to it: a shade shared across sites gives every
 * consumer the sunlit fraction under the sun of the shade's site.
 * heat_shades_check (host-only) and heat_batch_march_series_shaded run the same checks before any device work; every message
 * names "shade j", "horizon p", "surface s" or "aperture a": a negative count, a NULL array a positive count needs
 * (diffuse_factor, ground_factor, sh_horizon, front_shade, back_shade, aperture_shade may be NULL), n_shades > 0 with
 * n_steps > 0 and no sky or no sky->record, a vector component, width, height, depth, gap, factor or tan2 that is not
 * finite, a width or height that is not positive, a negative depth, gap or tan2, an aperture_shade without gains ->
 * HEAT_E_INVALID_ARG; sh_surface outside [0, n_surfaces), a shade number outside [-1, n_shades), a horizon number outside
 * [-1, n_horizons), a front_shade / back_shade on a side whose solar mode bit in the sky is not set -> HEAT_E_SIZE. Sharded
 * batches are refused as by the series; weather sites are supported.
 * heat_batch_march_series_shaded with shades == NULL or n_shades == 0 is heat_batch_march_series_air exactly (same launches,
 * same bits); sunlit is nullable.
 */
typedef struct heat_shades {
    int64_t n_shades;
    const int64_t *sh_surface;        /* [n_shades] used only for its weather site, as ap_surface is */
    const double *sh_normal_x, *sh_normal_y, *sh_normal_z;   /* outward normal n of the shaded plane */
    const double *sh_right_x, *sh_right_y, *sh_right_z;      /* u: in-plane horizontal axis, to the right seen from outside (u = v x n) */
    const double *sh_up_x, *sh_up_y, *sh_up_z;               /* v: in-plane upward axis */
    const double *sh_width, *sh_height;                      /* W, H of the shaded rectangle, m, > 0 */
    const double *overhang_depth, *overhang_gap;             /* horizontal plate above the top edge, unbounded along u; depth 0: none */
    const double *fin_pos_depth, *fin_pos_gap;               /* fin beside the +u edge, unbounded along v */
    const double *fin_neg_depth, *fin_neg_gap;               /* fin beside the -u edge */
    const double *diffuse_factor, *ground_factor;            /* nullable = 1: constant factors on the diffuse / ground part */
    const int32_t *sh_horizon;                               /* nullable / -1: no horizon profile */
    int64_t n_horizons;
    const double *horizon_tan2;       /* [n_horizons][16] tan^2 of the obstruction's elevation per 22.5 degree sector */
    const int32_t *front_shade, *back_shade;   /* [n_surfaces], nullable / -1: the side's sky-driven solar input is unshaded */
    const int32_t *aperture_shade;             /* [gains->n_apertures], nullable / -1 */
} heat_shades;

int heat_shades_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky,
                      const heat_solar_gains *gains, const heat_shades *shades); /* host-only */
int heat_batch_march_series_shaded(heat_batch *b, const heat_series *s, const heat_sky *sky /* nullable */,
                                   const heat_shades *shades /* nullable */, const heat_solar_gains *gains /* nullable */,
                                   const heat_zone_loads *l /* nullable */, heat_air_paths *air /* nullable */,
                                   heat_ideal_loads *il /* nullable */, heat_series_report *r /* nullable */, double *trace,
                                   double *applied, double *ideal_q, double *transmitted, double *path_q,
                                   double *sunlit /* [n_steps][n_shades], nullable */, int32_t *failed_step);

/*
 * Room radiation of a series: the LONG-WAVE IRRADIANCE of a side that faces a room, formed on the device at every step from
 * the emission of the other faces of its room — temperatures only the device holds, at the moment the step starts — instead
 * of a channel the caller computed in advance, the sky (which is for outside faces) or ir_own_face (where a face sees only
 * itself). Like a thermostat or an air path it cannot be a schedule at all. The reference has no counterpart (its harness
 * feeds EnergyPlus' long-wave columns plus the own-face term, validate_wall_heat_transfer.rs:689-699); the rule below is this
 * library's own contract, defined against the per-call loop with the same rule written on the host
 * (heat_amd/room_radiation.py, emitted() and irradiance()).
 * A RECEIVER r is a side whose long-wave input the rule forms: rc_side[r] (0 front, 1 back) of surface rc_surface[r]. An ENTRY
 * i gives receiver en_receiver[i] one term: the emission of an EMITTER side, en_side[i] of surface en_surface[i] — or, with
 * en_surface[i] == -1, the value of channel en_chan[i] (a radiant panel, the radiant part of an internal gain; W/m2) — weighted
 * by en_factor[i]: a view factor times whatever emissivity convention the caller uses, any finite number, the caller's
 * business. Entries come in any order; a receiver's sum runs over its entries in the caller's order. An emitter may be the
 * receiver itself, and a side in another zone or at another site.
 * Step k, behind the solar gains' receivers and before the ideal loads' begin; Tn = the node temperatures the device holds
 * then (what step k - 1 left; for step 0 the state as it is — nothing on the step's head writes them), row = channel[k];
 * every line is ONE rounded f64 operation in the order written, no fused multiply-add:
 *   emitter (surface e, side d):  tk = Tn[first node of e if d == 0, last node if d == 1] + 273.15
 *                                 t2 = tk * tk;  t4 = t2 * t2;  E = 5.670374419e-8 * t4
 *   receiver r:                   v = 0.0
 *     per entry i of r:           x = en_factor[i] * (en_surface[i] >= 0 ? E(en_surface[i], en_side[i]) : row[en_chan[i]])
 *                                 v = v + x
 *     if the series carries that input's gain array (ir_front_gain / ir_back_gain):  v = v * gain[s]
 *   irradiance[k * n_receivers + r] = v;   sum_irradiance[r] = sum_irradiance[r] + v
 * From v on it is the raw value of a driven long-wave input of the series: into the state mirror where the batch keeps one,
 * through (v / SIGMA)^0.25 - 273.15 (surface.rs:647,692) into the side's radiant temperature. The side's solar input is never
 * written here. A receiver without entries gets v = 0.0. Every emitter is read as it was at the START of the step: no
 * receiver sees a value this step has formed. Unlike the own-face term of heat_series this rule is exempt from nothing: the
 * host applying it between march calls reproduces every bit.
 * An input has ONE source: a receiver's long-wave channel in the series is -1 and it has no long-wave sky bit (an ir_own_face
 * bit on it is therefore refused by the series already). sum_irradiance (in/out, nullable) adds onto what the caller passes;
 * the rule has no other memory: a series of k steps followed by one of n - k with the returned array gives the bits of the
 * series of n. irradiance is nullable; an array that is not asked for costs no traffic and changes no bit of the others.
 * n_sub == 0 still evaluates every step. A NaN temperature or channel value propagates as a NaN channel value does. Weather
 * sites are supported (nothing here reads a site); sharded batches are refused as by the series.
 * heat_room_radiation_check (host-only; it also builds and verifies the tables the march uploads) and
 * heat_batch_march_series_radiation run the same checks before any device work; every message names "receiver r" or
 * "entry i": a negative count, a NULL array a positive count needs (sum_irradiance may be NULL; en_chan may be NULL when no
 * en_surface is -1), a side byte above 1, a factor that is not finite, en_chan other than -1 on an entry whose emitter is a
 * surface -> HEAT_E_INVALID_ARG; rc_surface outside [0, n_surfaces), en_surface outside [-1, n_surfaces), en_receiver
 * outside [0, n_receivers), a channel outside [0, n_channels) where the emitter is -1, the same (surface, side) twice among
 * the receivers, a receiver whose long-wave input has a channel or a sky bit already -> HEAT_E_SIZE.
 * heat_batch_march_series_radiation with radiation == NULL, or n_receivers == 0 and n_entries == 0, is
 * heat_batch_march_series_shaded exactly (same launches, same bits).
 */
typedef struct heat_room_radiation {
    int64_t n_receivers;
    const int64_t *rc_surface;        /* [n_receivers] */
    const uint8_t *rc_side;           /* [n_receivers] 0 front, 1 back */
    double *sum_irradiance;           /* [n_receivers] in/out, nullable */
    int64_t n_entries;
    const int64_t *en_receiver;       /* [n_entries] */
    const int64_t *en_surface;        /* [n_entries] the emitter's surface; -1: the entry is a channel */
    const uint8_t *en_side;           /* [n_entries] the emitter's side (not read where en_surface is -1) */
    const int32_t *en_chan;           /* [n_entries] nullable when no en_surface is -1; -1 where it is >= 0 */
    const double *en_factor;          /* [n_entries] */
} heat_room_radiation;

int heat_room_radiation_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky /* nullable */,
                              const heat_room_radiation *radiation); /* host-only */
int heat_batch_march_series_radiation(heat_batch *b, const heat_series *s, const heat_sky *sky /* nullable */,
                                      const heat_shades *shades /* nullable */, const heat_solar_gains *gains /* nullable */,
                                      const heat_zone_loads *l /* nullable */, heat_air_paths *air /* nullable */,
                                      heat_ideal_loads *il /* nullable */, heat_series_report *r /* nullable */, double *trace,
                                      double *applied, double *ideal_q, double *transmitted, double *path_q, double *sunlit,
                                      heat_room_radiation *radiation /* nullable */,
                                      double *irradiance /* [n_steps][n_receivers], nullable */, int32_t *failed_step);

/*
 * Ambient temperatures after creation: a side of kind HEAT_BOUNDARY_AMBIENT takes Boundary::AmbientTemperature
 * { temperature } from front_ambient / back_ambient of the descriptor; these two entry points change it afterwards — per call
 * (heat_batch_set_ambient) and per step of a series (heat_ambient_drive). What it is for: a floor slab or basement wall at
 * the month's ground temperature (HEAT_BOUNDARY_GROUND is refused, the reference panics there), a party wall to a neighbour
 * at a scheduled temperature, and an unheated neighbour space (attic, garage, stairwell) by the temperature-reduction
 * factor b of EN ISO 13789 / EN 12831, T_u = T_out + (1 - b) * (T_zone - T_out), which needs a zone temperature only the
 * device holds. The reference has no counterpart (its boundaries are fixed at construction); the rule below is this
 * library's own contract, defined against the per-call loop with the same rule on the host (heat_amd/ambient.py, apply()).
 *
 * heat_batch_set_ambient sets the temperature (degrees C) of the n listed sides — side[i] (0 front, 1 back) of surface
 * surface[i], the descriptor's numbering — from the next march on. The value is durable until set again: it survives
 * heat_batch_upload_state, heat_batch_upload_inputs, heat_batch_set_fusion, graph replay (use_graph) and a series. It is
 * ordered on the batch's stream behind earlier work; the caller's arrays are free when the call returns. Where the side is a
 * FRONT whose surface's BACK is Ambient as well, the back side's radiant temperature (t_front, surface.rs:672-686) follows.
 * Any double is accepted, a NaN included: it acts as a NaN in the descriptor's field would. Checks, all before any device
 * work, the message names "entry i": n < 0, a NULL array with n > 0, a side byte above 1 -> HEAT_E_INVALID_ARG; a surface
 * outside [0, n_surfaces), a side whose kind is not HEAT_BOUNDARY_AMBIENT, the same (surface, side) twice -> HEAT_E_SIZE.
 * n == 0 does nothing. A sharded batch (n_ranks > 1) is refused with HEAT_E_INVALID_ARG, as the series refuses one.
 *
 * heat_ambient_drive: driven side i is side[i] of surface[i], of kind HEAT_BOUNDARY_AMBIENT. Step k, behind the step's head
 * and before its sub-timesteps (nothing else in a step's preparation reads or writes these temperatures); T = the zone
 * temperatures the device holds when the step starts (what step k - 1 left), row = channel[k]; every line is ONE rounded f64
 * operation in the order written, no fused multiply-add:
 *   v = row[chan[i]]
 *   if gain:    v = gain[i] * v
 *   if offset:  v = v + offset[i]
 *   if mix_zone and mix_zone[i] >= 0:   d = T[mix_zone[i]] - v;   m = mix[i] * d;   v = v + m
 *   ambient temperature of (surface[i], side[i]) = v      (and the back side's t_front, as in the setter)
 *   ambient_t[k * n_sides + i] = v;   sum_temperature[i] = sum_temperature[i] + v
 * mix is 1 - b of EN ISO 13789 (b = 1: the outside channel alone; b = 0: the zone's temperature up to rounding). Every zone
 * temperature is read as it was at the START of the step, as air paths read it. A side not listed keeps what the descriptor,
 * the setter or an earlier series left; after the series the listed sides hold the values of step n_steps - 1, as the
 * per-call loop would leave them. Device state, trace, ambient_t and the sums are bit for bit what n_steps successive
 * heat_batch_march_ex calls give with heat_batch_set_ambient before call k, the values formed by the rule from the zone
 * temperatures downloaded before that call. sum_temperature (in/out, nullable) adds onto what the caller passes; the rule
 * has no other memory: a series of k steps followed by one of n - k with the returned array gives the bits of the series of
 * n. ambient_t is nullable; an array that is not asked for costs no traffic and changes no bit of the others. n_sub == 0
 * still sets every step's values. A NaN channel value propagates as a NaN in the descriptor's field would. Weather sites
 * need nothing; sharded batches are refused as by the series.
 * heat_ambient_check (host-only; it also builds and verifies the tables the march uploads) and
 * heat_batch_march_series_ambient run the same checks before any device work; every message names "ambient side i": a
 * negative count, a NULL array a positive count needs (gain, offset, mix_zone, sum_temperature may be NULL; mix may be NULL
 * when no mix_zone is >= 0), a side byte above 1, a gain, offset or (where mix_zone is >= 0) mix that is not finite ->
 * HEAT_E_INVALID_ARG; a surface outside [0, n_surfaces), a side that is not Ambient, a channel outside [0, n_channels), a
 * mix_zone outside [-1, n_zones), the same (surface, side) twice (an input has ONE source) -> HEAT_E_SIZE.
 * heat_batch_march_series_ambient with ambient == NULL, or n_sides == 0, is heat_batch_march_series_radiation exactly (same
 * launches, same bits).
 */
int heat_batch_set_ambient(heat_batch *b, int64_t n, const int64_t *surface /* [n] descriptor numbering */,
                           const uint8_t *side /* [n] 0 front, 1 back */, const double *temperature /* [n] C */);

typedef struct heat_ambient_drive {
    int64_t n_sides;
    const int64_t *surface;      /* [n_sides] */
    const uint8_t *side;         /* [n_sides] 0 front, 1 back; the side's kind is HEAT_BOUNDARY_AMBIENT */
    const int32_t *chan;         /* [n_sides] channel of the series, C */
    const double *gain, *offset; /* [n_sides], nullable = 1 / = 0 */
    const int32_t *mix_zone;     /* [n_sides], nullable / -1: none */
    const double *mix;           /* [n_sides], read only where mix_zone >= 0 (1 - b of EN ISO 13789) */
    double *sum_temperature;     /* [n_sides] in/out, nullable */
} heat_ambient_drive;

int heat_ambient_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_ambient_drive *a); /* host-only */
int heat_batch_march_series_ambient(heat_batch *b, const heat_series *s, const heat_sky *sky /* nullable */,
                                    const heat_shades *shades /* nullable */, const heat_solar_gains *gains /* nullable */,
                                    const heat_zone_loads *l /* nullable */, heat_air_paths *air /* nullable */,
                                    heat_ideal_loads *il /* nullable */, heat_series_report *r /* nullable */, double *trace,
                                    double *applied, double *ideal_q, double *transmitted, double *path_q, double *sunlit,
                                    heat_room_radiation *radiation /* nullable */, double *irradiance,
                                    heat_ambient_drive *ambient /* nullable */,
                                    double *ambient_t /* [n_steps][n_sides], nullable */, int32_t *failed_step);

/*
 * Blinds of a series: MOVABLE solar protection — a blind, roller shade or shutter that closes when the sun is on the window and
 * the room is warm, or that follows a position schedule. Nothing else that acts on the sun can move: an aperture's ap_scale and
 * a shade's diffuse_factor / ground_factor are constant over a series and the sunlit fraction is pure geometry. A blind cannot
 * be a channel (what an aperture transmits is formed on the device from the sky record) and, where it is controlled, not a
 * schedule either: the decision needs a zone temperature only the device holds, as a thermostat, an air path and a b-factor mix
 * do. The reference has no counterpart; the rule below is this library's own contract, defined against the per-call loop with
 * the same rule written on the host (heat_amd/blinds.py, incident_on() and apply()).
 * A BLIND i rides on shade j = shade[i] of the call's heat_shades (at most one blind per shade; a window without overhang or
 * fins uses a shade of zero depths). It turns the shade's three factors (f, diffuse_factor, ground_factor) into EFFECTIVE
 * factors (f', fd', fg'), and every consumer of that shade — sky-driven solar sides and apertures — reads those where it reads
 * (f, fd, fg) without blinds. A shade without a blind gets plain copies. sunlit[k][j] keeps the geometric f.
 * Step k, behind the shades and before the sky; r = the record of the shade's own site, f = the sunlit fraction the shades have
 * just stored for shade j, fd, fg = the shade's constant factors (1 where NULL), n = the shade's normal, T = the zone
 * temperatures the device holds when the step starts (as air paths and the ambient drive read them), row = channel[k]. Every
 * line is ONE rounded f64 operation in the order written, no fused multiply-add; max and min are those of heat_shades (the
 * FIRST operand where the comparison is false):
 *   c  = (n.x * r.sun_x + n.y * r.sun_y) + n.z * r.sun_z;   fs = 0.5 + 0.5 * n.z;   fg_ = 0.5 - 0.5 * n.z
 *   bm = c > 0 ? r.beam * c : 0.0;  bm = bm * f;  dv = (r.diffuse * fs) * fd;  gv = (r.ground * fg_) * fg
 *   I  = (bm + dv) + gv                       (W/m2: what an unblinded sky-driven side in the shade's plane receives)
 *   scheduled (pos_chan[i] >= 0):   p = row[pos_chan[i]];  p = max(p, 0.0);  p = min(p, 1.0)
 *                                             (a NaN position stays NaN and propagates; the state byte is left as it is)
 *   controlled (pos_chan NULL or -1):
 *       enabled = enable_chan[i] < 0 or row[enable_chan[i]] > 0
 *       d = band[i] / 2;  hi = set + d;  lo = set - d          (set = row[set_chan[i]]; only where zone[i] >= 0)
 *       hot  = zone[i] < 0 or T[zone[i]] > hi
 *       cool = zone[i] >= 0 and T[zone[i]] < lo
 *       if not enabled:                                   state = 0
 *       else if I > irr_close[i] and hot:                 state = 1
 *       else if state == 1 and (I < irr_open[i] or cool): state = 0
 *       p = state            (a NaN makes every comparison false: the state stays; a NaN enable value disables)
 *   q = 1.0 - p
 *   kb = q + p * beam_closed[i];   kd = q + p * diffuse_closed[i];   kg = q + p * ground_closed[i]      (two operations each)
 *   f' = f * kb;   fd' = fd * kd;   fg' = fg * kg
 *   position[k * n_blinds + i] = p;   blind_incident[k * n_blinds + i] = I;   sum_position[i] = sum_position[i] + p
 *   steps_closed[i] += (p > 0);   switches[i] += (state after != before)
 * With p == 0 every factor is multiplied by exactly 1.0: an open blind gives the bits of the call without blinds. With p == 1
 * the factors are exactly f * beam_closed and so on. Between irr_open and irr_close, and inside the band, a blind keeps its
 * state (hysteresis). A scheduled blind never switches. position, blind_incident, state and the accumulators are in the
 * caller's blind order. State and the accumulators carry a cut: a series of k steps followed by one of n - k with the
 * returned arrays gives the bits of the series of n; state == NULL: every controlled blind starts open and the states are not
 * returned. n_sub == 0 still evaluates the blinds of every step. A blind reads the record of ITS SHADE's site: weather sites
 * are supported. Sharded batches are refused, as by the series.
 * Out of scope: a blind that redirects beam into diffuse radiation (venetian slats), and a blind's effect on the window's
 * long-wave exchange or convection — the blind acts on the three solar factors alone.
 * heat_blinds_check (host-only; it also builds and verifies the table the march uploads) and heat_batch_march_series_blinds
 * run the same checks before any device work; every message names "blind i": a negative count, a NULL array a positive count
 * needs (pos_chan, zone, enable_chan, state and the accumulators may be NULL; irr_close and irr_open may be NULL when every
 * blind is scheduled; set_chan and band when no zone is >= 0), n_blinds > 0 without shades, a closed factor that is not finite
 * or negative, irr_open > irr_close or either not finite on a controlled blind, a band that is negative or not finite where
 * zone >= 0, a state byte above 1 -> HEAT_E_INVALID_ARG; a shade outside [0, n_shades), a shade named twice, a zone outside
 * [-1, n_zones), set_chan outside [0, n_channels) where zone >= 0, pos_chan or enable_chan outside [-1, n_channels) ->
 * HEAT_E_SIZE.
 * heat_batch_march_series_blinds with blinds == NULL or n_blinds == 0 is heat_batch_march_series_ambient exactly (same
 * launches, same bits); position and blind_incident are nullable, and an array that is not asked for costs no traffic and
 * changes no bit of the others.
 */
typedef struct heat_blinds {
    int64_t n_blinds;
    const int32_t *shade;          /* [n_blinds] the shade the blind rides on */
    const double *beam_closed, *diffuse_closed, *ground_closed;   /* [n_blinds] factors of the fully closed blind, finite, >= 0 */
    const int32_t *pos_chan;       /* [n_blinds] nullable / -1: controlled; else SCHEDULED: the position is a channel */
    const double *irr_close, *irr_open;   /* [n_blinds] W/m2 on the shade's plane, irr_open <= irr_close; read only where controlled */
    const int32_t *zone;           /* [n_blinds] nullable / -1: no room condition; else the zone whose temperature gates the blind */
    const int32_t *set_chan;       /* [n_blinds] the zone's setpoint channel, C; read only where zone >= 0 */
    const double *band;            /* [n_blinds] K, >= 0; read only where zone >= 0 */
    const int32_t *enable_chan;    /* [n_blinds] nullable / -1: always enabled; else enabled where row[chan] > 0 */
    uint8_t *state;                /* [n_blinds] in/out, nullable (= all open): 0 open, 1 closed; controlled blinds only */
    int64_t *steps_closed;         /* [n_blinds] in/out, nullable */
    int64_t *switches;             /* [n_blinds] in/out, nullable */
    double *sum_position;          /* [n_blinds] in/out, nullable */
} heat_blinds;

int heat_blinds_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky,
                      const heat_solar_gains *gains, const heat_shades *shades, const heat_blinds *blinds); /* host-only */
int heat_batch_march_series_blinds(heat_batch *b, const heat_series *s, const heat_sky *sky /* nullable */,
                                   const heat_shades *shades /* nullable */, const heat_solar_gains *gains /* nullable */,
                                   const heat_zone_loads *l /* nullable */, heat_air_paths *air /* nullable */,
                                   heat_ideal_loads *il /* nullable */, heat_series_report *r /* nullable */, double *trace,
                                   double *applied, double *ideal_q, double *transmitted, double *path_q, double *sunlit,
                                   heat_room_radiation *radiation /* nullable */, double *irradiance,
                                   heat_ambient_drive *ambient /* nullable */, double *ambient_t,
                                   heat_blinds *blinds /* nullable */, double *position /* [n_steps][n_blinds], nullable */,
                                   double *blind_incident /* [n_steps][n_blinds], nullable */, int32_t *failed_step);

/*
 * Anisotropic sky of a series: every solar term above takes the sky's diffuse radiation as isotropic, diffuse * (0.5 + 0.5 * n.z)
 * on every plane. Hay-Davies, Reindl and Perez share one form,
 *   D_tilt = D * [ (1 - F1) * sky_view + F1 * cos(incidence) / max(cos 85 deg, cos(zenith)) + F2 * band(plane) ],
 * with F1 the circumsolar fraction and F2 the horizon coefficient, functions of site and step alone (clearness, brightness and
 * zenith: transcendental work of the caller, as the sun's direction is), and band a function of the plane alone. The caller
 * passes ONE PAIR (circ, horiz) = (F1, F2) per site and step beside the record, and one band per consumer; the device does a
 * handful of multiplications and one division. The circumsolar part comes from the sun's direction: it is shaded by the sunlit
 * fraction, passes a window with the beam transmittance at the sun's incidence, lands through en_beam and counts in the
 * irradiance a blind decides on — which is why it cannot be pre-mixed into `diffuse`. The reference has no counterpart; the rule
 * below is this library's own contract, defined against the per-call loop with the same rule written on the host
 * (heat_amd/sky.py incident(), solar_gains.py transmitted(), blinds.py incident_on(), each with aniso=).
 * q = coef[k * n_sites + site], the site being the one whose record the consumer reads; Z0 = 0.08715574274765817 (cos 85 deg:
 * the literal is the contract); c, fs, fg, t, ib, scale, f, fd, fgr as the consumer has them above. Every line is ONE rounded
 * f64 operation in the order written, no fused multiply-add; a NaN makes every comparison false:
 *   up  = r.sun_z > 0.0
 *   zb  = r.sun_z > Z0 ? r.sun_z : Z0
 *   rb  = (c > 0 and up) ? c / zb : 0.0
 *   iso = 1.0 - q.circ
 * A sky-driven solar side (mode bit 0 / 1), band = front_band[s] / back_band[s]:
 *   bm = c > 0 ? r.beam * c : 0.0
 *   cs = (r.diffuse * q.circ) * rb;      sun = bm + cs
 *   dv = (r.diffuse * fs) * iso;         hv = (r.diffuse * q.horiz) * band;    dv = dv + hv
 *   gv = r.ground * fg
 *   with a shade j (the effective factors where blinds act):  sun = sun * f;  dv = dv * fd;  gv = gv * fgr
 *   v  = (sun + dv) + gv                 (then the gain, the mirror, the clamp, the absorptance: unchanged)
 * An aperture, band = aperture_band[a]:
 *   pbm = (ib * t) * scale
 *   ics = (r.diffuse * q.circ) * rb;     pcs = (ics * t) * scale;              ps = pbm + pcs
 *   with a shade:  ps = ps * f
 *   Pb  = c > 0 ? ps : 0.0
 *   dd  = (r.diffuse * fs) * iso;        hv = (r.diffuse * q.horiz) * band;    dd = dd + hv
 *   gg  = r.ground * fg
 *   with a shade:  dd = dd * fd;  gg = gg * fgr
 *   id  = dd + gg;   Pd = (id * tau_diffuse) * scale;   P = Pb + Pd            (transmitted, ap_sum, the entries: unchanged)
 * A blind's I is the rule of a shaded side with the shade's normal, the shade's own geometric f and constant fd, fg (as
 * heat_blinds has them), band = shade_band[j] and q of the shade's own site.
 * Long-wave inputs, channel-driven inputs and everything behind the raw value are untouched. With q.circ == 0 and q.horiz == 0
 * every consumer gives the bits of the isotropic rule (the sign of a zero aside), shaded or not. The rule has no memory: a
 * series of k steps followed by one of n - k gives the bits of the series of n; n_sub == 0 still sets every input. Weather
 * sites are supported; sharded batches are refused, as by the series.
 * heat_sky_aniso_check (host-only) and heat_batch_march_series_call run the same checks before any device work: aniso without
 * sky or without sky->record, coef NULL with n_steps > 0, aperture_band without gains, shade_band without shades, a band that
 * is negative or not finite on a consumer that reads it — "surface s" where the side's solar mode bit is set, every "aperture
 * a", every "shade j" -> HEAT_E_INVALID_ARG. The coefficients are not checked: they are the caller's, as the transmittance
 * polynomial is, and a NaN propagates as a NaN record field does.
 */
typedef struct heat_sky_coef { double circ, horiz; } heat_sky_coef;   /* F1, F2 of one site at one step; 16 bytes */

typedef struct heat_sky_aniso {
    const heat_sky_coef *coef;                 /* [n_steps][n_sites]: [k * n_sites + site] */
    const double *front_band, *back_band;      /* [n_surfaces], nullable = 0: band of the front / back solar input */
    const double *aperture_band;               /* [gains->n_apertures], nullable = 0 */
    const double *shade_band;                  /* [shades->n_shades], nullable = 0: read by blinds for I */
} heat_sky_aniso;

/*
 * One call for every term of a series: heat_batch_march_series_call takes what heat_batch_march_series_blinds takes, by name,
 * plus aniso. Zero-initialise the struct, set size = sizeof(heat_series_call) and fill the fields the call has; every pointer
 * but s may be NULL, and a NULL trace records none. call or call->s NULL, or a size that is not this library's
 * sizeof(heat_series_call) -> HEAT_E_INVALID_ARG. With aniso == NULL it is heat_batch_march_series_blinds on the same arguments
 * exactly: same launches, same bits. A refused call leaves the device state untouched.
 */
typedef struct heat_series_call {
    size_t size;                               /* sizeof(heat_series_call) as the caller compiled it */
    const heat_series *s;
    const heat_sky *sky;
    const heat_sky_aniso *aniso;
    const heat_shades *shades;
    const heat_solar_gains *gains;
    const heat_zone_loads *l;
    heat_air_paths *air;
    heat_ideal_loads *il;
    heat_series_report *r;
    heat_room_radiation *radiation;
    heat_ambient_drive *ambient;
    heat_blinds *blinds;
    double *trace, *applied, *ideal_q, *transmitted, *path_q, *sunlit, *irradiance, *ambient_t, *position, *blind_incident;
    int32_t *failed_step;
} heat_series_call;

int heat_sky_aniso_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky,
                         const heat_solar_gains *gains, const heat_shades *shades, const heat_sky_aniso *aniso); /* host-only */
int heat_batch_march_series_call(heat_batch *b, const heat_series_call *call);

/*
 * Comfort of a series: the operative temperature of rooms, reported per step, accumulated against limits that are channels,
 * and — where a sensor says so — sensed by the controls in place of the zone's air temperature. A sensor stands in a zone and
 * sees a list of faces: entry j gives sensor en_sensor[j] the first (en_side 0) or last (en_side 1) node of surface
 * en_surface[j] with weight en_weight[j]; the weighted sum is the mean radiant temperature, mixed with the zone's air by
 * air_weight. The faces are temperatures only the device holds at the start of a step: neither the rows nor the controls'
 * reaction can be formed by the caller ahead of time. The reference has no comfort model; the rule below is this library's
 * own contract, defined against the per-call loop with the same rule written on the host (heat_amd/comfort.py operative(),
 * control_temperatures(), accumulate()).
 * The rule of step k, evaluated behind the step's head and before the zone loads: T the node temperatures and Tz the zone
 * temperatures the device holds at that moment — what step k - 1 left; nothing on the head writes either —, row = channel[k],
 * K = step_base + k. Every line is ONE rounded f64 operation in the order written, no fused multiply-add; a NaN makes every
 * comparison false:
 *   per sensor i:
 *     r = 0.0;  per entry j of i, in the caller's order:  x = en_weight[j] * T[face(en_surface[j], en_side[j])];  r = r + x
 *     a = air_weight[i];  xa = a * Tz[zone[i]];  b = 1.0 - a;  xr = b * r;  top = xa + xr
 *     mrt[k][i] = r;  operative[k][i] = top
 *     occ = occ_chan[i] < 0 or row[occ_chan[i]] > 0
 *     if occ:  n_occupied += 1;  sum_operative = sum_operative + top
 *              if top < min_operative { min_operative = top; step_min = K }      (strict: the first occurrence stays)
 *              if top > max_operative { max_operative = top; step_max = K }
 *              if lo_chan[i] >= 0 and top < row[lo]:  n_below += 1;  d = row[lo] - top;  deg_below = deg_below + d
 *              if hi_chan[i] >= 0 and top > row[hi]:  n_above += 1;  d = top - row[hi];  deg_above = deg_above + d
 *                                                     if d > max_above { max_above = d; step_max_above = K }
 *   the control temperature of the step:  Tc[z] = top of the sensor with control == 1 and zone == z, else Tz[z]
 * Who reads Tc: the thermostats of heat_zone_loads (Ts = Tc[sensor]); the air paths for e = s * (Tc[target] - set) alone — Tt
 * in g, dT and q stays the air temperature: the air that moves is air —; the blinds for their room condition (Tc[zone]).
 * The ideal loads and the ambient drive's mix keep the air temperature: they act on, or stand for, the zone's air.
 * A sensor without entries has r = 0.0. Row k describes the state at the START of step k, as path_q and irradiance do.
 * n_sub == 0 still evaluates every step, on the unchanged state. Every accumulator is in/out and nullable; resume == 0: the
 * library initialises on the device (sums and counts 0, min = +inf, max = -inf, max_above = -inf, steps = -1); resume != 0:
 * they start from the caller's arrays. The term has no other memory: a series of k steps followed by one of n - k with
 * resume = 1 and step_base + k gives the bits of the series of n.
 * heat_comfort_check (host-only) and heat_batch_march_series_comfort run the same checks before any device work; every
 * message names "comfort sensor i" or "comfort entry j". HEAT_E_INVALID_ARG: a negative count; a NULL array that a positive
 * count needs (zone; en_sensor, en_surface, en_side, en_weight); an en_weight or air_weight that is not finite; an air_weight
 * outside [0, 1]; a control byte above 1; a step array without its extremum (step_min / step_max / step_max_above without
 * min_operative / max_operative / max_above). HEAT_E_SIZE: a zone, surface, sensor or channel out of range; a side above 1; a
 * second control sensor on a zone. Sharded batches are refused, as by the series. A refused call leaves the device state
 * untouched.
 * With c == NULL or n_sensors == 0 heat_batch_march_series_comfort is heat_batch_march_series_call on `call` exactly: same
 * launches, same bits. Sensors without a control bit change no bit of any other output.
 */
typedef struct heat_comfort {
    int64_t n_sensors;
    const int32_t *zone;          /* [n_sensors] the zone whose air the sensor stands in */
    const double  *air_weight;    /* [n_sensors] nullable = 0.5; finite, in [0, 1] */
    const uint8_t *control;       /* [n_sensors] nullable = 0; 1: this sensor is the control temperature of its zone */
    int64_t n_entries;
    const int32_t *en_sensor;     /* entries in any order; summed per sensor in the caller's order */
    const int64_t *en_surface;
    const uint8_t *en_side;       /* 0: first node, 1: last node of the surface */
    const double  *en_weight;     /* finite; the caller makes them sum to 1 per sensor (comfort.by_area does) */
    const int32_t *occ_chan, *lo_chan, *hi_chan;   /* [n_sensors] each nullable / -1: always occupied / no limit */
    int32_t resume;               /* as heat_series_report::resume, for the arrays below */
    int64_t step_base;            /* K = step_base + k is what the step arrays record */
    /* accumulators, [n_sensors] each, in/out, nullable */
    int64_t *n_occupied;
    double *sum_operative;
    double *min_operative;
    int64_t *step_min;
    double *max_operative;
    int64_t *step_max;
    int64_t *n_below;
    double *deg_below;
    int64_t *n_above;
    double *deg_above;
    double *max_above;
    int64_t *step_max_above;
} heat_comfort;

int heat_comfort_check(const heat_batch_desc *desc, const heat_series *s, const heat_comfort *c); /* host-only */
int heat_batch_march_series_comfort(heat_batch *b, const heat_series_call *call, heat_comfort *c /* nullable */,
                                    double *operative /* [n_steps][n_sensors], nullable */,
                                    double *mrt /* [n_steps][n_sensors], nullable */);

/*
 * Air handlers of a series: mechanical ventilation with HEAT RECOVERY — a unit that extracts air from zones, passes it through
 * an exchanger against the outdoor air it takes in, and supplies that air to zones, past a summer bypass and a supply-air coil.
 * A flow of heat_zone_loads and a supply path of heat_air_paths (source == -1) take their inlet temperature from a channel; a
 * recovery unit supplies at T_out + eta * (T_extract - T_out), and T_extract is the flow-weighted mix of zone temperatures only
 * the device holds when the step starts. The bypass and the coil's power depend on the same temperatures: none of it can be a
 * schedule. The reference has no counterpart (heating_cooling.rs is a todo!(), model.rs:522-544 knows scheduled flows only);
 * the rule below is this library's own contract, defined against the per-call loop with the same rule written on the host
 * (heat_amd/air_handlers.py, apply()). The air properties are the reference's (gas.rs:49,165-179), written exactly as the
 * zone loads and the air paths write them.
 * A UNIT u has an outdoor-air temperature channel, a recovery effectiveness (a constant gain times an optional channel), an
 * optional bypass controller with hysteresis, an optional heating coil (a minimum supply temperature channel and a capacity in
 * W) and an optional cooling coil (a maximum supply temperature channel and a capacity in W). A BRANCH j joins a unit to a
 * zone: a volume channel times a gain, m3/s, and a kind byte — it supplies (bit 0), extracts (bit 1) or both (3).
 * The rule of step k, behind the air paths and before the ambient drive — a zone's sum is ((row + loads) + paths) + branches.
 * T = the zone AIR temperatures the device holds then (what step k - 1 left; no control temperature: a unit senses air),
 * row = channel[k]. Every line is ONE rounded f64 operation in the order written, no fused multiply-add; a NaN makes every
 * comparison false:
 *   per unit u:
 *     To = row[outdoor_chan]
 *     st = 0.0;  sv = 0.0
 *     per EXTRACT branch j of u, in the caller's order:
 *         V = br_volume_gain[j] * row[br_volume_chan[j]];  x = V * T[br_zone[j]];  st = st + x;  sv = sv + V
 *     Te = sv > 0.0 ? st / sv : To                      (no extraction: nothing to recover from)
 *     eta = eff_gain[u]
 *     eff_chan >= 0:  eta = eta * row[eff_chan]
 *     if eta < 0.0: eta = 0.0
 *     if eta > 1.0: eta = 1.0
 *     bypass (bypass_chan >= 0):
 *         set = row[bypass_chan];  d = bypass_band / 2;  e = Te - set;  g = Te - To
 *         if      e > d and g > bypass_min_delta             state = 1
 *         else if state == 1 and (e < -d or g <= 0.0)        state = 0
 *         state == 1: eta = 0.0
 *     dT = Te - To;  r = eta * dT;  Tr = To + r         (behind the exchanger; the fan stands here)
 *     Tk = Tr + 273.15;  rho = 101325 * 28.97 / (8314.46261815324 * Tk);  cp = 1002.7370 + 1.2324e-2 * Tk
 *     M = 0.0
 *     per SUPPLY branch j of u, in the caller's order:
 *         V = gain * row[chan];  m[j] = (rho * V) * cp;  M = M + m[j]
 *     recovered = M * r                                 (W, positive when the exchanger warms the supply)
 *     Ts = Tr;  q = 0.0
 *     if heat_chan >= 0 and Tr < row[heat_chan]:
 *         lift = row[heat_chan] - Tr;  need = M * lift
 *         if need <= heat_cap:  Ts = row[heat_chan];  q = need
 *         else:                 q = heat_cap;  x = heat_cap / M;  Ts = Tr + x;  heat-saturated
 *     else if cool_chan >= 0 and Tr > row[cool_chan]:
 *         drop = Tr - row[cool_chan];  need = M * drop
 *         if need <= cool_cap:  Ts = row[cool_chan];  q = 0.0 - need
 *         else:                 q = 0.0 - cool_cap;  x = cool_cap / M;  Ts = Tr - x;  cool-saturated
 *     supply_t[k][u] = Ts;  recovered[k][u] = recovered;  coil_q[k][u] = q
 *     sum_recovered += recovered;  sum_heating += q where q > 0;  sum_cooling += q where q < 0
 *     steps_bypass += state;  switches += (state after != before);  steps_*_saturated += 1 where saturated
 *   per zone z, its SUPPLY branches in the caller's order:
 *     mt = m[j] * Ts[unit];  a0[z] = a0[z] + mt;  b0[z] = b0[z] + m[j]
 *     dz = Ts[unit] - T[z];  bq = m[j] * dz
 *     branch_q[k][j] = bq;  sum_branch_q[j] = sum_branch_q[j] + bq
 * An extract-only branch adds nothing to its zone — only inflows appear in the balance — and its branch_q is 0.0. Every T is
 * the start of the step's value, whatever the order of units and zones. The terms hold for all n_sub sub-timesteps of the
 * step: ideal loads see them. n_sub == 0 still evaluates every step. bypass and every accumulator carry a cut: a series of k
 * steps followed by one of n - k with the returned arrays gives the bits of the series of n. bypass == NULL: every unit starts
 * recovering and nothing is returned. A unit without a bypass controller recovers whatever its byte says and leaves the byte
 * as it is (steps_bypass still adds the byte: pass 0). A supply branch that turns a clean a0 or b0 into NaN is HEAT_N_NAN_ZONE for that zone at that step, as for the
 * air paths; a NaN in a unit without supply branches reaches its rows only. An array that is not asked for costs no traffic
 * and changes no bit of the others. With h == NULL or n_units == 0 heat_batch_march_series_handlers is
 * heat_batch_march_series_comfort exactly: same launches, same bits. A refused call leaves the device state untouched. Sharded
 * batches are refused as by the series; weather sites need nothing.
 * heat_air_handlers_check (host-only; it also builds and verifies the tables the march uploads) and
 * heat_batch_march_series_handlers run the same checks before any device work; every message names "air handler u" or "air
 * handler branch j". HEAT_E_INVALID_ARG: a negative count; a NULL array that a positive count needs (outdoor_chan; br_unit,
 * br_zone, br_volume_chan); NULL bypass_band or bypass_min_delta where some unit bypasses; an eff_gain, br_volume_gain, band or
 * min_delta that is not finite; a negative band or min_delta; a negative or NaN capacity; a br_kind outside 1..3; a bypass
 * byte above 1; branches with n_units == 0. HEAT_E_SIZE: a unit, zone or channel out of range (eff_chan, bypass_chan,
 * heat_chan and cool_chan may be -1).
 * Out of scope: frost protection of the exchanger, fan heat, latent recovery, variable-volume control by a zone, and a unit
 * whose mass flow follows the coil outlet (every m[j] is taken at the exchanger's outlet, Tr).
 */
typedef struct heat_air_handlers {
    int64_t n_units;
    const int32_t *outdoor_chan;        /* [n_units] outdoor-air temperature, C */
    const int32_t *eff_chan;            /* nullable / -1: eta = eff_gain */
    const double  *eff_gain;            /* nullable = 1 */
    const int32_t *bypass_chan;         /* nullable / -1: no bypass; else the setpoint of the extract air, C */
    const double  *bypass_band, *bypass_min_delta;   /* K >= 0; read only where bypass_chan >= 0 */
    const int32_t *heat_chan, *cool_chan;            /* nullable / -1: no coil; minimum / maximum supply temperature, C */
    const double  *heat_cap, *cool_cap;              /* W >= 0, +inf allowed; nullable = +inf */
    int64_t n_branches;
    const int32_t *br_unit, *br_zone, *br_volume_chan;
    const double  *br_volume_gain;      /* nullable = 1 */
    const uint8_t *br_kind;             /* nullable = 3; 1 supplies, 2 extracts, 3 both */
    uint8_t *bypass;                    /* [n_units] in/out, nullable (= all recovering): 0 / 1 */
    double  *sum_recovered, *sum_heating, *sum_cooling;            /* [n_units] in/out, nullable */
    int64_t *steps_bypass, *switches, *steps_heat_saturated, *steps_cool_saturated;
    double  *sum_branch_q;              /* [n_branches] in/out, nullable */
} heat_air_handlers;

int heat_air_handlers_check(const heat_batch_desc *desc, const heat_series *s, const heat_air_handlers *h); /* host-only */
int heat_batch_march_series_handlers(heat_batch *b, const heat_series_call *call, heat_comfort *c /* nullable */,
                                     double *operative, double *mrt, heat_air_handlers *h /* nullable */,
                                     double *supply_t  /* [n_steps][n_units], nullable */,
                                     double *recovered /* [n_steps][n_units], nullable */,
                                     double *coil_q    /* [n_steps][n_units], nullable */,
                                     double *branch_q  /* [n_steps][n_branches], nullable */);

/*
 * Air species of a series: what rides on the air a series moves — CO2, moisture, any pollutant — as one well-mixed
 * concentration per species and zone, held on the device over the steps, and DEMAND VENTS whose volume flow follows such a
 * concentration. Every flow of air of a series enters the balance: the zone loads' flows, the air paths that are open in the
 * step, the handlers' supply branches and the vents themselves. A concentration depends on which controlled paths are open
 * — a state the device decides from temperatures only it holds — and a vent's flow enters the zones' a0 / b0: none of it can
 * be a schedule. The reference has no counterpart (zone.rs, model.rs:500-597); the rule below is this library's own contract,
 * defined against the per-call loop with the same rule written on the host (heat_amd/air_species.py, apply()). The unit of a
 * concentration is the caller's (amount per m3 of air); a source is amount per second.
 * The rule of step k, behind the air handlers and before the ambient drive — a zone's sum is
 * (((row + loads) + paths) + branches) + vents. T = the zone AIR temperatures, C = the concentrations the device holds when
 * the step starts, row = channel[k], K = step_base + k. Every line is ONE rounded f64 operation in the order written, no fused
 * multiply-add; a NaN makes every comparison false:
 *   per vent j (zone z, species s); a zone's vents in the caller's order:
 *     c = C[s][z];  x = c - c_lo;  span = c_hi - c_lo;  f = x / span
 *     if f < 0.0: f = 0.0
 *     if f > 1.0: f = 1.0
 *     saturated = (f == 1.0)
 *     dv = v_max - v_min;  y = f * dv;  V = v_min + y
 *     disabled (enable_chan >= 0 and not row[enable_chan] > 0):  V = 0.0, q = 0.0, nothing is added to a0 / b0, not saturated
 *     else: Tin = row[temp_chan];  Tk = Tin + 273.15;  rho = 101325 * 28.97 / (8314.46261815324 * Tk)
 *           cp = 1002.7370 + 1.2324e-2 * Tk;  m = (rho * V) * cp       (exactly the zone loads' expressions and grouping)
 *           mt = m * Tin;  a0[z] = a0[z] + mt;  b0[z] = b0[z] + m;  dT = Tin - T[z];  q = m * dT
 *     vent_v[k][j] = V;  vent_q[k][j] = q;  sum_volume += V;  sum_q += q;  steps_saturated += saturated
 *   per species s and zone z:
 *     h = (double)n_sub * dt;  c = C[s][z];  co = outdoor_chan[s][z] >= 0 ? row[outdoor_chan[s][z]] : 0.0
 *     S = 0.0;  per source of (s, z), in the caller's order:  x = src_factor * row[src_chan];  S = S + x
 *     F = 0.0;  G = 0.0;  per inflow into z:  g = V * ci;  F = F + V;  G = G + g,  in this order:
 *       the zone loads' flows of z, caller's order:     V = flow_volume_gain * row[flow_volume_chan];  ci = co
 *       the air paths with target z that are OPEN in step k (uncontrolled, or state == 1 after this step's decision),
 *           caller's order:                             V = volume_gain * row[volume_chan];  ci = source >= 0 ? C[s][source] : co
 *       the handlers' SUPPLY branches of z, caller's order:  V = br_volume_gain * row[br_volume_chan];  ci = co
 *       the vents of z (of whatever species), caller's order:  V as above (0.0 where disabled);  ci = co
 *     p = S + G;  hp = h * p;  vc = vol[z] * c;  num = vc + hp;  hF = h * F;  den = vol[z] + hF;  c_new = num / den
 *     conc_rows[k][s][z] = c                            (the state at the START of step k, as every other row)
 *     occupied (occ_chan[z] < 0 or row[occ_chan[z]] > 0):
 *         n_occupied += 1;  sum_conc = sum_conc + c;  if c > max_conc { max_conc = c; step_max = K }
 *         if limit_chan[s] >= 0 and c > row[limit]:  n_above += 1;  d = c - row[limit];  excess_above = excess_above + d
 *     C[s][z] = c_new                                   (after every lane of the step has read its sources)
 * A backward-Euler step of vol dc/dt = S + sum V (ci - c): only inflows appear, as in the heat balance, and neighbours are
 * taken as they were at the START of the step — a chain A -> B -> C does not propagate within a step. Unconditionally stable
 * for V >= 0. A gain of 1 is multiplied like any other (x * 1.0 is x). The vents' terms hold for all n_sub sub-timesteps: ideal
 * loads see them. n_sub == 0 still evaluates every step, with h = 0. conc, the accumulators and the air paths' state carry a
 * cut: a series of k steps followed by one of n - k with the returned arrays and step_base + k gives the bits of the series of
 * n. resume == 0 initialises every accumulator on the device, the vents' three included (sums and counts 0, max_conc = -inf,
 * step_max = -1); conc is always read. A vent that turns a clean a0 / b0 into NaN is
 * HEAT_N_NAN_ZONE for its zone at that step, as for the air paths; a NaN concentration that reaches no vent is no failure and
 * stays in its rows. An array that is not asked for costs no traffic and changes no bit of the others. With sp == NULL or
 * n_species == 0 heat_batch_march_series_species is heat_batch_march_series_handlers exactly: same launches, same bits. A
 * refused call leaves the device state untouched. Sharded batches are refused as by the series.
 * heat_air_species_check (host-only; it checks l, air and h as their own checks do, and builds and verifies the tables the
 * march uploads) and heat_batch_march_series_species run the same checks before any device work; every message names "air
 * species s", "species source i" or "demand vent j". HEAT_E_INVALID_ARG: a negative count; a NULL array that a positive count
 * needs (outdoor_chan, conc; src_zone, src_species, src_chan; vent_zone, vent_species, vent_temp_chan, vent_v_min, vent_v_max,
 * vent_c_lo, vent_c_hi); sources or vents with n_species == 0; a src_factor, v_min, v_max, c_lo or c_hi that is not finite;
 * v_min < 0, v_max < v_min or c_hi <= c_lo. A conc entry that is not finite is data and is accepted. HEAT_E_SIZE: a zone,
 * species or channel out of range (outdoor_chan, vent_enable_chan, limit_chan and occ_chan may be -1).
 * Out of scope: density differences between inflow and zone air (a volume flow carries its concentration as it is);
 * recirculating units (a handler supplies outside air); sorption in materials; latent heat; deposition and filters, except as
 * a negative source.
 */
typedef struct heat_air_species {
    int64_t n_species;
    const int32_t *outdoor_chan;        /* [n_species][n_zones] the concentration of OUTSIDE air entering zone z; -1: 0.0 */
    int64_t n_sources;
    const int32_t *src_zone, *src_species, *src_chan;
    const double  *src_factor;          /* nullable = 1; amount per second = factor * row[chan], negative allowed */
    int64_t n_vents;
    const int32_t *vent_zone, *vent_species;
    const int32_t *vent_temp_chan;      /* outdoor-air temperature, C */
    const int32_t *vent_enable_chan;    /* nullable / -1: always enabled; else enabled where row[chan] > 0 */
    const double  *vent_v_min, *vent_v_max;          /* m3/s, finite, 0 <= min <= max */
    const double  *vent_c_lo, *vent_c_hi;            /* finite, lo < hi */
    const int32_t *limit_chan;          /* [n_species] nullable / -1: no limit */
    const int32_t *occ_chan;            /* [n_zones] nullable / -1: always occupied; else occupied where row[chan] > 0 */
    int64_t resume;                     /* as heat_comfort::resume, for the nine accumulators below */
    int64_t step_base;                  /* K = step_base + k is what step_max records */
    double  *conc;                      /* [n_species][n_zones] in/out, required when n_species > 0 */
    /* accumulators, [n_species][n_zones] each, in/out, nullable */
    int64_t *n_occupied;
    double  *sum_conc;
    double  *max_conc;
    int64_t *step_max;                  /* kept where max_conc is: it records the step of that maximum */
    int64_t *n_above;
    double  *excess_above;
    /* per vent, [n_vents] each, in/out, nullable */
    double  *sum_volume;
    double  *sum_q;
    int64_t *steps_saturated;
} heat_air_species;

int heat_air_species_check(const heat_batch_desc *desc, const heat_series *s, const heat_zone_loads *l /* nullable */,
                           const heat_air_paths *air /* nullable */, const heat_air_handlers *h /* nullable */,
                           const heat_air_species *sp /* nullable */); /* host-only */
int heat_batch_march_series_species(heat_batch *b, const heat_series_call *call, heat_comfort *c /* nullable */,
                                    double *operative, double *mrt, heat_air_handlers *h /* nullable */,
                                    double *supply_t, double *recovered, double *coil_q, double *branch_q,
                                    heat_air_species *sp /* nullable */,
                                    double *conc_rows /* [n_steps][n_species][n_zones], nullable */,
                                    double *vent_v    /* [n_steps][n_vents], nullable */,
                                    double *vent_q    /* [n_steps][n_vents], nullable */);

/*
 * Openings of a series: the volume flow that wind and buoyancy drive through an open window, a doorway or a vent, as a
 * DERIVED CHANNEL. Every flow of air of a series takes its volume from a channel, and a channel is a schedule; the flow
 * through an opening depends on |Ta - Tb| between two zones, or a zone and outside, at the start of the step — temperatures
 * only the device holds. An opening therefore WRITES its volume flow into one column of the step's row in the device's copy
 * of the channel table, and every consumer reads that column as it reads any channel, through its volume channel: the air
 * paths (volume_gain * row[volume_chan]), the zone loads' flows (wind- and stack-driven infiltration), the handlers' branches
 * and, through the same tables, the species. No struct and no kernel of those terms changes. The reference has no
 * counterpart (model.rs:546,592-593 take infiltration and mixing volumes as given numbers); the rule below is this library's
 * own contract, defined against the per-call loop with the same rule written on the host (heat_amd/openings.py, apply()).
 * Each opening is an explicit formula, the superposition form of EnergyPlus' wind-and-stack open area and of de Gids-Phaff.
 * The rule of step k. The openings are the first kernel of the step behind the controllers (heat_controllers, below: an
 * open fraction may be a controller's output), ahead of the comfort term: nothing else of the step has read the row yet. T = the zone AIR temperatures the device holds when the step starts, row = the device's channel[k],
 * K = step_base + k. Every line is ONE rounded f64 operation in the order written, no fused multiply-add; a NaN makes every
 * comparison false:
 *   per opening i:
 *     Ta = T[zone_a];  Tb = zone_b >= 0 ? T[zone_b] : row[temp_chan]
 *     d = Ta - Tb;  ad = |d|            (sign bit cleared)
 *     sm = Ta + Tb;  tm = sm * 0.5;  tk = tm + 273.15
 *     r = ad / tk;  st = cs * r;  sa = ca * ad
 *     u = wind_chan >= 0 ? row[wind_chan] : 0.0;  u2 = u * u;  w = cw * u2
 *     x = w + st;  x2 = x + sa;  y = x2 + c0
 *     if y < 0.0: y = 0.0
 *     U = sqrt(y)                        (correctly rounded)
 *     f = frac_chan >= 0 ? row[frac_chan] : 1.0;  if f < 0.0: f = 0.0;  if f > 1.0: f = 1.0
 *     af = area * f;  V = af * U
 *     row[out_chan] = V;  opening_v[k][i] = V;  sum_v = sum_v + V;  if V > max_v { max_v = V; step_max = K }
 * V is symmetric in a and b (both |Ta - Tb| and Ta + Tb are): a doorway is ONE opening whose channel both of its air paths
 * read. V is the flow the opening WOULD carry: whether a controlled path is open remains that path's decision, and path_q
 * shows what actually moved. The caller's host channel array is never written; a derived column's host values are ignored.
 * resume == 0 initialises the accumulators on the device (sums 0, max_v = -inf, step_max = -1); a series of k steps followed
 * by one of n - k with the returned arrays and step_base + k gives the bits of the series of n. n_sub == 0 still evaluates
 * every step. A NaN V is data here: it becomes HEAT_N_NAN_ZONE where a consumer adds it to a zone, as today. An array that is
 * not asked for costs no traffic and changes no bit of the others. With op == NULL or n_openings == 0
 * heat_batch_march_series_openings is heat_batch_march_series_species exactly: same launches, same bits. A refused call
 * leaves the device state untouched. Sharded batches are refused as by the series.
 * heat_openings_check (host-only; it also builds and verifies the tables the march uploads) and
 * heat_batch_march_series_openings run the same checks before any device work; every message names "opening i".
 * HEAT_E_INVALID_ARG: a negative count; a NULL array that a positive count needs (zone_a, zone_b, out_chan, area);
 * zone_a == zone_b; an area or coefficient that is not finite or is negative. HEAT_E_SIZE: a zone out of range (zone_b in
 * [-1, n_zones)); a channel out of range (wind_chan and frac_chan may be -1); zone_b == -1 without a temperature channel; a
 * temperature channel on a zone-to-zone opening; two openings with the same out_chan; an out_chan that is also some
 * opening's temp_chan, wind_chan or frac_chan — a derived channel feeds consumers and never another opening.
 * Out of scope: a pressure network or mass balance across several openings, two-way flow with a neutral plane resolved over
 * the opening height, wind pressure coefficients from direction, density of moist air, and the opening's own effect on
 * convection coefficients.
 * (The flows of several openings that balance one another are a term of their own: heat_air_networks, below.)
 */
typedef struct heat_openings {
    int64_t n_openings;
    const int32_t *zone_a;              /* [n] a zone */
    const int32_t *zone_b;              /* [n] a zone, or -1: outside air at row[temp_chan] */
    const int32_t *temp_chan;           /* [n] nullable when no zone_b is -1; must be -1 where zone_b >= 0 */
    const int32_t *wind_chan;           /* [n] nullable / -1: no wind term; else the effective wind speed at the opening, m/s */
    const int32_t *frac_chan;           /* [n] nullable / -1: fully open; else the open fraction, clamped to [0, 1] */
    const int32_t *out_chan;            /* [n] the DERIVED channel this opening writes, m3/s */
    const double  *area;                /* [n] m2 (discharge coefficient folded in), finite, >= 0 */
    const double  *cw, *cs, *ca, *c0;   /* [n] each nullable = 0; finite, >= 0 */
    int64_t resume;                     /* as heat_air_species::resume, for the three accumulators below */
    int64_t step_base;                  /* K = step_base + k is what step_max records */
    /* accumulators, [n] each, in/out, nullable */
    double  *sum_v;
    double  *max_v;
    int64_t *step_max;                  /* kept where max_v is: it records the step of that maximum */
} heat_openings;

int heat_openings_check(const heat_batch_desc *desc, const heat_series *s, const heat_openings *op /* nullable */); /* host-only */
int heat_batch_march_series_openings(heat_batch *b, const heat_series_call *call, heat_comfort *c /* nullable */,
                                     double *operative, double *mrt, heat_air_handlers *h /* nullable */,
                                     double *supply_t, double *recovered, double *coil_q, double *branch_q,
                                     heat_air_species *sp /* nullable */, double *conc_rows, double *vent_v, double *vent_q,
                                     heat_openings *op /* nullable */,
                                     double *opening_v /* [n_steps][n_openings], nullable */);

/*
 * Controllers of a series: modulating control loops as DERIVED CHANNELS. A thermostat of the zone loads is on or off at a
 * fixed power into the zone air, and ideal loads need no sizing; nothing else of a series can modulate. A controller senses
 * a temperature only the device holds — a zone's air, a node of a wall — or a channel, compares it with a setpoint channel
 * and WRITES its output into one column of the step's row in the device's copy of the channel table, as an opening does.
 * Every consumer reads that column as it reads any channel: a gain of the zone loads (a modulating radiator), a channel of
 * the room radiation (a panel), an opening's frac_chan (a window that follows the room temperature), an air path's volume,
 * a blind's schedule, and the driven solar input of a side, gain[s] * row[chan[s]], which front_alpha / back_alpha spread
 * over the wall's nodes: with an alpha row that is 1 at one node a controller's watts heat that node (underfloor heating, a
 * thermally activated ceiling), and since the back side's value is not clamped at zero a negative output cools it
 * (heat_amd/controllers.py, embed()). No struct and no kernel of those terms changes, and the march kernels do not. The
 * reference has no counterpart; the rule below is this library's own contract, defined against the per-call loop with the
 * same rule written on the host (heat_amd/controllers.py, apply()).
 * The rule of step k. The controllers are the FIRST kernel of the step, ahead of the openings — an opening's frac_chan may be
 * a controller's output — and nothing of the step has read the row yet. T = the zone AIR temperatures the device holds when
 * the step starts, N = the node temperatures it holds when the step starts, row = the device's channel[k]. Every line is ONE
 * rounded f64 operation in the order written, no fused multiply-add; a NaN makes every comparison false:
 *   per controller i:
 *     Ts = sense_kind 0: T[sense_index]
 *          sense_kind 1: N[surface sense_index, node sense_node]     (sense_node -1: the surface's last node)
 *          sense_kind 2: row[sense_index]
 *     sp = row[set_chan]
 *     e0 = sp - Ts;  e = action > 0 ? e0 : -e0          (heating / cooling action; a sign flip)
 *     enabled = en_chan < 0 or row[en_chan] > 0.0
 *     if lim_kind >= 0:                                  (a high-limit cut-out, e.g. a floor surface at 29 C)
 *         Tl = as Ts, from lim_kind / lim_index / lim_node
 *         if Tl > lim_hi: { if trip == 0: trips += 1;  trip = 1 }
 *         else if trip == 1 and Tl < lim_lo: trip = 0
 *     if not enabled: I = 0.0; u = 0.0
 *     else if trip == 1: u = 0.0                         (I is held)
 *     else:
 *         p = kp * e;  ie = ki * e;  I1 = I + ie
 *         if I1 < 0.0: I1 = 0.0;  if I1 > 1.0: I1 = 1.0;  I = I1     (clamped integrator: the anti-windup)
 *         ub = p + I1;  u = ub + bias
 *         if u < 0.0: u = 0.0;  if u > 1.0: u = 1.0
 *     span = out_hi - out_lo;  o = u * span;  out = out_lo + o
 *     row[out_chan] = out;  control_u[k][i] = u;  control_out[k][i] = out
 *     sum_u += u;  sum_out += out;  if u > 0.0: steps_on += 1;  if u >= 1.0: steps_sat += 1
 * ki is per step: the caller folds the step length in (a reset time of n steps is ki = kp / n). A NaN u stays NaN through
 * both clamps, and a NaN error makes the integral NaN whatever ki is (0 * NaN), which it stays until the controller is
 * disabled; a NaN u or out is data here, as a NaN V is for openings: it becomes HEAT_N_NAN_ZONE where a consumer adds it
 * to a zone. The caller's host channel array is never written; a derived column's host values are ignored.
 * State and accumulators are in/out and nullable. resume == 0 starts them on the device (I = 0, trip = 0, sums and counts 0);
 * resume != 0 takes them from the arrays (a NULL one starts at zero). A series of k steps followed by one of n - k with the
 * returned arrays gives the bits of the series of n. The state is kept on the device whether or not the caller takes it.
 * n_sub == 0 still evaluates every step. An array that is not asked for costs no traffic and changes no bit of the others.
 * With ct == NULL or n_controllers == 0 heat_batch_march_series_controllers is heat_batch_march_series_openings exactly:
 * same launches, same bits. A refused call leaves the device state untouched. Sharded batches are refused as by the series.
 * heat_controllers_check (host-only; it also builds and verifies the tables the march uploads, with the nodes numbered as
 * the descriptor numbers them) and heat_batch_march_series_controllers run the same checks before any device work; every
 * message names "controller i". HEAT_E_INVALID_ARG: a negative count; a NULL array that a positive count needs
 * (sense_index, set_chan, out_chan, kp, out_hi; lim_index, lim_hi and lim_lo where some lim_kind >= 0); a sense_kind
 * outside [0, 2] or a lim_kind outside [-1, 2]; a constant that is not finite; kp or ki negative; lim_lo > lim_hi; on
 * resume a tripped byte above 1 or an integral outside [0, 1]. HEAT_E_SIZE: a zone, surface or channel out of range
 * (en_chan may be -1); a sense_node or lim_node outside [-1, the surface's nodes); set_chan missing (-1); two controllers
 * with the same out_chan; an out_chan that is also some opening's out_chan; an out_chan that any controller reads, as sense,
 * setpoint, enable or limit channel — a controller never reads a controller; a controller that reads an opening's out_chan,
 * because the openings run behind the controllers. With these every element of the row has one writer, and no lane reads
 * what another writes.
 * Out of scope: sensing the comfort term's operative temperature, which is formed later in the step; cascades, where a
 * controller reads a controller; minimum on and off times; derivative action; any change to the march kernels.
 */
typedef struct heat_controllers {
    int64_t n_controllers;
    const int32_t *sense_kind;          /* [n] nullable = 0; 0: a zone's air, 1: a node of a surface, 2: a channel */
    const int32_t *sense_index;         /* [n] the zone, the surface (the descriptor's number) or the channel */
    const int32_t *sense_node;          /* [n] nullable = -1; kind 1: the node, -1: the surface's last node; else ignored */
    const int32_t *set_chan;            /* [n] the setpoint */
    const int32_t *action;              /* [n] nullable = +1; > 0: heating (e = sp - Ts), else cooling (e = Ts - sp) */
    const int32_t *en_chan;             /* [n] nullable / -1: always enabled; else enabled where row[en_chan] > 0 */
    const int32_t *lim_kind;            /* [n] nullable / -1: no limit; else as sense_kind */
    const int32_t *lim_index;           /* [n] as sense_index, where lim_kind >= 0 */
    const int32_t *lim_node;            /* [n] nullable = -1, as sense_node */
    const int32_t *out_chan;            /* [n] the DERIVED channel this controller writes */
    const double  *kp;                  /* [n] 1 / K, finite, >= 0 (a proportional band of B K is kp = 1 / B) */
    const double  *ki;                  /* [n] nullable = 0; 1 / K per step, finite, >= 0 */
    const double  *bias;                /* [n] nullable = 0; finite */
    const double  *out_lo;              /* [n] nullable = 0; the output at u = 0, finite */
    const double  *out_hi;              /* [n] the output at u = 1, finite (below out_lo: a reverse-acting or cooling output) */
    const double  *lim_hi, *lim_lo;     /* [n] trip above lim_hi, release below lim_lo; finite, lim_lo <= lim_hi */
    int64_t resume;                     /* as heat_openings::resume, for the state and the accumulators below */
    /* state, [n] each, in/out, nullable */
    double  *integral;                  /* I, in [0, 1] */
    uint8_t *tripped;                   /* trip, 0 or 1 */
    /* accumulators, [n] each, in/out, nullable */
    double  *sum_u, *sum_out;
    int64_t *steps_on, *steps_sat, *trips;
} heat_controllers;

int heat_controllers_check(const heat_batch_desc *desc, const heat_series *s, const heat_openings *op /* nullable */,
                           const heat_controllers *ct /* nullable */); /* host-only */
int heat_batch_march_series_controllers(heat_batch *b, const heat_series_call *call, heat_comfort *c /* nullable */,
                                        double *operative, double *mrt, heat_air_handlers *h /* nullable */,
                                        double *supply_t, double *recovered, double *coil_q, double *branch_q,
                                        heat_air_species *sp /* nullable */, double *conc_rows, double *vent_v, double *vent_q,
                                        heat_openings *op /* nullable */, double *opening_v,
                                        heat_controllers *ct /* nullable */,
                                        double *control_u   /* [n_steps][n_controllers], nullable */,
                                        double *control_out /* [n_steps][n_controllers], nullable */);

/*
 * Air networks of a series: pressure-balanced flows as DERIVED CHANNELS. An opening (heat_openings) is an explicit formula of
 * its own two temperatures, so nothing makes the flows of a building add up: cross ventilation, a stairwell's stack effect
 * over several storeys and the infiltration an extract fan pulls in cannot be expressed, and the species ride on flows that
 * do not conserve mass. A network is a building's zones joined by links. Per step and per network the device solves the zone
 * reference pressures that balance the mass flows through all links — the pressures depend on the zone temperatures of the
 * moment, which only the device holds — and WRITES each link's volume flow into derived channels of the step's row. The air
 * paths read those as any channel, and the loads' flows, the handlers' branches and the species read them through the air
 * paths: a zone-to-zone link feeds two paths, a -> b with volume out_ab and b -> a with volume out_ba; an outside link feeds
 * one supply path (source -1, the same temp_chan) with volume out_ba; what leaves a zone enters no balance, so out_ab of an
 * outside link is normally -1. The air path's m = rho(Ts) V is the network's ru q: heat and species ride on flows that
 * conserve mass. A tall doorway is two links at 1/4 and 3/4 of its height: two-way flow falls out of the balance. No existing
 * struct, kernel or check changes. The reference has no counterpart; the rule below is this library's own contract, defined
 * against the per-call loop with the same rule written on the host (heat_amd/air_networks.py, apply()). It is what
 * EnergyPlus' AirflowNetwork, CONTAM and COMIS solve per time step, with Walton's AIRNET acceleration.
 * Structure. Network w owns the nodes net_offset[w] ... net_offset[w + 1] - 1 of node_zone: zones, in the caller's order; a
 * zone is in at most one network; 1 <= n_w <= 64. Link l joins zone_a[l] to zone_b[l], a zone of the same network or -1:
 * outside. c: the flow coefficient, m3/s per sqrt(Pa), discharge coefficient and area folded in; gh: 9.81 times the link's
 * height above the network's datum; p_lin > 0: below it the law is linear. frac_chan (optional) scales c, clamped to [0, 1];
 * it may be a controller's output. Outside links: temp_chan, the outside temperature, and optionally wp_chan with wp_gain,
 * the wind pressure at the link in Pa (the caller forms 1/2 rho Cp(theta) u2 per facade as a schedule). Per node an optional
 * src_chan with src_gain: a net mechanical mass inflow in kg/s (an extract fan is negative). Per network tol (kg/s),
 * max_iter and g_min, a conductance to the datum that keeps the matrix definite.
 * The rule of step k. Order in the step: controllers -> openings -> networks -> everything else, unchanged. T = the zone AIR
 * temperatures the device holds when the step starts, row = the device's channel[k], P = the node pressures the step before
 * left (state). Every line is ONE rounded f64 operation in the order written, no fused multiply-add; sqrt is correctly
 * rounded; no pow, no transcendental function; a NaN makes every comparison false:
 *   rho(t):  tk = t + 273.15;  rho = 101325 * 28.97 / (8314.46261815324 * tk)     (expression and grouping of heat_air_paths' rho)
 *   link l, a = its first node, b = its second node or outside:
 *     f = frac_chan >= 0 ? row[frac_chan] : 1.0;  if f < 0.0: f = 0.0;  if f > 1.0: f = 1.0;  C = c * f
 *     ra = rho(T[zone_a]);  rb = b is a zone ? rho(T[zone_b]) : rho(row[temp_chan])
 *     pb = b is a zone ? P[b] : (wp_chan >= 0 ? wp_gain * row[wp_chan] : 0.0)
 *     dr = ra - rb;  sh = gh * dr;  d0 = P[a] - pb;  dp = d0 - sh;  ad = |dp|
 *     if ad >= p_lin:  s = sqrt(ad);  q = C * s;  hq = 0.5 * q;  gq = hq / ad
 *     else:            ca = C * ad;  q = ca / s_lin;  gq = C / s_lin          (s_lin = sqrt(p_lin), formed once on the host)
 *     fwd = dp >= 0.0;  ru = fwd ? ra : rb;  m = ru * q;  gm = ru * gq;  ms = fwd ? m : -m
 *   assemble:  F[i] = src_chan >= 0 ? src_gain * row[src_chan] : 0.0;  A[i][i] = g_min;  A[i][j] = 0.0
 *     links of the network in ascending l:  F[a] = F[a] - ms;  A[a][a] = A[a][a] + gm
 *         b a zone:  F[b] = F[b] + ms;  A[b][b] = A[b][b] + gm;  A[a][b] = A[a][b] - gm;  A[b][a] = A[b][a] - gm
 *     res = 0.0;  for i ascending:  af = |F[i]|;  if af > res: res = af
 *   iterate:  dold[i] = 0.0;  conv = 0
 *     for it = 0 ... max_iter - 1:  assemble;  if res <= tol: conv = 1, stop
 *         eliminate, no pivoting (A is symmetric positive definite):  for kk ascending, r > kk:  fac = A[r][kk] / A[kk][kk]
 *             for j > kk ascending:  t = fac * A[kk][j];  A[r][j] = A[r][j] - t
 *             t = fac * F[kk];  F[r] = F[r] - t
 *         back-substitute by columns:  for j = n - 1 ... 0:  d[j] = F[j] / A[j][j];  for r < j:  t = A[r][j] * d[j];  F[r] = F[r] - t
 *         per node (Walton's AIRNET acceleration):  w = 1.0;  if dold[i] != 0.0: { r = d[i] / dold[i];  if r < -0.5: { o = 1.0 - r;  w = 1.0 / o } }
 *             dn = w * d[i];  P[i] = P[i] + dn;  dold[i] = dn
 *     if conv == 0:  assemble once more (the flows written belong to the final P);  unconverged += 1
 *   write, per link from the last assembly:  link_q[k][l] = fwd ? q : -q;  row[out_ab] = fwd ? q : 0.0;  row[out_ba] = fwd ? 0.0 : q   (where not -1)
 *              sum_ab += (fwd ? q : 0.0);  sum_ba += (fwd ? 0.0 : q)
 *   per network:  net_iters[k][w] = it, the iterations that solved;  iters_sum += it;  if res > max_res: max_res = res
 *   per node:  node_p[k][i] = P[i]
 * Plain Newton on a square-root law maps x to -x and cycles; the acceleration halves such a step. The flows hold for all
 * sub-timesteps of the step, as every a0 / b0 term does. A NaN temperature makes the flows it reaches NaN; |NaN| never raises
 * res, so a network whose every residual is NaN stops at once. NaN flows are data until a consumer adds them to a zone
 * (HEAT_N_NAN_ZONE, as today). The caller's host channel array is never written; a derived column's host values are ignored.
 * State and accumulators are in/out and nullable: pressure [n_nodes] is state, carried over a cut; sum_ab, sum_ba per link;
 * iters_sum, unconverged, max_res per network. resume == 0 starts them on the device at zero; resume != 0 takes them from the
 * arrays (a NULL one starts at zero). A series of k steps followed by one of n - k with the returned arrays gives the bits of
 * the series of n. The pressures are kept on the device whether or not the caller takes them. n_sub == 0 still evaluates
 * every step. An array that is not asked for costs no traffic and changes no bit of the others. With nw == NULL or
 * n_networks == 0 heat_batch_march_series_networks is heat_batch_march_series_controllers exactly: same launches, same bits.
 * A network reads no opening's out_chan and no network's; no opening or controller reads a network's; every derived column
 * has one writer. A network may read a controller's output channel.
 * A refused call leaves the device state untouched. Sharded batches are refused as by the series. heat_air_networks_check
 * (host-only; it also builds and verifies the tables the march uploads) and heat_batch_march_series_networks run the same
 * checks before any device work; every message names "network w", "node i" or "link l". HEAT_E_INVALID_ARG: a negative
 * count; a NULL array that a positive count needs (net_offset, node_zone, tol, max_iter, g_min; zone_a, zone_b, temp_chan, c,
 * p_lin); a c, gh or tol that is not finite or is negative; a p_lin or g_min that is not positive and finite; a src_gain or
 * wp_gain that is not finite; max_iter outside [1, 64]; zone_a == zone_b; on resume a pressure that is not finite.
 * HEAT_E_SIZE: a zone or channel out of range; net_offset not starting at 0, not ending at n_nodes or with a network of 0 or
 * of more than 64 nodes; a zone in two networks; a link whose zones are in different networks or in none; an outside link
 * without temp_chan, or a zone-to-zone link with a temp_chan or wp_chan; a network with no outside link; two writers of one
 * channel (out_ab, out_ba, an opening's or a controller's out_chan); a network that reads an opening's or a network's derived
 * channel; an opening or a controller that reads a network's.
 * Out of scope: power-law exponents other than 1/2; ducts and fan curves; wind pressure coefficients from direction (the
 * caller's wp_chan carries them); moist-air density; networks of more than 64 zones; more than one datum per network; any
 * change to the march kernels or to a consumer.
 */
typedef struct heat_air_networks {
    int64_t n_networks, n_nodes, n_links;
    const int32_t *net_offset;          /* [n_networks + 1] into node_zone, ascending from 0 to n_nodes */
    const double  *tol;                 /* [n_networks] kg/s, finite, >= 0 */
    const int32_t *max_iter;            /* [n_networks] in [1, 64] */
    const double  *g_min;               /* [n_networks] kg/s per Pa, finite, > 0 */
    const int32_t *node_zone;           /* [n_nodes] the zone of every node */
    const int32_t *src_chan;            /* [n_nodes] nullable / -1: no source */
    const double  *src_gain;            /* [n_nodes] nullable = 1; finite */
    const int32_t *zone_a;              /* [n_links] a zone of a network */
    const int32_t *zone_b;              /* [n_links] a zone of the same network, or -1: outside */
    const int32_t *temp_chan;           /* [n_links] the outside temperature where zone_b == -1, else -1 */
    const int32_t *wp_chan;             /* [n_links] nullable / -1: no wind pressure; only where zone_b == -1 */
    const int32_t *frac_chan;           /* [n_links] nullable / -1: fully open */
    const int32_t *out_ab;              /* [n_links] nullable / -1: the DERIVED channel of the flow a -> b, m3/s */
    const int32_t *out_ba;              /* [n_links] nullable / -1: the DERIVED channel of the flow b -> a, m3/s */
    const double  *c;                   /* [n_links] m3/s per sqrt(Pa), finite, >= 0 */
    const double  *gh;                  /* [n_links] nullable = 0; m2/s2, finite, >= 0 */
    const double  *p_lin;               /* [n_links] Pa, finite, > 0 */
    const double  *wp_gain;             /* [n_links] nullable = 1; finite */
    int64_t resume;                     /* as heat_openings::resume, for the state and the accumulators below */
    double  *pressure;                  /* [n_nodes] state, in/out, nullable: Pa, finite */
    double  *sum_ab;                    /* [n_links] accumulators, in/out, nullable */
    double  *sum_ba;
    int64_t *iters_sum;                 /* [n_networks] */
    int64_t *unconverged;
    double  *max_res;
} heat_air_networks;

int heat_air_networks_check(const heat_batch_desc *desc, const heat_series *s, const heat_openings *op /* nullable */,
                            const heat_controllers *ct /* nullable */, const heat_air_networks *nw /* nullable */); /* host-only */
int heat_batch_march_series_networks(heat_batch *b, const heat_series_call *call, heat_comfort *c /* nullable */,
                                     double *operative, double *mrt, heat_air_handlers *h /* nullable */,
                                     double *supply_t, double *recovered, double *coil_q, double *branch_q,
                                     heat_air_species *sp /* nullable */, double *conc_rows, double *vent_v, double *vent_q,
                                     heat_openings *op /* nullable */, double *opening_v,
                                     heat_controllers *ct /* nullable */, double *control_u, double *control_out,
                                     heat_air_networks *nw /* nullable */,
                                     double  *link_q    /* [n_steps][n_links], nullable */,
                                     double  *node_p    /* [n_steps][n_nodes], nullable */,
                                     int32_t *net_iters /* [n_steps][n_networks], nullable */);

/* Where the numerical failure heat_batch_synchronize / heat_batch_march last reported was seen FIRST (the reference's
 * panics name the offending values, surface.rs:704-707; model.rs:417-420): *index = the surface's number in the
 * descriptor — or the zone's, when *kind == HEAT_N_NAN_ZONE found by the zone balance itself (the cluster-resident
 * march reports a surface of the zone's cluster instead) — and *kind = the HEAT_N_* code seen there. -1 / 0 when no
 * failure has been reported yet. Host-side bookkeeping: no device access. */
int heat_batch_failed_surface(const heat_batch *b, int64_t *index, int32_t *kind);

/* Split-phase sub-timestep, for the sharded (multi-GPU) case. All asynchronous on the stream.
 * step_surfaces ≙ iterate_surfaces over this rank's surfaces + this rank's partial (a,b) sums.
 * step_zones    ≙ the zone update from `gathered` = n_ranks consecutive partial blocks
 *                 (device pointer, layout [rank][2][n_zones]: a then b), summed in rank order. */
/* set_weather: the weather of the next n_sub sub-timesteps (n_sub * n_sites records [k * n_sites + s] on a batch of
 * weather sites) and the zones' a0 / b0 terms. */
int heat_batch_set_weather(heat_batch *b, const heat_weather *weather, int32_t n_sub,
                           const double *zone_a0, const double *zone_b0);
int heat_batch_step_surfaces(heat_batch *b, int32_t sub_step);
int heat_batch_step_zones(heat_batch *b, const double *gathered_dev, int32_t n_blocks);
double *heat_batch_zone_partials(heat_batch *b); /* device pointer, [2][n_zones] doubles */
/* Makes step_surfaces write the partial sums into caller-owned device memory ([2][n_zones] doubles,
 * e.g. a tensor the caller hands to its collective); NULL restores the batch's own buffer. */
int heat_batch_use_partials(heat_batch *b, double *partials_dev);
/* Sharded batches, compact exchange. heat_batch_touched_zones fills mask[n_zones] with 1 for every zone a surface
 * of this batch faces. After the ranks have agreed on the zones more than one of them touches,
 * heat_batch_set_shared_zones(shared_zone[n_shared]: global zone numbers, the same list in the same order on every
 * rank) switches the split-phase sequence to the compact form: heat_batch_step_surfaces updates the zones only this
 * rank touches at once and writes the partial (a, b) of the shared ones into the partials buffer, laid out
 * [2][n_shared]; heat_batch_step_zones(gathered, n_blocks) then updates the shared zones from the gathered blocks
 * [block][2][n_shared], summed in block order. Zones this rank does not touch are not kept up to date on it. */
int heat_batch_touched_zones(const heat_batch *b, uint8_t *mask);
int heat_batch_set_shared_zones(heat_batch *b, const int32_t *shared_zone, int32_t n_shared);

/*
 * Library-owned collective (the default multi-GPU mode; one process per GPU): the batch holds an RCCL
 * communicator and heat_batch_march_resident / heat_batch_march run the whole sharded sub-timestep on the batch's
 * stream: surfaces -> zones only this rank touches + partial (a, b) of the shared ones -> ncclAllGather of the
 * [2][n_shared] blocks over xGMI -> shared zones updated from the blocks summed in rank order. No torch, no second
 * stream: a kernel, a collective and a kernel in one queue.
 *   heat_comm_unique_id   ncclGetUniqueId; one rank calls it and the host program hands the bytes to every rank
 *                         (any means: MPI, a file, torch.distributed's store, ...).
 *   heat_batch_comm_init  ncclCommInitRank(n_ranks, rank of the batch's options) — collective: every rank calls it;
 *                         then the ranks agree on the shared zones (an all-reduce of the touched masks) and the
 *                         batch is switched to the compact exchange (as heat_batch_set_shared_zones does).
 * RCCL is loaded at run time (dlopen "librccl.so.1"); without it both calls return HEAT_E_COMM.
 *   heat_comm_available   HEAT_OK when RCCL can be loaded (no collective inside: the ranks can vote on it BEFORE any
 *                         of them enters the collective heat_batch_comm_init).
 *   heat_batch_comm_init_ex  as heat_batch_comm_init, with extra_shared[n_extra] zones exchanged as well (the union
 *                         with the agreed list; tests and single-GPU rehearsals of the exchange).
 * Zones NO rank faces still follow their a0 / b0 terms (model.rs:410-423): rank z % n_ranks finishes zone z
 * (heat_batch_comm_init and heat_batch_create_shard arrange that; heat_batch_set_owned_zones for callers that cut
 * their shards themselves: owned[n_zones], OR-ed with the zones the batch's surfaces face).
 * A sharded batch that shares no zone with another rank — a partition along the clusters, heat_partition —
 * needs no communicator at all: after heat_batch_set_shared_zones(b, NULL, 0) (heat_batch_create_shard does it)
 * heat_batch_march[_resident] run as on a single GPU, on the zones the batch owns.
 */
#define HEAT_COMM_ID_BYTES 128
int heat_comm_available(void);
int heat_comm_unique_id(uint8_t id[HEAT_COMM_ID_BYTES]);
int heat_batch_comm_init(heat_batch *b, const uint8_t id[HEAT_COMM_ID_BYTES]);
int heat_batch_comm_init_ex(heat_batch *b, const uint8_t id[HEAT_COMM_ID_BYTES], const int32_t *extra_shared,
                            int32_t n_extra);
int heat_batch_set_owned_zones(heat_batch *b, const uint8_t *owned);
int32_t heat_batch_n_shared_zones(const heat_batch *b);
/* Ranks of the batch's communicator (0: it has none — single GPU, a partition that shares no zone, or a host that
 * brings its own collective). */
int32_t heat_batch_comm_ranks(const heat_batch *b);
/* Gives the communicator up (ncclCommDestroy) and returns the batch to "sharded, no communicator, shared zones not
 * agreed": for a host whose ranks found out — collectively, by their own means — that heat_batch_comm_init failed
 * on SOME rank, and that now fall back to the split-phase calls with their own collective on EVERY rank. No-op
 * without a communicator. (A failed heat_batch_comm_init[_ex] has already done this on the rank it failed on.) */
int heat_batch_comm_destroy(heat_batch *b);

/*
 * Cluster-resident march (on by default). ThermalModel::march runs its dt_subdivisions sub-timesteps back to back
 * and nothing outside reads the state in between (model.rs:369-424), and surfaces exchange heat only through the
 * zones they face (model.rs:556-590). So the batch is cut into zone-connected clusters; a cluster whose surfaces
 * are all palette-form fast-path walls (gas cavities between massive nodes and no-mass chunks of one or two nodes
 * allowed with 4 or 8 nodes per lane) or small all-no-mass surfaces, and for which the planner's cost model expects a
 * gain, is marched for ALL n_sub sub-timesteps of a heat_batch_march[_resident] call resident on the chip: node
 * temperatures stay in registers, the zone balance is summed on the chip, and only the final temperatures,
 * coefficients and flows are written. A cluster of up to eight wavefronts is one workgroup's; a larger one (a building
 * whose rooms are all joined by interior walls: up to 32 wavefronts, 256 zones) is marched by a TEAM of up to eight
 * workgroups that exchange the partial sums of the zones they share through L2 once per sub-timestep (a march that
 * could not complete that exchange returns HEAT_E_DEVICE). Everything else is streamed one sub-timestep per launch. The zone sums (here and in the streamed k_zones) are lane-strided partial sums followed
 * by a fixed reduction tree: deterministic run to run, but NOT the sequential surface order of model.rs:562-585 — the
 * results differ from a sequential sum by rounding (~1e-16 relative; everything is tested at 1e-9 against the oracle).
 * March calls of a single sub-timestep are streamed as well (the fused launch pays off from two on).
 * heat_batch_set_fusion(b, 0) streams everything (used to measure the per-sub-timestep kernel on its own). */
int heat_batch_set_fusion(heat_batch *b, int32_t enabled);
int64_t heat_batch_n_fused_surfaces(const heat_batch *b);
int64_t heat_batch_n_fused_launches(const heat_batch *b); /* cluster-resident launches issued since creation */

/*
 * Ideal loads in the cluster-resident march (heat_ideal_loads, RESIDENT FORM), opt-in per batch. Default 0: an ideal series
 * marches streamed, every bit and every launch as without this call. enabled != 0 is durable until set again and
 * independent of heat_batch_set_fusion (which still decides whether anything marches resident at all).
 * heat_batch_ideal_resident: 1 when the next ideal series of this batch would march its resident clusters resident — the
 * opt-in, fusion on, and an eligible batch — otherwise 0 (also for a NULL batch).
 * heat_plan_ideal_resident (host-only, needs no device; arguments as heat_plan_check_sites, n_sites = 1 and a NULL
 * site_of_surface for a single site): 1 when a batch made from this descriptor and these options is eligible, 0 when not,
 * a negative heat_status when the descriptor cannot be planned; *reason (nullable) receives why not. opt->no_fusion = 1
 * plans nothing resident, so the answer is 0, HEAT_IDEAL_RESIDENT_NONE_PLANNED. The batch asks the same function of its
 * own plan.
 */
typedef enum heat_ideal_resident_reason {
    HEAT_IDEAL_RESIDENT_OK = 0,
    HEAT_IDEAL_RESIDENT_NONE_PLANNED = 1,     /* nothing of the batch is planned resident */
    HEAT_IDEAL_RESIDENT_TEAMS = 2,            /* clusters marched by teams of workgroups */
    HEAT_IDEAL_RESIDENT_CAVITY_CLASS = 3,     /* resident workgroups of walls only in a class with gas cavities (workgroups
                                                 that also hold small surfaces — rooms with windows — are eligible) */
    HEAT_IDEAL_RESIDENT_CHUNK_LOOP_CLASS = 4  /* resident workgroups in a class with no-mass chunks other than facings */
} heat_ideal_resident_reason;
int heat_batch_set_ideal_resident(heat_batch *b, int32_t enabled);
int32_t heat_batch_ideal_resident(const heat_batch *b);
int heat_plan_ideal_resident(const heat_batch_desc *desc, const heat_batch_options *opt, int32_t n_sites,
                             const int32_t *site_of_surface, int32_t *reason);

/* Introspection (tests, bench). */
int64_t heat_batch_n_surfaces(const heat_batch *b);
int64_t heat_batch_n_nodes(const heat_batch *b);
int64_t heat_batch_n_zones(const heat_batch *b);
/* Bytes one sub-timestep must move at minimum: 32 B per node + per-surface scalars. */
int64_t heat_batch_algorithmic_bytes(const heat_batch *b);
/* Total iterations of the no-mass fixed-point loop (surface.rs:808-896) since creation. */
int64_t heat_batch_nomass_iterations(heat_batch *b);
/* Number of surfaces routed to {fast M=4, fast M=8, fast M=16, small all-no-mass, general catch-all}. */
int heat_batch_class_counts(const heat_batch *b, int64_t counts[5]);
/* Kernel timing with HIP events recorded on the batch's stream around the surface kernels of
 * every sub-timestep executed while enabled (the march then runs eagerly, not as a graph).
 * heat_batch_get_timing synchronises and returns the mean duration in microseconds of the
 * surface kernels of one sub-timestep (*surf_us), of one whole sub-timestep (*substep_us) and
 * the number of sub-timesteps sampled; it then clears the samples.
 * enabled = k > 1: of the streamed march calls only every k-th one records events (and runs eagerly); the others
 * replay the graph as they do untimed — the rate of a timed region then stays close to the untimed one. */
int heat_batch_set_timing(heat_batch *b, int32_t enabled);
int heat_batch_get_timing(heat_batch *b, double *surf_us, double *substep_us, int64_t *n_samples);

/*
 * Partition of a model over the GPUs of a node (host-only: needs no device). Surfaces exchange heat only through
 * the zones they face (model.rs:556-590), so a shard cut ALONG the zone-connected clusters shares no zone with
 * another shard and needs no exchange at all; only a cluster heavier than a quarter of a shard (a whole building
 * whose zones are all joined by interior walls) is cut by surface ranges, sharing zones at the cuts.
 *   rank_of_surface[n_surfaces]   out: the rank every surface goes to, in [0, n_ranks); balanced by the algorithmic
 *                                 bytes of the surfaces (32 n + 152), clusters kept in model order
 *   n_shared_zones                out, nullable: zones faced by surfaces of more than one rank (0: no collective
 *                                 is ever issued by the sharded march)
 * heat_batch_create_shard builds the batch of one rank from the WHOLE model's descriptor and that partition
 * (rank = opt->rank; zones, cavities and state slots stay global).
 */
int heat_partition(const heat_batch_desc *desc, int32_t n_ranks, int32_t *rank_of_surface, int64_t *n_shared_zones);
int heat_batch_create_shard(const heat_batch_desc *desc, const heat_batch_options *opt, const int32_t *rank_of_surface,
                            heat_batch **out);
/* Host-only self-check of the planner (tests): plans `desc` as heat_batch_create_ex would and verifies the plan's
 * internal consistency (every surface in exactly one tile, every index inside its array, every workgroup of the
 * cluster-resident march inside the kernel's limits). summary (nullable): surfaces per kernel class [5], surfaces
 * in the cluster-resident march, its workgroups, tiles. */
int heat_plan_check(const heat_batch_desc *desc, const heat_batch_options *opt, int64_t summary[8]);
/* Same for a batch of weather sites (heat_batch_create_sites: the same argument checks and codes), and checks that every
 * tile, cluster-resident workgroup and team holds surfaces of one site. n_sites == 1: what heat_plan_check gives. */
int heat_plan_check_sites(const heat_batch_desc *desc, const heat_batch_options *opt, int32_t n_sites,
                          const int32_t *site_of_surface, int64_t summary[8]);

const char *heat_last_error(void);
int heat_amd_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
