// plan.hpp — host-only planning of a heat batch: descriptor checks, classification of the surfaces into kernel
// classes, zone-connected clusters and their workgroups (cluster-resident march), tiles, the packed constants in
// the device layout (layout.hpp), zone contribution lists, and the partition of a model over ranks.
//
// Nothing here touches a device: plan.cpp compiles with g++ as well as hipcc, so that the planner runs under
// AddressSanitizer / UBSan on the CPU (tests/test_planner_host.py) — heat_batch_create only uploads what
// make_plan produced.
#pragma once
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/heat_amd.h"
#include "layout.hpp"

namespace heat {

constexpr int kMaxNodesGeneral = 4096;
constexpr int kScratchArrays = 7;
// fast classes: index = mi * 6 + nm * 3 + v;  M = 4 << mi;  nm: no-mass facings allowed;
// v = 0 per-node arrays, 1 palette constants, 2 palette + gas cavities between massive nodes
constexpr int kNumFast = 18;
extern const int kFastM[kNumFast], kFastNM[kNumFast], kFastPAL[kNumFast], kFastCAV[kNumFast];
constexpr int kSmall = kNumFast;         // all-no-mass surfaces of <= 4 nodes (general layout, register kernel)
constexpr int kSmallCav = kNumFast + 1;  // ... with a gas cavity (double glazing)
constexpr int kGeneral = kNumFast + 2;   // catch-all

// Everything heat_batch_create uploads, in device order.
struct Plan {
    int64_t n_surf = 0, n_zones = 0, n_state = 0, n_nodes = 0, n_cav = 0;
    double dt = 0;
    int64_t algorithmic_bytes = 0;
    int64_t class_counts[5] = {0, 0, 0, 0, 0};  // M4, M8, M16, small, general
    int64_t n_palette = 0;                      // surfaces whose constants are in palette form
    int64_t n_fused_surfaces = 0;

    // tiles
    std::vector<FastTile> fast_tiles[kNumFast];
    int n_stream_tiles[kNumFast] = {};  // tiles marched one sub-timestep per launch; the fused workgroups' tiles follow
    std::vector<GeneralTile> gen_tiles;  // [0, n_small_tiles) small (cavity-free first), the rest catch-all
    int n_small_tiles = 0, n_small_plain_tiles = 0, n_smallcav_stream_tiles = 0;
    int64_t gen_base = 0;       // first node slot of the general group
    int64_t node_slots = 0;     // total node slots incl. padding
    int64_t scratch_slots = 0;  // doubles of tri-diagonal scratch (catch-all kernel)

    // cluster-resident march: workgroup lists per class, index = width group (0: <= 4 wavefronts, 1: <= 8) + 2 * mixed
    std::vector<FusedBlock> fblocks[kNumFast][4];
    // teams of workgroups (clusters larger than one workgroup; layout.hpp, FusedSuper): the member blocks per class, the
    // clusters as runs of them, and per fused zone (fzones index) its exchange slot | members << 16
    std::vector<FusedBlock> team_blocks[kNumFast];
    std::vector<FusedSuper> team_supers[kNumFast];
    std::vector<uint32_t> team_zinfo;
    std::vector<int32_t> fzones, fzone_eoff;
    std::vector<uint16_t> fslots;
    std::vector<double> side_area;    // [2 * S]
    std::vector<int16_t> side_lzone;  // [2 * S]
    std::vector<int32_t> zone_block;  // zone -> fused workgroup (global number) or -1
    bool any_fused = false;

    // weather sites (heat_batch_create_sites): every tile, fused workgroup and team holds surfaces of one site, so the
    // kernels read the weather record of device surface surf_base's site for the whole wavefront (layout.hpp, SideArrays)
    int32_t n_sites = 1;
    std::vector<int32_t> dev_site;  // [S] site of device surface d; empty for a single-site batch

    // per-node constants (device layout)
    std::vector<double> V, U, alpha_f, alpha_b, mass, pal;
    std::vector<uint8_t> cls;
    int pal_stride = kPalNarrow;  // doubles per palette, and where its U entries start (layout.hpp)
    int pal_ubase = kPalVNarrow;
    std::vector<int32_t> cav_idx, cavref;
    std::vector<CavityDev> cavs;

    // where the nodes of a surface sit in the T buffer (ORIGINAL surface order; node_slot_index below): first node slot
    // of the surface's tile, and lanes the tile uses (Lk) | nodes per lane (M; 0: general layout) << 8 | the surface's
    // first lane << 16
    std::vector<int64_t> node_tile_base;
    std::vector<int32_t> node_geom;

    // per-surface records (device order)
    std::vector<int32_t> meta;
    std::vector<SideConst> side;
    std::vector<double> side_alpha, hs_fix;
    std::vector<int64_t> first_slot, slots;  // slots: 8 arrays of S
    std::vector<int64_t> dev_of, orig_of;    // original surface <-> device surface

    // zones
    std::vector<int64_t> zone_off, zone_slot;
    std::vector<double> zone_vol;
    std::vector<ZoneEntry> zone_entries;
    std::vector<uint8_t> touched;  // zones this batch's surfaces face

    // host copies used by download (original surface order)
    std::vector<int64_t> h_first_slot, h_node_count, h_out_slots[4];

    size_t nm_count_base[kNumFast + 1] = {};  // no-mass pass counters: one per tile of the NM fast classes, then
    size_t n_nm_counters = 0;                 // one per lane of the general-layout tiles
};

// Checks of heat_batch_create (reference: ThermalModel::new's Err / setup-time panics). Returns a heat_status.
int check_desc(const heat_batch_desc *d, std::string &err);
// The whole plan. Returns HEAT_OK or a negative heat_status with `err` set. site_of_surface (nullable: one site):
// the weather site of every surface, in [0, n_sites) — checked by check_sites first.
int make_plan(const heat_batch_desc *d, const heat_batch_options &opt, Plan &p, std::string &err, int32_t n_sites = 1,
              const int32_t *site_of_surface = nullptr);
// Internal consistency of a plan against its descriptor (every surface placed once, every index inside its
// array, every workgroup inside the kernel's limits; with sites: every tile, workgroup and team of one site). Used by
// the host-only tests; HEAT_OK or HEAT_E_SIZE.
int check_plan(const Plan &p, const heat_batch_desc *d, std::string &err, const int32_t *site_of_surface = nullptr);
// The arguments of heat_batch_create_sites / heat_plan_check_sites: HEAT_E_INVALID_ARG for a site count outside
// [1, kMaxSites] or a sharded batch, HEAT_E_SIZE for a surface whose site is out of range.
constexpr int32_t kMaxSites = 65536;
int check_sites(const heat_batch_desc *d, const heat_batch_options &opt, int32_t n_sites, const int32_t *site_of_surface,
                std::string &err);

// Ideal loads in the cluster-resident march (heat_batch_set_ideal_resident, include/heat_amd.h): whether EVERY resident
// launch a batch would make has an ideal instantiation of its kernel — decided for the whole batch from its workgroup
// lists: n_blocks[c][g2] workgroups per class and list (Plan::fblocks / heat_batch::h_fblocks), n_supers[c] team clusters,
// has_chunks[c] the class holds tiles with no-mass chunks other than facings (kTileChunkyBit). Returns a
// heat_ideal_resident_reason: HEAT_IDEAL_RESIDENT_OK, or why not — the first that applies of: nothing planned resident,
// teams, workgroups of walls only in a cavity class (a workgroup that also holds small surfaces marches the universal
// variant of its blocking factor, which has an ideal instantiation), workgroups that march with the chunk-loop variant.
// heat_plan_ideal_resident (from a plan) and the batch (from its lists) both ask this function.
int ideal_resident_reason(const size_t (&n_blocks)[kNumFast][4], const size_t (&n_supers)[kNumFast], const bool (&has_chunks)[kNumFast]);
const char *ideal_resident_reason_text(int reason);

// Index into the T buffer of node i of a surface placed at (tile_base, geom) — Plan::node_tile_base / node_geom; the
// layouts k_nodes_fast / k_nodes_general walk (layout.hpp).
inline int64_t node_slot_index(int64_t tile_base, int32_t geom, int i) {
    const int Lk = geom & 0xff, M = (geom >> 8) & 0xff, lane0 = (geom >> 16) & 0xff;
    if (M == 0) return tile_base + (int64_t)i * kWave + lane0;
    const int lane = lane0 + i / M, j = i % M;
    return tile_base + ((int64_t)(j >> 1) * Lk + lane) * 2 + (j & 1);
}

// Series march (heat_series, include/heat_amd.h): the host-only half. What a series may probe is described by the
// slots of the descriptor — or by the host copies a batch keeps of them — in the caller's surface order.
struct SeriesModel {
    int64_t n_surfaces = 0, n_zones = 0;
    const int64_t *first_node_slot = nullptr, *node_count = nullptr;  // [n_surfaces]
    const int64_t *out_slot[4] = {nullptr, nullptr, nullptr, nullptr};  // hs front, hs back, flow front, flow back
    const int64_t *zone_slot = nullptr;                                 // [n_zones]
};
enum : int { PROBE_NODE = 0, PROBE_HS_FRONT = 1, PROBE_HS_BACK = 2, PROBE_FLOW_FRONT = 3, PROBE_FLOW_BACK = 4, PROBE_ZONE = 5 };
// Slot of the caller's state -> what this path keeps there. The tables are sorted copies built when first needed, the
// zones' first (a run that probes its zones only never pays for the 4 S scalar slots); a batch keeps its resolver.
class SlotResolver {
  public:
    explicit SlotResolver(const SeriesModel &m) : m_(m) {}
    // kind: PROBE_*; index: the surface (or zone) in the caller's numbering; node: the node (PROBE_NODE). false: the slot
    // is none of this path's outputs.
    bool resolve(int64_t slot, int &kind, int64_t &index, int &node);

  private:
    SeriesModel m_;
    bool zones_built_ = false, nodes_built_ = false, scalars_built_ = false;
    std::vector<std::pair<int64_t, int64_t>> zones_, nodes_, scalars_;  // (slot, zone) | (first slot, surface) | (slot, 4 s + a)
};
// Everything heat_series_check promises (include/heat_amd.h). HEAT_OK or a negative heat_status with `err` set.
int check_series(const SeriesModel &m, SlotResolver &res, int32_t n_sites, const heat_series *s, std::string &err);

// Zone loads of a series (heat_zone_loads, include/heat_amd.h). Everything heat_zone_loads_check promises about the loads
// themselves; l == nullptr is no loads. HEAT_OK or a negative heat_status with `err` set.
int check_zone_loads(int64_t n_zones, int32_t n_channels, const heat_zone_loads *l, std::string &err);
// The tables of k_series_zone_loads (one lane per zone): the three term lists stably sorted by (target) zone — the caller's
// order survives inside a zone — each with CSR offsets; gains that are NULL in the ABI are ones here. th_orig keeps the
// caller's number of a thermostat: `applied` and the mode bytes stay in the caller's order.
struct ZoneLoadTables {
    std::vector<int32_t> off;  // [3][n_zones + 1]: gains, flows, thermostats
    std::vector<int32_t> gain_chan;
    std::vector<double> gain_factor;
    std::vector<int32_t> flow_volume_chan, flow_temp_chan;
    std::vector<double> flow_volume_gain;
    std::vector<int32_t> th_sensor, th_heat_chan, th_cool_chan, th_orig;
    std::vector<double> th_heat_power, th_cool_power, th_half_band;
};
// (of loads that passed check_zone_loads)
void build_zone_load_tables(int64_t n_zones, const heat_zone_loads *l, ZoneLoadTables &t);

// Air paths of a series (heat_air_paths, include/heat_amd.h). Everything heat_air_paths_check promises about the paths
// themselves; air == nullptr is none. HEAT_OK or a negative heat_status with `err` set, naming "air path i".
int check_air_paths(int64_t n_zones, int32_t n_channels, const heat_air_paths *air, std::string &err);
// The tables of k_series_air_paths (one lane per zone): the paths stably sorted by target zone — the caller's order survives
// inside a zone — with CSR offsets, packed into one int32 and one f64 buffer (one upload each). A NULL volume_gain is ones
// here, an uncontrolled path has open_chan -1 and sense, half band and min_delta 0; orig keeps the caller's number of a
// path: path_q, the state bytes and the accumulators stay in the caller's order.
struct AirPathTables {
    int64_t n_zones = 0, n_paths = 0;
    std::vector<int32_t> i32;  // off [n_zones + 1] | source [n] | temp_chan [n] | volume_chan [n] | open_chan [n] | orig [n]
    std::vector<double> f64;   // volume_gain [n] | sense [n] (+1.0 / -1.0) | half_band [n] | min_delta [n]
    const int32_t *off() const { return i32.data(); }
    const int32_t *list(int a) const { return i32.data() + (n_zones + 1) + a * n_paths; }  // 0 source .. 4 orig
    const double *real(int a) const { return f64.data() + a * n_paths; }                   // 0 volume_gain .. 3 min_delta
};
// (of paths that passed check_air_paths)
void build_air_path_tables(int64_t n_zones, const heat_air_paths *air, AirPathTables &t);
// The tables against the caller's lists (used by the host-only check): every path present exactly once, the caller's order
// kept inside a zone, the offsets monotone and inside the buffers. HEAT_OK or HEAT_E_SIZE.
int check_air_path_tables(int64_t n_zones, const heat_air_paths *air, const AirPathTables &t, std::string &err);

// Air handlers of a series (heat_air_handlers, include/heat_amd.h). Everything heat_air_handlers_check promises about the
// term itself; h == nullptr is none. HEAT_OK or a negative heat_status with `err` set, naming "air handler u" or "air handler
// branch j".
int check_air_handlers(int64_t n_zones, int32_t n_channels, const heat_air_handlers *h, std::string &err);
// The tables of k_series_handler_units (one lane per unit) and k_series_handler_supply (one lane per zone): ALL branches stably
// sorted by unit and the SUPPLY branches (kind bit 0) stably sorted by zone — two counting sorts, the caller's order survives
// inside a range — each with CSR offsets; orig keeps the caller's number of a branch: m, branch_q and sum_branch_q stay in
// the caller's order. The units' rows in the caller's order: a NULL eff_gain is ones here, a NULL channel list -1, a NULL
// capacity +inf; half band (band / 2, the one operation the header gives it) and min_delta 0 where the unit has no bypass.
enum HandlerI32 : int { AH_OUTDOOR_CHAN, AH_EFF_CHAN, AH_BYPASS_CHAN, AH_HEAT_CHAN, AH_COOL_CHAN, kHandlerI32Rows };
enum HandlerF64 : int { AH_EFF_GAIN, AH_HALF_BAND, AH_MIN_DELTA, AH_HEAT_CAP, AH_COOL_CAP, kHandlerF64Rows };
struct HandlerTables {
    std::vector<int32_t> unit_off;                  // [n_units + 1]
    std::vector<int32_t> u_zone, u_chan, u_orig;    // [n_branches] by unit
    std::vector<uint8_t> u_kind;                    // [n_branches]
    std::vector<double> u_gain;                     // [n_branches]
    std::vector<int32_t> zone_off;                  // [n_zones + 1]
    std::vector<int32_t> z_unit, z_orig;            // [n_supply] by zone
    std::vector<int32_t> i32;                       // [kHandlerI32Rows][n_units]
    std::vector<double> f64;                        // [kHandlerF64Rows][n_units]
};
// (of a term that passed check_air_handlers)
void build_air_handler_tables(int64_t n_zones, const heat_air_handlers *h, HandlerTables &t);
// The tables against the caller's lists (used by the host-only check): every branch present exactly once in its unit's
// range, every supply branch exactly once in its zone's, both in the caller's order, the offsets monotone and inside the
// buffers, every row the caller's. HEAT_OK or HEAT_E_SIZE.
int check_air_handler_tables(int64_t n_zones, const heat_air_handlers *h, const HandlerTables &t, std::string &err);

// Air species of a series (heat_air_species, include/heat_amd.h). Everything heat_air_species_check promises about the term
// itself; sp == nullptr is none. HEAT_OK or a negative heat_status with `err` set, naming "air species s", "species source i"
// or "demand vent j".
int check_air_species(int64_t n_zones, int32_t n_channels, const heat_air_species *sp, std::string &err);
// The tables of k_series_vents (one lane per zone) and k_series_species (one lane per (species, zone), lane = s * n_zones + z):
// the sources stably sorted by lane and the vents stably sorted by zone — two counting sorts, the caller's order survives
// inside a range — each with CSR offsets; v_orig keeps the caller's number of a vent: V, vent_v, vent_q and the vents'
// accumulators stay in the caller's order. A NULL src_factor is ones here, a NULL channel list -1. br_chan / br_gain: the
// volume channel and gain of every branch of the handlers in the CALLER's order (a NULL gain is ones), which the species'
// lanes reach through the handlers' own supply table (HandlerTables::zone_off, z_orig); empty without handlers.
struct SpeciesTables {
    std::vector<int32_t> outdoor_chan;                              // [n_species][n_zones]
    std::vector<int32_t> src_off;                                   // [n_species * n_zones + 1]
    std::vector<int32_t> src_chan;                                  // [n_sources] by lane
    std::vector<double> src_factor;                                 // [n_sources] by lane
    std::vector<int32_t> vent_off;                                  // [n_zones + 1]
    std::vector<int32_t> v_species, v_temp_chan, v_enable_chan, v_orig;   // [n_vents] by zone
    std::vector<double> v_min, v_max, c_lo, c_hi;                   // [n_vents] by zone
    std::vector<int32_t> limit_chan;                                // [n_species]
    std::vector<int32_t> occ_chan;                                  // [n_zones]
    std::vector<int32_t> br_chan;                                   // [n_branches], the caller's order
    std::vector<double> br_gain;                                    // [n_branches], the caller's order
};
// (of terms that passed check_air_handlers and check_air_species)
void build_air_species_tables(int64_t n_zones, const heat_air_handlers *h, const heat_air_species *sp, SpeciesTables &t);
// The tables against the caller's lists (used by the host-only check): every source present exactly once in its lane's
// range, every vent exactly once in its zone's, both in the caller's order, the offsets monotone and inside the buffers,
// every row the caller's. HEAT_OK or HEAT_E_SIZE.
int check_air_species_tables(int64_t n_zones, const heat_air_handlers *h, const heat_air_species *sp, const SpeciesTables &t,
                             std::string &err);

// Openings of a series (heat_openings, include/heat_amd.h). Everything heat_openings_check promises about the term itself;
// op == nullptr is none. HEAT_OK or a negative heat_status with `err` set, naming "opening i".
int check_openings(int64_t n_zones, int32_t n_channels, const heat_openings *op, std::string &err);
// The tables of k_series_openings (one lane per opening, the caller's order), packed into one int32 and one f64 buffer (one
// upload each). A NULL channel list is -1 here, a NULL coefficient list zeros.
enum OpeningI32 : int { OP_ZONE_A, OP_ZONE_B, OP_TEMP_CHAN, OP_WIND_CHAN, OP_FRAC_CHAN, OP_OUT_CHAN, kOpeningI32Rows };
enum OpeningF64 : int { OP_AREA, OP_CW, OP_CS, OP_CA, OP_C0, kOpeningF64Rows };
struct OpeningTables {
    int64_t n_openings = 0;
    std::vector<int32_t> i32;  // [kOpeningI32Rows][n]
    std::vector<double> f64;   // [kOpeningF64Rows][n]
    const int32_t *list(int a) const { return i32.data() + a * n_openings; }
    const double *real(int a) const { return f64.data() + a * n_openings; }
};
// (of a term that passed check_openings)
void build_opening_tables(const heat_openings *op, OpeningTables &t);
// The tables against the caller's lists (used by the host-only check): every row the caller's, bit for bit, every zone and
// channel a lane would index inside [0, n_zones) / [0, n_channels), and every derived channel written by one opening and read
// by none. HEAT_OK or HEAT_E_SIZE.
int check_opening_tables(int64_t n_zones, int32_t n_channels, const heat_openings *op, const OpeningTables &t, std::string &err);

// Controllers of a series (heat_controllers, include/heat_amd.h). Everything heat_controllers_check promises about the term
// itself and about it beside the openings `op` (nullable; it has passed check_openings); ct == nullptr is none. m: the
// surfaces' node counts and the zones. HEAT_OK or a negative heat_status with `err` set, naming "controller i".
int check_controllers(const SeriesModel &m, int32_t n_channels, const heat_openings *op, const heat_controllers *ct, std::string &err);
// The tables of k_series_controllers (one lane per controller, the caller's order), packed into one int32 and one f64 buffer
// (one upload each). A NULL list holds its neutral value here (sense_kind 0, action +1, en_chan and lim_kind -1, reals 0).
// CT_SENSE_AT / CT_LIM_AT: where the lane reads — the zone, the channel, or for kind 1 the node's index in the device's T
// buffer as `node_at` gives it (32 bits, unsigned, as the probes'), the node already resolved (-1: the last).
enum ControllerI32 : int { CT_SENSE_KIND, CT_SENSE_AT, CT_SET_CHAN, CT_ACTION, CT_EN_CHAN, CT_LIM_KIND, CT_LIM_AT, CT_OUT_CHAN, kControllerI32Rows };
enum ControllerF64 : int { CT_KP, CT_KI, CT_BIAS, CT_OUT_LO, CT_OUT_HI, CT_LIM_HI, CT_LIM_LO, kControllerF64Rows };
struct ControllerTables {
    int64_t n_controllers = 0;
    std::vector<int32_t> i32;  // [kControllerI32Rows][n]
    std::vector<double> f64;   // [kControllerF64Rows][n]
    const int32_t *list(int a) const { return i32.data() + a * n_controllers; }
    const double *real(int a) const { return f64.data() + a * n_controllers; }
};
// (of a term that passed check_controllers) node_at(surface, node): the index of that node in the T buffer
void build_controller_tables(const SeriesModel &m, const heat_controllers *ct, const std::function<uint32_t(int64_t, int)> &node_at,
                             ControllerTables &t);
// The tables against the caller's lists (used by the host-only check): every row the caller's, every zone, channel and node
// index a lane would use inside [0, n_zones) / [0, n_channels) / [0, n_nodes), and every derived channel written by one
// controller and read by none. HEAT_OK or HEAT_E_SIZE.
int check_controller_tables(const SeriesModel &m, int32_t n_channels, int64_t n_nodes, const heat_controllers *ct, const ControllerTables &t,
                            std::string &err);

// Air networks of a series (heat_air_networks, include/heat_amd.h). Everything heat_air_networks_check promises about the term
// itself and about it beside the openings `op` and the controllers `ct` (nullable; they have passed their checks);
// nw == nullptr is none. HEAT_OK or a negative heat_status with `err` set, naming "network w", "node i" or "link l".
int check_air_networks(int64_t n_zones, int32_t n_channels, const heat_openings *op, const heat_controllers *ct, const heat_air_networks *nw,
                       std::string &err);
// The tables of k_series_networks<W> (one lane per node, W = 8, 16, 32 or 64 lanes per network by its node count). The networks
// are SORTED by width class (stable: the caller's order within a class) and their nodes follow them; class c (W = 8 << c)
// holds the sorted networks [class_start[c], class_start[c + 1]). NW_ID / ND_ID: the caller's number of a sorted network or
// node — the index the outputs and the state go through. ND_INC0 / ND_INC_N: the node's incident links in `inc`, ascending
// link number (the order in which its balance is summed). The links stay in the caller's order; LK_LA / LK_LB: the local
// numbers of their nodes within the network (LK_LB -1: outside). A NULL list holds its neutral value (a channel -1, a gain 1,
// gh 0). LK_S_LIN = sqrt(p_lin), formed here once.
enum NetworkNetI32 : int { NW_ID, NW_N, NW_NODE0, NW_MAX_ITER, kNetworkNetI32Rows };
enum NetworkNetF64 : int { NW_TOL, NW_G_MIN, kNetworkNetF64Rows };
enum NetworkNodeI32 : int { ND_ID, ND_ZONE, ND_SRC_CHAN, ND_INC0, ND_INC_N, kNetworkNodeI32Rows };
enum NetworkLinkI32 : int { LK_ZONE_A, LK_ZONE_B, LK_LA, LK_LB, LK_TEMP_CHAN, LK_WP_CHAN, LK_FRAC_CHAN, LK_OUT_AB, LK_OUT_BA, kNetworkLinkI32Rows };
enum NetworkLinkF64 : int { LK_C, LK_GH, LK_P_LIN, LK_S_LIN, LK_WP_GAIN, kNetworkLinkF64Rows };
constexpr int kNetworkClasses = 4;
constexpr int kNetworkMaxNodes = 64;
struct NetworkTables {
    int64_t n_networks = 0, n_nodes = 0, n_links = 0;
    int32_t class_start[kNetworkClasses + 1] = {0, 0, 0, 0, 0};
    std::vector<int32_t> net_i32;   // [kNetworkNetI32Rows][n_networks], sorted
    std::vector<double> net_f64;    // [kNetworkNetF64Rows][n_networks], sorted
    std::vector<int32_t> node_i32;  // [kNetworkNodeI32Rows][n_nodes], sorted
    std::vector<double> node_f64;   // [n_nodes] src_gain, sorted
    std::vector<int32_t> inc;       // the incident links of every sorted node
    std::vector<int32_t> link_i32;  // [kNetworkLinkI32Rows][n_links], the caller's order
    std::vector<double> link_f64;   // [kNetworkLinkF64Rows][n_links]
    const int32_t *net(int a) const { return net_i32.data() + a * n_networks; }
    const int32_t *node(int a) const { return node_i32.data() + a * n_nodes; }
    const int32_t *link(int a) const { return link_i32.data() + a * n_links; }
    const double *link_real(int a) const { return link_f64.data() + a * n_links; }
};
// (of a term that passed check_air_networks)
void build_network_tables(const heat_air_networks *nw, NetworkTables &t);
// The tables against the caller's lists (used by the host-only check): the classes a partition of the networks with every
// network inside its width, the nodes and networks permutations, every zone, channel, link and local node number a lane would
// use inside its array, every incidence list ascending and of links that touch its node. HEAT_OK or HEAT_E_SIZE.
int check_network_tables(int64_t n_zones, int32_t n_channels, const heat_air_networks *nw, const NetworkTables &t, std::string &err);

// Ideal loads of a series (heat_ideal_loads, include/heat_amd.h). Everything heat_ideal_loads_check promises about the loads
// themselves; il == nullptr is none. HEAT_OK or a negative heat_status with `err` set, naming "ideal load i".
// load_of_zone (nullable): [n_zones], the load of every zone or -1 — the table k_zone_update_ideal looks its zone up in.
int check_ideal_loads(int64_t n_zones, int32_t n_channels, const heat_ideal_loads *il, std::string &err,
                      std::vector<int32_t> *load_of_zone = nullptr);

// Sky of a series (heat_sky, include/heat_amd.h). Everything heat_sky_check promises about the sky itself; sky == nullptr is
// none. s has passed check_series. HEAT_OK or a negative heat_status with `err` set, naming "surface s".
// any_bits (nullable): the OR of every mode byte — 0: the series launches nothing for the sky.
int check_sky(int64_t n_surfaces, const heat_series *s, const heat_sky *sky, std::string &err, unsigned *any_bits = nullptr);
// The struct heat_batch_march_series_call takes: it is there, of this library's size, and names a series.
int check_series_call(const heat_series_call *call, std::string &err);
// The anisotropic sky of a series (heat_sky_aniso), behind check_sky, check_solar_gains and check_shades: what the bands and
// the coefficient table need of the other terms, and every band a consumer reads.
int check_sky_aniso(int64_t n_surfaces, const heat_series *s, const heat_sky *sky, const heat_solar_gains *g, const heat_shades *sh,
                    const heat_sky_aniso *an, std::string &err);

// Solar gains of a series (heat_solar_gains, include/heat_amd.h). Everything heat_solar_gains_check promises about the
// gains themselves; g == nullptr is none. s has passed check_series and sky check_sky. HEAT_OK or a negative heat_status
// with `err` set, naming "aperture a" or "entry i".
int check_solar_gains(int64_t n_surfaces, const heat_series *s, const heat_sky *sky, const heat_solar_gains *g, std::string &err);
// The tables of k_series_solar_gains (one lane per receiver). The receivers are the sides that have entries, in device
// record order (side * S + device surface); slice q holds receivers [64 q, 64 q + 64) and as many rows as its longest
// receiver has entries, row i of all 64 lanes contiguous (sliced ELL): element slice_off[q] + 64 i + lane. A receiver's
// entries stand in the caller's order; what is left of a lane's column is padding, aperture -1. The layout does not enter
// the bits: a receiver's sum is one lane's sequential chain, whatever the slice width.
constexpr int kGainSlice = 64;
struct SolarGainTables {
    std::vector<uint32_t> rec;       // [n_receivers] side * S + device surface, ascending
    std::vector<int64_t> slice_off;  // [n_slices + 1] in elements, multiples of kGainSlice
    std::vector<int32_t> ap;         // [slice_off.back()] aperture, -1: padding
    std::vector<double> share;       // [slice_off.back()][2]: en_beam, en_diffuse (0 where padding)
};
// (of gains that passed check_solar_gains; dev_of: caller's surface -> device surface, nullptr: the caller's own order)
void build_solar_gain_tables(int64_t n_surfaces, const int32_t *dev_of, const heat_solar_gains *g, SolarGainTables &t);
// The tables against the caller's lists (used by the host-only check): every entry present exactly once, the caller's
// order kept inside a receiver, every offset inside the buffers. HEAT_OK or HEAT_E_SIZE.
int check_solar_gain_tables(int64_t n_surfaces, const int32_t *dev_of, const heat_solar_gains *g, const SolarGainTables &t,
                            std::string &err);

// Shades of a series (heat_shades, include/heat_amd.h). Everything heat_shades_check promises about the shades themselves;
// sh == nullptr is none. s has passed check_series, sky check_sky and g check_solar_gains. HEAT_OK or a negative heat_status
// with `err` set, naming "shade j", "horizon p", "surface s" or "aperture a".
int check_shades(int64_t n_surfaces, const heat_series *s, const heat_sky *sky, const heat_solar_gains *g, const heat_shades *sh,
                 std::string &err);
// The table of k_series_shading (one lane per shade): the shade's geometry as a structure of arrays in one f64 buffer, row a
// of all shades contiguous — a NULL diffuse_factor / ground_factor is ones here — and the horizon numbers (-1 where
// sh_horizon is NULL). The rows: layout.hpp, ShadeRow.
struct ShadeTables {
    std::vector<double> f64;       // [kShadeRows][n_shades]
    std::vector<int32_t> horizon;  // [n_shades]
};
// (of shades that passed check_shades)
void build_shade_tables(const heat_shades *sh, ShadeTables &t);

// Blinds of a series (heat_blinds, include/heat_amd.h). Everything heat_blinds_check promises about the blinds themselves;
// bl == nullptr is none. s has passed check_series and sh check_shades. HEAT_OK or a negative heat_status with `err` set,
// naming "blind i".
int check_blinds(int64_t n_zones, const heat_series *s, const heat_shades *sh, const heat_blinds *bl, std::string &err);
// The tables of k_series_blinds (one lane per SHADE): the blind of every shade (-1: none) and the blinds as structures of
// arrays in the caller's blind order, row a of all blinds contiguous. What the rule does not read is neutral here: a NULL
// pos_chan / zone / enable_chan is -1, set_chan is -1 and the half band 0 where the blind has no zone, the thresholds are 0
// where the blind is scheduled. The half band is band / 2, the one operation the header gives it.
enum BlindI32 : int { BL_POS_CHAN, BL_ZONE, BL_SET_CHAN, BL_ENABLE_CHAN, kBlindI32Rows };
enum BlindF64 : int { BL_BEAM, BL_DIFFUSE, BL_GROUND, BL_IRR_CLOSE, BL_IRR_OPEN, BL_HALF_BAND, kBlindF64Rows };
struct BlindTables {
    std::vector<int32_t> blind_of_shade;  // [n_shades]
    std::vector<int32_t> i32;             // [kBlindI32Rows][n_blinds]
    std::vector<double> f64;              // [kBlindF64Rows][n_blinds]
};
// (of blinds that passed check_blinds)
void build_blind_tables(int64_t n_shades, const heat_blinds *bl, BlindTables &t);
// The tables against the caller's lists (used by the host-only check): every blind on its shade and no other shade taken,
// every row of the caller's values. HEAT_OK or HEAT_E_SIZE.
int check_blind_tables(int64_t n_shades, const heat_blinds *bl, const BlindTables &t, std::string &err);

// Comfort of a series (heat_comfort, include/heat_amd.h). Everything heat_comfort_check promises about the term itself;
// c == nullptr is none. s has passed check_series. HEAT_OK or a negative heat_status with `err` set, naming
// "comfort sensor i" or "comfort entry j".
int check_comfort(int64_t n_surfaces, int64_t n_zones, const heat_series *s, const heat_comfort *c, std::string &err);
// The tables of k_series_comfort (one lane per sensor) and k_series_control_T (one lane per zone): the entries stably sorted
// by sensor (a counting sort: the caller's order survives inside a sensor) with CSR offsets, each entry's face as an index
// into the node buffer and its weight; the sensors' rows in the caller's order (a NULL air_weight is 0.5 here, a NULL channel
// list -1); the control sensor of every zone, -1 for none.
enum ComfortI32 : int { CF_ZONE, CF_OCC_CHAN, CF_LO_CHAN, CF_HI_CHAN, kComfortI32Rows };
struct ComfortTables {
    std::vector<int32_t> off;         // [n_sensors + 1]
    std::vector<uint32_t> face;       // [n_entries]
    std::vector<double> weight;       // [n_entries]
    std::vector<int32_t> orig;        // [n_entries] the caller's number of the entry (host side only: the check reads it)
    std::vector<int32_t> i32;         // [kComfortI32Rows][n_sensors]
    std::vector<double> air_weight;   // [n_sensors]
    std::vector<int32_t> ctl_sensor;  // [n_zones]
    bool any_control = false;
};
// (of a term that passed check_comfort) The node buffer's layout is a batch's: node_tile_base / node_geom in the caller's
// surface order (Plan). Without one (node_tile_base == nullptr: the host-only check) a face stands as the caller's state
// slot, first_node_slot[surface] (+ node_count[surface] - 1 for the last node).
void build_comfort_tables(int64_t n_zones, const heat_comfort *c, const int64_t *node_tile_base, const int32_t *node_geom,
                          const int64_t *first_node_slot, const int64_t *node_count, ComfortTables &t);
// The tables against the caller's lists (used by the host-only check): every entry present exactly once in its sensor's
// range and in the caller's order, the offsets monotone, every row the caller's, every zone's control sensor the caller's.
int check_comfort_tables(int64_t n_zones, const heat_comfort *c, const ComfortTables &t, std::string &err);

// Room radiation of a series (heat_room_radiation, include/heat_amd.h). Everything heat_room_radiation_check promises about
// the radiation itself; rr == nullptr is none. s has passed check_series and sky check_sky. HEAT_OK or a negative heat_status
// with `err` set, naming "receiver r" or "entry i".
int check_room_radiation(int64_t n_surfaces, const heat_series *s, const heat_sky *sky, const heat_room_radiation *rr, std::string &err);
// The tables of k_series_emission (one lane per distinct emitter side) and k_series_room_radiation (one lane per receiver).
// The entries are sorted by receiver into CSR ranges — a counting sort, stable: the caller's order survives inside a
// receiver — and the emitter sides they name are deduplicated into a compact list, ascending by side * n_surfaces + surface
// in the CALLER's numbering (the batch turns a key into the face node's place in the T buffer). src of an entry: the number
// of its emitter in that list, or ~channel (negative) for a channel entry.
struct RoomRadiationTables {
    std::vector<int32_t> off;      // [n_receivers + 1] entries of receiver r: [off[r], off[r + 1])
    std::vector<int32_t> src;      // [n_entries] >= 0: emitter number; < 0: ~en_chan
    std::vector<double> factor;    // [n_entries]
    std::vector<int64_t> emitter;  // [n_emitters] side * n_surfaces + surface, strictly ascending
};
// (of radiation that passed check_room_radiation)
void build_room_radiation_tables(int64_t n_surfaces, const heat_room_radiation *rr, RoomRadiationTables &t);
// The tables against the caller's lists (used by the host-only check): every entry present exactly once in its receiver's
// range, the caller's order kept, every emitter in the list once and named by an entry, every index inside its array.
// HEAT_OK or HEAT_E_SIZE.
int check_room_radiation_tables(int64_t n_surfaces, const heat_room_radiation *rr, const RoomRadiationTables &t, std::string &err);

// Ambient temperatures after creation (heat_batch_set_ambient, heat_ambient_drive; include/heat_amd.h). kind[0] / kind[1]:
// the descriptor's front_kind / back_kind in the CALLER's numbering (the batch keeps a copy). The sides of a list: n < 0, a
// NULL array with n > 0, a side byte above 1 -> HEAT_E_INVALID_ARG; a surface out of range, a side that is not Ambient, the
// same (surface, side) twice -> HEAT_E_SIZE; `what` ("entry", "ambient side") names the element in the message.
int check_ambient_sides(int64_t n_surfaces, const int32_t *const kind[2], int64_t n, const int64_t *surface, const uint8_t *side,
                        const char *what, std::string &err);
// Everything heat_ambient_check promises about the drive itself; a == nullptr is none. s has passed check_series. HEAT_OK or a
// negative heat_status with `err` set, naming "ambient side i".
int check_ambient(int64_t n_surfaces, const int32_t *const kind[2], int64_t n_zones, const heat_series *s, const heat_ambient_drive *a,
                  std::string &err);
// The tables of k_series_ambient (one lane per listed side), shared by the setter and the drive: the side's device record
// side * n_surfaces + dev_of[surface] (dev_of == nullptr: the identity), and for a FRONT whose surface's BACK is Ambient as
// well that back record, n_surfaces + dev_of[surface], whose `forced` slot carries the front's ambient temperature
// (layout.hpp, SideConst) — kNoAmbientPeer (layout.hpp) otherwise.
struct AmbientTables {
    std::vector<uint32_t> rec;   // [n]
    std::vector<uint32_t> peer;  // [n]
};
// (of sides that passed check_ambient_sides)
void build_ambient_tables(int64_t n_surfaces, const int32_t *dev_of, const int32_t *const kind[2], int64_t n, const int64_t *surface,
                          const uint8_t *side, AmbientTables &t);
// The tables against the caller's lists (used by the host-only check): every record inside [0, 2 n_surfaces), of an Ambient
// side, named once, and the peer exactly where the rule puts one. HEAT_OK or HEAT_E_SIZE.
int check_ambient_tables(int64_t n_surfaces, const int32_t *dev_of, const int32_t *const kind[2], int64_t n, const int64_t *surface,
                         const uint8_t *side, const AmbientTables &t, std::string &err);

// Report of a series (heat_series_report, include/heat_amd.h). Everything heat_series_report_check promises about the
// report itself; r == nullptr is no report. l has passed check_zone_loads. HEAT_OK or a negative
// heat_status with `err` set, naming "group g" or "group entry i".
// resolved (nullable): what every group entry is, in the caller's order.
struct ResolvedSlot {
    int32_t kind, node;
    int64_t index;
};
int check_series_report(SlotResolver &res, const heat_zone_loads *l, const heat_series_report *r, std::string &err,
                        std::vector<ResolvedSlot> *resolved = nullptr);
// The tables of k_series_groups. A group of at most kGroupRowEntries entries is ONE segment reduced by a 16-lane row; a
// larger one is cut into segments of kGroupSegment entries (the last one shorter), one wavefront each. Both constants are
// part of the result's bits — the order of a group's summation follows from its own entry count and keys alone — and so
// are fixed here, not derived from the device. Inside a group the entries are sorted by `key` (where the entry lives on the
// device: neighbouring entries are neighbouring records where the layout allows), ties by weight: the caller's order of
// the entries does not enter the result.
constexpr int kGroupSegment = 1024;
constexpr int kGroupRowEntries = 64;
struct GroupTables {
    std::vector<uint64_t> key;      // [n_entries], group-major, sorted inside a group
    std::vector<double> weight;     // [n_entries] in the same order; empty: all ones
    std::vector<uint32_t> wave_seg; // [n_wave][3]: first entry, end entry, index of the segment's partial sum
    std::vector<uint32_t> row_seg;  // [n_row][3]: the same, segments a 16-lane row reduces
    std::vector<uint32_t> part_off; // [n_groups + 1]: a group's partial sums, in segment order (none: an empty group)
};
// (of a report that passed check_series_report; key[i]: the device-order key of the caller's entry i)
void build_group_tables(int64_t n_groups, const int64_t *offset, const double *weight, const uint64_t *key, GroupTables &t);
// Internal consistency of the tables against the report's offsets (used by the host-only check): HEAT_OK or HEAT_E_SIZE.
int check_group_tables(int64_t n_groups, const int64_t *offset, const GroupTables &t, std::string &err);

// Zone-connected clusters (model.rs:556-590: surfaces exchange heat only through the zones they face): cluster id
// per surface (-1: faces no zone) and per zone, ids dense in [0, n_clusters).
void find_clusters(const heat_batch_desc *d, std::vector<int32_t> &cluster_of_surface,
                   std::vector<int32_t> &cluster_of_zone, int32_t &n_clusters);

// The message heat_last_error() returns (per thread).
std::string &last_error();

// heat_partition (include/heat_amd.h): rank of every surface, whole clusters kept together.
int partition_surfaces(const heat_batch_desc *d, int32_t n_ranks, int32_t *rank_of_surface, int64_t *n_shared_zones,
                       std::string &err);

// heat_batch_create_shard: the descriptor of the surfaces of one rank, with the arrays it points into.
struct ShardDesc {
    heat_batch_desc desc;
    std::vector<int64_t> original_index;  // surface q of the shard is surface original_index[q] of the model
    void build(const heat_batch_desc *d, const int32_t *rank_of_surface, int32_t rank);

  private:
    std::vector<int64_t> node_offset, i64[9];
    std::vector<double> mass, uvalue, front_alpha, back_alpha, f64[12];
    std::vector<int32_t> seg_cavity, i32[4];
};

}  // namespace heat
