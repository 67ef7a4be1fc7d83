// batch.hpp — private to batch.hip (the march engine) and series.hip (the series driver): the batch itself, the error and
// device-buffer helpers both use, and the engine functions the series driver may call. That list is the interface between
// the two: beside it the series driver calls only the public C ABI (heat_batch_synchronize).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is loaded at run time (heat_batch_comm_init), never linked

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/heat_amd.h"
#include "kernels.hpp"
#include "layout.hpp"
#include "hostpool.hpp"
#include "plan.hpp"

namespace heat {

inline int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    heat::last_error() = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(HEAT_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        release();
        n = count;
        if (count == 0) return hipSuccess;
        return hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T));
    }
    hipError_t upload(const std::vector<T> &h) {
        hipError_t e = alloc(h.size());
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t zeros(size_t count) {
        hipError_t e = alloc(count);
        if (e != hipSuccess || count == 0) return e;
        // (the batch's streams do not wait for the null stream — hipStreamNonBlocking —: the fill must be over before
        // any of them may touch the buffer. Found by tools/fuzz.py: the teams' exchange areas, allocated with the first team
        // launch, were still being zeroed while the members published into them.)
        e = hipMemset(p, 0, count * sizeof(T));
        if (e != hipSuccess) return e;
        return hipStreamSynchronize(nullptr);
    }
};

// A weather record as the kernels read it (heat_batch_set_weather and the series' schedules lay out the same records).
inline StepWeather to_step_weather(const heat_weather &w) {
    return StepWeather{w.dry_bulb, std::sqrt(w.wind_speed), std::sin(w.wind_direction), std::cos(w.wind_direction)};
}

}  // namespace heat

using namespace heat;  // (heat_batch is the C ABI's type, so it stands outside the namespace its members' types come from)

// The batch. What the series driver (series.hip) may touch of it — a term that needs another field adds it to this list:
//   reads   sizes and layout: n_surf, n_zones, n_sites, n_ranks, weather_cap, sl, direct_runs, dt; the host tables h_orig_of,
//           h_dev_of, h_kind, h_site, h_node_tile_base, h_node_geom, h_node_count, h_first_slot, h_out_slots, h_zone_slot_h;
//           the thread pool `pool`; the stream `stream`
//   hands to its kernels (the device buffers, never resized or freed by the driver): d_T, d_state, d_zone_T, d_zone_a0,
//           d_zone_b0, d_zone_vol, d_side_const, d_side_alpha, d_side_dyn, d_side_out, d_site, d_weather, d_step, d_flags
//   writes  resolver (made by the first series, kept), n_weather (the sub-timesteps of the step, as heat_batch_set_weather does)
// Everything else — tiles, workgroup lists, teams, graphs, timing, the collective — is the engine's alone.
struct heat_batch {
    int device = 0;
    int n_cu = 256;  // compute units of `device` (sizes the persistent grids and the fused launches' room)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // Independent surface classes run on side streams between a fork and a join event (captured into
    // the sub-timestep graph as parallel branches).
    static constexpr int kSideStreams = 3;
    hipStream_t side[kSideStreams] = {nullptr, nullptr, nullptr};
    hipStream_t fused_stream = nullptr;  // the cluster-resident march when other surfaces are streamed beside it
    hipEvent_t ev_fork = nullptr, ev_join[kSideStreams] = {nullptr, nullptr, nullptr};
    int n_ranks = 1, rank = 0;
    bool use_graph = false;

    int64_t n_surf = 0, n_zones = 0, n_state = 0, n_nodes = 0, n_cav = 0;
    double dt = 0;
    int64_t algorithmic_bytes = 0;
    int64_t class_counts[5] = {0, 0, 0, 0, 0};  // M4, M8, M16, small, general
    int64_t n_palette = 0;                      // surfaces whose constants are in palette form

    // layout
    int64_t n_fused_surfaces = 0;
    int n_stream_tiles[kNumFast] = {};  // tiles marched one sub-timestep per launch; the fused workgroups' tiles follow
    // cluster-resident march: workgroups per class, in two width groups (<= 4 tiles, <= 8 tiles)
    // workgroup lists per class: index = width group (0: <= 4 wavefronts, 1: <= 8) + 2 * mixed (small-surface tiles too)
    std::vector<FusedBlock> h_fblocks[kNumFast][4];
    DevBuf<FusedBlock> d_fblocks[kNumFast][4];
    // teams of workgroups (clusters larger than one workgroup; layout.hpp, FusedSuper)
    std::vector<FusedBlock> h_team_blocks[kNumFast], h_team_blocks0[kNumFast];
    std::vector<FusedSuper> h_team_supers[kNumFast];
    DevBuf<FusedBlock> d_team_blocks[kNumFast];
    DevBuf<FusedSuper> d_team_supers[kNumFast];
    DevBuf<uint32_t> d_team_zinfo;
    DevBuf<unsigned long long> d_xbuf;  // the teams' exchange areas (allocated with the first team launch)
    int xbuf_teams = 0;                 // teams the exchange areas are sized for
    uint32_t team_epoch = 0;            // launches so far: names the granules of a launch (tag_base)
    bool any_teams = false;
    DevBuf<unsigned int> d_fqueue;      // work-queue counters of the fused launches: one per list, never reset ...
    unsigned int fqueue_base[kNumFast * 4] = {};  // ... the tickets the list's launches so far have drawn (FusedArgs::queue_base)
    DevBuf<int32_t> d_fzones, d_fzone_eoff;
    DevBuf<uint16_t> d_fslots;
    DevBuf<double> d_side_area;
    DevBuf<int16_t> d_side_lzone;
    // the plan as made at create time (heat_batch_set_shared_zones derives the current one from it: a workgroup
    // that owns a zone shared with another rank is demoted — its tiles and zones are streamed, so that the zone
    // exchange can happen every sub-timestep)
    std::vector<FastTile> h_tiles0[kNumFast];
    std::vector<FusedBlock> h_fblocks0[kNumFast][4];
    int n_stream_tiles0[kNumFast] = {};
    std::vector<int32_t> h_fzones;      // global zone of fused-zone index i (FusedBlock::first_zone + j)
    DevBuf<int32_t> d_zlist_stream;     // sharded: touched zones that no fused workgroup owns (shared ones first)
    int n_touched_stream = 0;
    std::vector<int32_t> h_zone_block;  // zone -> fused workgroup (global number) or -1
    DevBuf<int32_t> d_stream_zones;     // zones whose balance is done by k_zones (not owned by a fused workgroup)
    int n_stream_zones = 0;
    bool any_fused = false;
    hipEvent_t ev_fused = nullptr;
    hipEvent_t ev_staged = nullptr;  // the H2D copies of a march call's weather / zone terms have run
    bool staged = false;
    int n_fast_tiles[kNumFast] = {};
    DevBuf<FastTile> d_fast_tiles[kNumFast];
    std::vector<FastTile> h_tiles_cur[kNumFast];  // the tile lists as they are on the device now
    // Unified streamed lists (k_surfaces_stream): the palette-form fast classes and the cavity-free small surfaces in
    // one tile list. [0]: the streamed tiles only (beside a cluster-resident march), [1]: every tile.
    DevBuf<FastTile> d_ulist[2];
    int n_ulist[2] = {0, 0};
    // ... in three parts, one per variant of the kernel (kernels.hip: 16 nodes per lane | 8 / 4 nodes per lane and small
    // surfaces | tiles with no-mass chunks other than facings), launched back to back: [part] = first tile, tiles
    int ulist_part[2][kStreamVariants][2] = {};
    bool capturing = false;         // a stream capture of the batch's stream is under way (enqueue_surfaces does not fork then)
    bool host_zones_stale = false;  // the device has marched since the caller's state last received the zone temperatures
    unsigned int sweep_parity = 0;  // enqueue_surfaces: direction of the next streamed sweep (zig-zag)
    unsigned int fused_parity = 0;  // enqueue_fused: direction of the next cluster-resident launch
    bool class_has_chunks[kNumFast] = {};  // the class holds tiles with such chunks: its own launch takes the NM = 2 variant
    bool in_ulist[2][kNumFast] = {};
    bool small_in_ulist[2] = {false, false};
    bool smallcav_in_ulist[2] = {false, false};  // the double glazing (small surfaces with a gas cavity) as well
    DevBuf<unsigned long long> d_ucount;  // no-mass pass counters of the unified lists: [list][tile]
    size_t ucount_stride = 0;
    int n_gen_tiles = 0;    // tiles in the general layout: [0, n_small_tiles) small, the rest catch-all
    int n_small_tiles = 0;      // small tiles, cavity-free ones first
    int n_small_plain_tiles = 0;
    int n_smallcav_stream_tiles = 0;  // streamed small-with-cavity tiles; the fused workgroups' small tiles follow them
    int n_smallcav_stream_tiles0 = 0;
    std::vector<GeneralTile> h_gen_tiles0;
    std::vector<GeneralTile> h_gen_tiles_cur;  // as on the device now
    size_t nm_count_base[kNumFast + 1] = {};
    DevBuf<GeneralTile> d_gen_tiles;
    int64_t gen_base = 0;     // first node slot of the general group
    int64_t node_slots = 0;   // total node slots incl. padding

    DevBuf<double> d_T, d_V, d_U, d_alpha_f, d_alpha_b, d_mass, d_scratch;
    DevBuf<int32_t> d_cav_idx;
    DevBuf<int32_t> d_cavref;  // CAV fast classes: 4 ints per device surface
    DevBuf<uint8_t> d_cls;   // palette class bytes (PAL fast classes)
    DevBuf<double> d_pal;    // palettes, na.pal_stride doubles per device surface
    DevBuf<CavityDev> d_cavs;

    DevBuf<int32_t> d_meta;        // node count per device surface (upload/download kernels)
    DevBuf<SideConst> d_side_const;  // [2 * S]: front records, then back records
    DevBuf<double> d_side_alpha;     // [2 * S]: factor applied to the solar irradiance at upload (layout.hpp, SideDyn)
    DevBuf<SideDyn> d_side_dyn;      // [2 * S]
    DevBuf<SideOut> d_side_out;      // [2 * S]
    DevBuf<double> d_hs_fix;         // [2 * S] or empty
    DevBuf<int64_t> d_first_slot, d_slots;  // d_slots: 8 arrays of n_surf
    DevBuf<int64_t> d_zone_slot, d_zone_off;
    DevBuf<ZoneEntry> d_zone_entries;
    int zone_rows = 0;  // k_zones gives a zone a row of 16 lanes (few walls per zone) instead of a wavefront
    DevBuf<ZoneContrib> d_zone_contrib;  // [zone entries], written by the surface kernels
    DevBuf<double> d_zone_vol, d_zone_T, d_zone_a0, d_zone_b0, d_partial;
    double *partial_ptr = nullptr;  // where step_surfaces writes (a, b): d_partial or caller memory
    // sharded batches (heat_batch_set_shared_zones)
    bool shared_set = false;
    int n_shared = 0, n_touched = 0;
    DevBuf<int32_t> d_zlist, d_slot_of, d_shared_zone;
    std::vector<int64_t> h_orig_of;  // device surface -> surface of the caller's descriptor
    // series march: where a surface's nodes sit in d_T (plan.hpp, node_slot_index; caller's surface order), and the
    // caller's slots resolved to what the device keeps there (built with the first series that probes)
    std::vector<int64_t> h_node_tile_base;
    std::vector<int32_t> h_node_geom;
    std::vector<int32_t> h_dev_of;  // surface of the caller's descriptor -> device surface
    std::vector<int32_t> h_kind[2];  // the descriptor's front_kind / back_kind, caller's numbering (heat_batch_set_ambient, heat_ambient_drive)
    SlotResolver *resolver = nullptr;
    int64_t fail_index = -1;         // where the last reported numerical failure happened first (heat_batch_failed_surface)
    int32_t fail_kind = 0;
    std::vector<uint8_t> h_touched;
    // Zones this batch finishes itself (unless they are shared with another rank): every zone on a single GPU; on a
    // sharded batch the zones its surfaces face plus the zones NO rank faces that fall to it (z % n_ranks == rank) —
    // such a zone still follows its a0 / b0 terms (heaters, infiltration: model.rs:410-423).
    std::vector<uint8_t> h_owned;
    // library-owned collective (heat_batch_comm_init): RCCL communicator + the gathered partial blocks
    ncclComm_t comm = nullptr;
    DevBuf<double> d_gathered;  // [n_ranks][2][n_shared]
    DevBuf<double> d_state;
    DevBuf<StepWeather> d_weather;
    DevBuf<int> d_step, d_flags;
    int *h_flags = nullptr;  // pinned: the flags as of the last heat_batch_synchronize
    DevBuf<unsigned long long> d_nomass_iters;

    StepWeather *h_weather = nullptr;  // pinned
    double *h_zone_ab = nullptr;       // pinned, [2][n_zones]
    size_t weather_cap = 0;            // records per site (sa.wstride)
    int n_weather = 0;
    // weather sites (heat_batch_create_sites): h_weather / d_weather hold n_sites x weather_cap records, site-major
    int32_t n_sites = 1;
    DevBuf<int32_t> d_site;            // [S] site of every device surface (layout.hpp, SideArrays::site)
    std::vector<int32_t> h_site;       // its host copy (empty for a single-site batch): a shade's site is resolved on the host

    // heat_batch_march on a caller-owned state: compact transfers through pinned staging, host gathers / scatters
    // on a thread pool ("Data at the boundary")
    std::vector<int64_t> h_in_slots;   // [4][S] in device surface order: solar_f, solar_b, ir_f, ir_b
    std::vector<int64_t> h_node_off;   // [S + 1] node offsets in the caller's surface order
    DevBuf<double> d_compact;          // inputs [4 S + Z]; outputs [N nodes | 4 S scalars | Z zones]
    DevBuf<int64_t> d_compact_off;     // per device surface: where its nodes go in the compact output
    DevBuf<int32_t> d_orig_of32;
    double *h_pin = nullptr;           // pinned staging
    size_t pin_doubles = 0;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copy[2] = {nullptr, nullptr};
    std::vector<std::pair<int64_t, int64_t>> out_chunks;  // surface ranges of the node part, a staging half each
    HostPool *pool = nullptr;
    // Runs of the state in which EVERY slot is an output of this path or an input it was just handed (the reference's
    // layout: one run over all surface blocks, surface_trait.rs:223-378). heat_batch_march copies them from the state
    // mirror straight into the caller's array — no staging, no host scatter. Empty: the layout is not of that kind.
    std::vector<std::pair<int64_t, int64_t>> direct_runs;

    // host copies for download (original surface order)
    std::vector<int64_t> h_first_slot, h_node_count, h_out_slots[4], h_zone_slot_h;
    std::vector<double> h_stage;

    SideArrays sa{};
    NodeArrays na{};
    SlotArrays sl{};

    // graph
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;

    // timing
    bool timing = false;
    int timing_every = 1;      // heat_batch_set_timing(k > 1): only every k-th streamed march call records events
    int64_t timing_calls = 0;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    struct EvTriple { hipEvent_t e0, e1, e2; };            // one streamed sub-timestep: start, surfaces done, zones done
    struct EvPair { hipEvent_t e0, e1; int n_sub; };       // one cluster-resident launch over n_sub sub-timesteps
    std::vector<EvTriple> ev_triples;
    std::vector<EvPair> ev_fused_pairs;
    bool fusion_on = true;     // heat_batch_options::no_fusion / heat_batch_set_fusion
    int64_t n_fused_launches = 0;  // cluster-resident launches issued since creation (introspection)
    bool ideal_resident_on = false;   // heat_batch_set_ideal_resident: an ideal series keeps its resident clusters resident
    bool ideal_reason_traced = false; // (HEAT_AMD_TRACE: why the opt-in has no effect on this batch, said once)
    bool graph_fused = false;  // what the captured sub-timestep graph leaves out
    int graph_subs = 0;        // sub-timesteps one replay of the captured graph runs
    int graph_recaptures = 0;  // captures forced by a change of the calls' length

    ~heat_batch();
};

namespace heat {

// Makes the batch's device the calling thread's current one.
int select_device(heat_batch *b);
// Room for the weather of a march call of n_sub sub-timesteps, in pinned and in device memory.
int grow_weather(heat_batch *b, int32_t n_sub);
// The body of a march call: n_sub sub-timesteps from the weather, zone terms and counter already on the device.
int march_body(heat_batch *b, int32_t n_sub);
// The same with the zone update under the ideal-loads rule: every sub-timestep streamed, or — heat_batch_set_ideal_resident
// on an eligible batch, fusion on, a call long enough — the resident clusters resident (the IDEAL instantiations host the
// rule) and the rest streamed beside or behind them. The engine decides; the caller hands the loads' view over.
int march_body_ideal(heat_batch *b, int32_t n_sub, const IdealLoadsDev &ild);

}  // namespace heat
