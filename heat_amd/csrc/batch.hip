// batch.hip — implementation of the C ABI declared in include/heat_amd.h.
//
// heat_batch_create re-orders the caller's surfaces into the lane-blocked device layout
// (layout.hpp), heat_batch_march* drive the kernels of kernels.hip on one HIP stream.
// There is no CPU fallback: every entry point that computes needs a HIP device and fails
// with HEAT_E_DEVICE otherwise.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is loaded at run time (heat_batch_comm_init), never linked

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/heat_amd.h"
#include "kernels.hpp"
#include "layout.hpp"
#include "hostpool.hpp"
#include "plan.hpp"

using namespace heat;

namespace {

int fail(int code, const char *fmt, ...) {
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

// RCCL entry points, bound at run time so that single-GPU users need no RCCL at all. In a process that
// has loaded torch, "librccl.so.1" resolves to the copy torch already mapped (same soname).
struct Rccl {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

struct RcclState {
    Rccl r;
    std::string err;
    std::once_flag once;
};
RcclState &rccl_state() {
    static RcclState st;
    return st;
}
const std::string &rccl_error() { return rccl_state().err; }

Rccl *rccl() {
    RcclState &st = rccl_state();
    std::call_once(st.once, [&st] {
        Rccl &r = st.r;
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        void *h = nullptr;
        for (const char *n : names) {
            h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
            const char *e = dlerror();  // (read once: dlerror() clears the message)
            st.err = e ? e : "dlopen failed";
        }
        if (!h) return;
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
        r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(h, "ncclAllGather"));
        r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(h, "ncclAllReduce"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
        if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.AllReduce || !r.GetErrorString) {
            st.err = "symbols missing";
            dlclose(h);
            return;
        }
        st.err.clear();
        r.handle = h;
    });
    return st.r.handle ? &st.r : nullptr;
}

#define RCCL_TRY(R, expr)                                                                             \
    do {                                                                                              \
        ncclResult_t e_ = (expr);                                                                     \
        if (e_ != ncclSuccess)                                                                        \
            return fail(HEAT_E_COMM, "%s failed: %s (%s:%d)", #expr, (R)->GetErrorString(e_), __FILE__, __LINE__); \
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

// march calls of fewer sub-timesteps are streamed (large batches). Round 3, 1 M x 32 on one MI355X (tools/short_calls.py): a
// cluster-resident call costs 155 us + 59 us per sub-timestep, the same batch streamed 198-212 us per sub-timestep (its layout
// pads every cluster to whole wavefronts; laid out for streaming alone it takes 166-188) -> resident from two sub-timesteps on.
static const int kFusedMinSubsteps = getenv("HEAT_AMD_FUSED_MIN") ? atoi(getenv("HEAT_AMD_FUSED_MIN")) : 2;
// ... and from which a list of more blocks than the chip holds is marched by persistent workgroups (enqueue_fused)
constexpr int kFusedQueueMinSubsteps = 12;

}  // namespace

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
    bool graph_fused = false;  // what the captured sub-timestep graph leaves out
    int graph_subs = 0;        // sub-timesteps one replay of the captured graph runs
    int graph_recaptures = 0;  // captures forced by a change of the calls' length

    ~heat_batch() {
        if (comm) {
            Rccl *r = rccl();
            if (r) (void)r->CommDestroy(comm);
        }
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        if (graph) (void)hipGraphDestroy(graph);
        for (auto e : ev_pool) (void)hipEventDestroy(e);
        delete pool;
        delete resolver;
        if (h_pin) (void)hipHostFree(h_pin);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        for (auto e : ev_copy) if (e) (void)hipEventDestroy(e);
        if (h_weather) (void)hipHostFree(h_weather);
        if (h_zone_ab) (void)hipHostFree(h_zone_ab);
        if (h_flags) (void)hipHostFree(h_flags);
        for (int i = 0; i < kSideStreams; i++) {
            if (ev_join[i]) (void)hipEventDestroy(ev_join[i]);
            if (side[i]) (void)hipStreamDestroy(side[i]);
        }
        if (fused_stream) (void)hipStreamDestroy(fused_stream);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_fused) (void)hipEventDestroy(ev_fused);
        if (ev_staged) (void)hipEventDestroy(ev_staged);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

int flags_to_status(int f) {
    if (f & FLAG_NAN_HS) return fail(HEAT_N_NAN_HS, "NaN convection coefficient (reference: surface.rs:704)");
    if (f & FLAG_NAN_NOMASS) return fail(HEAT_N_NAN_NOMASS, "NaN error in the no-mass loop (reference: surface.rs:850)");
    if (f & FLAG_NAN_ZONE) return fail(HEAT_N_NAN_ZONE, "NaN zone temperature (reference: model.rs:417)");
    if (f & FLAG_UNREACHABLE) return fail(HEAT_N_UNREACHABLE, "unreachable!() branch taken (NaN input)");
    if (f & FLAG_EXCHANGE)
        return fail(HEAT_E_DEVICE, "cluster-resident march: a workgroup of a team gave up waiting for another member's zone sums "
                                   "(the state of this march call is not to be used)");
    return HEAT_OK;
}

int rebuild_unified(heat_batch *b);

int build(heat_batch *b, const heat_batch_desc *d, const heat_batch_options &opt, int32_t n_sites = 1,
          const int32_t *site_of_surface = nullptr) {
    // Classification, clustering, tiling and packing are host-only work (plan.cpp); here the plan is uploaded.
    Plan p;
    {
        std::string err;
        const int rc = make_plan(d, opt, p, err, n_sites, site_of_surface);
        if (rc) return fail(rc, "%s", err.c_str());
    }
    b->n_sites = p.n_sites;
    if (!p.dev_site.empty()) HIP_TRY(b->d_site.upload(p.dev_site));
    b->h_site = p.dev_site;
    const int64_t S = p.n_surf, Z = p.n_zones;
    b->n_surf = S;
    b->n_zones = Z;
    b->n_state = p.n_state;
    b->n_cav = p.n_cav;
    b->dt = p.dt;
    b->n_nodes = p.n_nodes;
    b->algorithmic_bytes = p.algorithmic_bytes;
    for (int i = 0; i < 5; i++) b->class_counts[i] = p.class_counts[i];
    b->n_palette = p.n_palette;
    b->n_fused_surfaces = p.n_fused_surfaces;
    b->gen_base = p.gen_base;
    b->node_slots = p.node_slots;
    b->n_small_tiles = p.n_small_tiles;
    b->n_small_plain_tiles = p.n_small_plain_tiles;
    b->n_smallcav_stream_tiles = b->n_smallcav_stream_tiles0 = p.n_smallcav_stream_tiles;
    b->any_fused = p.any_fused;
    b->h_zone_block = p.zone_block;
    b->h_gen_tiles0 = b->h_gen_tiles_cur = p.gen_tiles;
    for (int c = 0; c < kNumFast; c++) {
        for (int g2 = 0; g2 < 4; g2++) {
            b->h_fblocks[c][g2] = b->h_fblocks0[c][g2] = p.fblocks[c][g2];
            HIP_TRY(b->d_fblocks[c][g2].upload(p.fblocks[c][g2]));
        }
        b->h_team_blocks[c] = b->h_team_blocks0[c] = p.team_blocks[c];
        b->h_team_supers[c] = p.team_supers[c];
        b->any_teams = b->any_teams || !p.team_supers[c].empty();
        HIP_TRY(b->d_team_blocks[c].upload(p.team_blocks[c]));
        HIP_TRY(b->d_team_supers[c].upload(p.team_supers[c]));
        b->h_tiles0[c] = b->h_tiles_cur[c] = p.fast_tiles[c];
        b->n_stream_tiles[c] = b->n_stream_tiles0[c] = p.n_stream_tiles[c];
        b->n_fast_tiles[c] = (int)p.fast_tiles[c].size();
        HIP_TRY(b->d_fast_tiles[c].upload(p.fast_tiles[c]));
        b->nm_count_base[c] = p.nm_count_base[c];
    }
    b->nm_count_base[kNumFast] = p.nm_count_base[kNumFast];
    b->h_fzones = p.fzones;
    HIP_TRY(b->d_fzones.upload(p.fzones));
    HIP_TRY(b->d_fzone_eoff.upload(p.fzone_eoff));
    HIP_TRY(b->d_team_zinfo.upload(p.team_zinfo));
    HIP_TRY(b->d_fslots.upload(p.fslots));
    HIP_TRY(b->d_side_area.upload(p.side_area));
    HIP_TRY(b->d_side_lzone.upload(p.side_lzone));
    b->h_touched = p.touched;
    b->h_owned = p.touched;
    if (b->n_ranks <= 1) b->h_owned.assign(Z, 1);
    {
        std::vector<int32_t> sz;
        for (int64_t z = 0; z < Z; z++) if (b->h_zone_block[z] < 0 && b->h_owned[z]) sz.push_back((int32_t)z);
        b->n_stream_zones = (int)sz.size();
        HIP_TRY(b->d_stream_zones.upload(sz));
    }

    // ---- host copies used by download ----
    b->h_first_slot = std::move(p.h_first_slot);
    b->h_node_count = std::move(p.h_node_count);
    for (int a = 0; a < 4; a++) b->h_out_slots[a] = std::move(p.h_out_slots[a]);
    b->h_zone_slot_h = p.zone_slot;

    // ---- upload ----
    b->n_gen_tiles = (int)p.gen_tiles.size();
    HIP_TRY(b->d_gen_tiles.upload(p.gen_tiles));
    HIP_TRY(b->d_T.zeros(p.node_slots));
    HIP_TRY(b->d_V.upload(p.V));
    HIP_TRY(b->d_U.upload(p.U));
    HIP_TRY(b->d_alpha_f.upload(p.alpha_f));
    HIP_TRY(b->d_alpha_b.upload(p.alpha_b));
    HIP_TRY(b->d_mass.upload(p.mass));
    HIP_TRY(b->d_cav_idx.upload(p.cav_idx));
    HIP_TRY(b->d_cavref.upload(p.cavref));
    HIP_TRY(b->d_cls.upload(p.cls));
    HIP_TRY(b->d_pal.upload(p.pal));
    HIP_TRY(b->d_scratch.alloc(p.scratch_slots));
    HIP_TRY(b->d_cavs.upload(p.cavs));
    HIP_TRY(b->d_meta.upload(p.meta));
    HIP_TRY(b->d_side_const.upload(p.side));
    HIP_TRY(b->d_side_alpha.upload(p.side_alpha));
    const bool has_fix = !p.hs_fix.empty();
    if (has_fix) HIP_TRY(b->d_hs_fix.upload(p.hs_fix));
    HIP_TRY(b->d_side_dyn.zeros(2 * S));
    HIP_TRY(b->d_side_out.zeros(2 * S));
    HIP_TRY(b->d_first_slot.upload(p.first_slot));
    HIP_TRY(b->d_slots.upload(p.slots));
    HIP_TRY(b->d_zone_slot.upload(p.zone_slot));
    HIP_TRY(b->d_zone_vol.upload(p.zone_vol));
    HIP_TRY(b->d_zone_off.upload(p.zone_off));
    HIP_TRY(b->d_zone_entries.upload(p.zone_entries));
    {
        static const char *rows_env = getenv("HEAT_AMD_ZONE_ROWS");  // measurement: 0 / 1 overrides the rule
        b->zone_rows = rows_env ? atoi(rows_env) : ((int64_t)p.zone_entries.size() <= 24 * (int64_t)b->n_zones);
    }
    HIP_TRY(b->d_zone_contrib.zeros(p.zone_entries.size()));
    HIP_TRY(b->d_zone_T.zeros(std::max<int64_t>(Z, 1)));  // (never empty: the surface kernels gather unconditionally)
    HIP_TRY(b->d_zone_a0.zeros(Z));
    HIP_TRY(b->d_zone_b0.zeros(Z));
    HIP_TRY(b->d_partial.zeros(2 * Z));
    b->partial_ptr = b->d_partial.p;
    HIP_TRY(b->d_state.zeros(p.n_state));
    HIP_TRY(b->d_step.zeros(2));  // [0] sub-timestep of the running march call, [1] its last one
    HIP_TRY(b->d_flags.zeros(4));  // [0] kinds OR-ed, [2..3] first failing surface / zone (report_failure, kernels.hip)
    HIP_TRY(hipMemset(b->d_flags.p + 2, 0xff, 2 * sizeof(int)));
    HIP_TRY(hipStreamSynchronize(nullptr));
    b->h_orig_of = p.orig_of;
    b->h_node_tile_base = std::move(p.node_tile_base);
    b->h_node_geom = std::move(p.node_geom);
    b->h_dev_of.assign(p.dev_of.begin(), p.dev_of.end());
    b->h_kind[0].assign(d->front_kind, d->front_kind + S);
    b->h_kind[1].assign(d->back_kind, d->back_kind + S);
    HIP_TRY(b->d_nomass_iters.zeros(p.n_nm_counters));
    if (Z > 0) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&b->h_zone_ab), 2 * Z * sizeof(double)));

    {
        const int rc = rebuild_unified(b);
        if (rc) return rc;
    }
    {   // compact transfers
        b->h_in_slots.assign(p.slots.begin() + 4 * S, p.slots.end());
        b->h_node_off.assign(d->node_offset, d->node_offset + S + 1);
        if (S == 0) b->h_node_off.assign(1, 0);
        std::vector<int64_t> coff(S);
        std::vector<int32_t> oo(S);
        for (int64_t dd = 0; dd < S; dd++) {
            coff[dd] = d->node_offset[p.orig_of[dd]];
            oo[dd] = (int32_t)p.orig_of[dd];
        }
        HIP_TRY(b->d_compact_off.upload(coff));
        HIP_TRY(b->d_orig_of32.upload(oo));
        const size_t n_out = (size_t)p.n_nodes + 4 * (size_t)S + (size_t)Z;
        HIP_TRY(b->d_compact.alloc(std::max<size_t>(n_out, 1)));
        // staging: two halves of up to 4 M doubles (32 MB) — a copy fills one while the pool empties the other; the
        // inputs (4 S + Z) and the scalar outputs (4 S + Z) must fit one buffer as a whole
        static const int stage_mb = getenv("HEAT_AMD_STAGE_MB") ? atoi(getenv("HEAT_AMD_STAGE_MB")) : 32;  // per half
        const size_t kHalf = (size_t)std::max(stage_mb, 1) << 17;
        b->pin_doubles = std::max<size_t>(2 * std::min<size_t>(kHalf, std::max<size_t>((size_t)p.n_nodes, 1)), 4 * (size_t)S + (size_t)Z + 1);
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&b->h_pin), b->pin_doubles * sizeof(double)));
        const size_t half = b->pin_doubles / 2;
        b->out_chunks.clear();
        for (int64_t s0 = 0; s0 < S;) {
            int64_t s1 = s0 + 1;
            while (s1 < S && (size_t)(d->node_offset[s1 + 1] - d->node_offset[s0]) <= half) s1++;
            b->out_chunks.push_back({s0, s1});
            s0 = s1;
        }
        HIP_TRY(hipStreamCreateWithFlags(&b->copy_stream, hipStreamNonBlocking));
        for (auto &e : b->ev_copy) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        {   // direct runs (see heat_batch::direct_runs)
            static const bool no_direct = getenv("HEAT_AMD_NO_DIRECT_DOWNLOAD") != nullptr;
            std::vector<uint8_t> mask((size_t)p.n_state, 0);
            const int64_t *sc[8] = {d->hs_front_slot, d->hs_back_slot, d->flow_front_slot, d->flow_back_slot,
                                    d->solar_front_slot, d->solar_back_slot, d->ir_front_slot, d->ir_back_slot};
            for (int64_t s = 0; s < S; s++) {
                const int64_t n = d->node_offset[s + 1] - d->node_offset[s];
                memset(&mask[d->first_node_slot[s]], 1, (size_t)n);
                for (int a = 0; a < 8; a++) mask[sc[a][s]] = 1;
            }
            int64_t covered = 0, wanted = 0;
            for (int64_t i = 0; i < p.n_state;) {
                if (!mask[i]) { i++; continue; }
                int64_t e = i;
                while (e < p.n_state && mask[e]) e++;
                wanted += e - i;
                if (e - i >= 65536) { b->direct_runs.push_back({i, e}); covered += e - i; }
                i = e;
            }
            // all of the surfaces' slots in a few long runs, or nothing (the staged path serves any layout)
            if (no_direct || covered != wanted || b->direct_runs.size() > 64) b->direct_runs.clear();
        }
        static const int n_env = getenv("HEAT_AMD_HOST_THREADS") ? atoi(getenv("HEAT_AMD_HOST_THREADS")) : 0;
        const int hw = (int)std::thread::hardware_concurrency();
        b->pool = new HostPool(n_env > 0 ? n_env : std::max(1, std::min(hw > 0 ? hw : 8, S > 20000 ? 16 : 1)));
        if (getenv("HEAT_AMD_TRACE")) fprintf(stderr, "heat_amd: %d host threads, staging 2 x %zu MB, %zu node pieces\n", b->pool->size(), half * 8 >> 20, b->out_chunks.size());
    }

    // ---- argument bundles ----
    SideArrays &sa = b->sa;
    sa.sc = b->d_side_const.p;
    sa.dyn = b->d_side_dyn.p;
    sa.out = b->d_side_out.p;
    sa.hs_fix = has_fix ? b->d_hs_fix.p : nullptr;
    sa.zc = b->d_zone_contrib.p;
    sa.S = (int32_t)S;
    sa.wstride = 0;
    sa.site = b->n_sites > 1 ? b->d_site.p : nullptr;
    NodeArrays &na = b->na;
    na.T = b->d_T.p; na.V = b->d_V.p; na.U = b->d_U.p;
    na.cls = b->d_cls.p; na.pal = b->d_pal.p;
    na.pal_stride = p.pal_stride;
    na.pal_ubase = p.pal_ubase;
    na.cavref = b->d_cavref.p; na.cavs = b->d_cavs.p;
    na.alpha_f = b->d_alpha_f.p; na.alpha_b = b->d_alpha_b.p; na.cav = b->d_cav_idx.p; na.mass = b->d_mass.p;
    SlotArrays &sl = b->sl;
    const int64_t *sp = b->d_slots.p;
    sl.hs_f = sp; sl.hs_b = sp + S; sl.flow_f = sp + 2 * S; sl.flow_b = sp + 3 * S;
    sl.solar_f = sp + 4 * S; sl.solar_b = sp + 5 * S; sl.ir_f = sp + 6 * S; sl.ir_b = sp + 7 * S;
    // (every upload and fill above went through the null stream; the batch's streams do not wait for it)
    HIP_TRY(hipDeviceSynchronize());
    return HEAT_OK;
}

int select_device(heat_batch *b) {
    HIP_TRY(hipSetDevice(b->device));
    return HEAT_OK;
}

// A persistent wavefront w of a k_surfaces_stream launch walks tiles[w], tiles[w + n_waves], ... — round after round. The
// tiles of a part differ in length by an order of magnitude (a window whose no-mass loop re-evaluates its gas cavity
// every pass against eight massive nodes per lane), so the list is laid out in rounds such that every wavefront's share
// takes about the same time: longest-processing-time-first over the wavefronts, each wavefront's tiles longest first,
// empty tiles (G = 0: a wavefront skips them at once) where a wavefront has fewer tiles than rounds.
std::vector<FastTile> balanced_rounds(const std::vector<FastTile> &tiles, const std::vector<float> &cost, int n_waves) {
    const size_t n = tiles.size();
    if (n_waves <= 0 || n <= (size_t)n_waves) return tiles;  // a tile per wavefront at most: nothing to balance
    std::vector<int32_t> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return cost[a] > cost[b]; });
    // least-loaded wavefront first (a binary heap of (load, wavefront))
    std::vector<std::pair<float, int32_t>> heap(n_waves);
    for (int w = 0; w < n_waves; w++) heap[w] = {0.f, w};
    auto later = [](const std::pair<float, int32_t> &a, const std::pair<float, int32_t> &b) {
        return a.first > b.first || (a.first == b.first && a.second > b.second);
    };
    std::make_heap(heap.begin(), heap.end(), later);
    std::vector<std::vector<int32_t>> mine(n_waves);
    for (int32_t t : order) {
        std::pop_heap(heap.begin(), heap.end(), later);
        auto &top = heap.back();
        mine[top.second].push_back(t);
        top.first += cost[t];
        std::push_heap(heap.begin(), heap.end(), later);
    }
    size_t rounds = 0;
    for (const auto &m : mine) rounds = std::max(rounds, m.size());
    FastTile empty;
    empty.node_base = 0;
    empty.surf_base = 0;
    empty.k = (int16_t)(kStreamKindSmall << kStreamKindShift);  // (a small tile of no surface: every lane leaves at once)
    empty.G = 0;
    std::vector<FastTile> out(rounds * (size_t)n_waves, empty);
    for (int w = 0; w < n_waves; w++)
        for (size_t r = 0; r < mine[w].size(); r++) out[r * (size_t)n_waves + w] = tiles[mine[w][r]];
    return out;
}

// The unified streamed tile lists from the current per-class lists (create time, and again when
// heat_batch_set_shared_zones has moved tiles between the fused workgroups and the streamed part).
int rebuild_unified(heat_batch *b) {
    static const bool off = getenv("HEAT_AMD_NO_UNIFIED") != nullptr;  // measurement: one launch per class as before
    // (16 nodes per lane with facings or cavities keep launches of their own: one wavefront per SIMD)
    auto eligible = [](int c) { return kFastPAL[c] && !(kFastM[c] == 16 && (kFastNM[c] || kFastCAV[c])); };
    static const bool cav_off = getenv("HEAT_AMD_NO_UNIFIED_CAV") != nullptr;  // measurement: round 2's two launches
    size_t cap = (size_t)b->n_small_tiles;
    for (int c = 0; c < kNumFast; c++) if (eligible(c)) cap += b->h_tiles_cur[c].size();
    // (the balanced parts are padded to whole rounds: two rounds more than the tiles need, per part, bound the padding)
    const int waves_light = b->n_cu * 3 * 4, waves_cav = b->n_cu * 2 * 4;  // persistent grids of the light / cavity variants
    cap += 2 * (size_t)(waves_light + waves_cav) + 2 * (size_t)(waves_light + waves_cav);
    if (b->d_ucount.n == 0) {
        b->ucount_stride = std::max<size_t>(cap, 1);
        HIP_TRY(b->d_ucount.zeros(2 * b->ucount_stride));
    }
    const int ns = b->n_small_plain_tiles;
    for (int c = 0; c < kNumFast; c++) {
        b->class_has_chunks[c] = false;
        for (const FastTile &ft : b->h_tiles_cur[c]) b->class_has_chunks[c] = b->class_has_chunks[c] || (ft.k & kTileChunkyBit) != 0;
    }
    for (int v = 0; v < 2; v++) {
        // the four parts (kernels.hip, k_surfaces_stream): wide | light | chunks | cavities
        std::vector<FastTile> part[kStreamVariants];
        int n_classes = 0, n_cav_classes = 0;
        // double glazing: the streamed small tiles with cavities ([plain | streamed with cavities | fused workgroups' ...])
        const int nsc = cav_off ? 0 : (v ? b->n_small_tiles - b->n_small_plain_tiles : b->n_smallcav_stream_tiles);
        for (int j = 0; j < nsc; j++) {  // (first in their part: the longest tiles)
            const GeneralTile &g = b->h_gen_tiles_cur[b->n_small_plain_tiles + j];
            FastTile ft;
            ft.node_base = g.node_base;
            ft.surf_base = g.surf_base;
            ft.k = (int16_t)(kStreamKindSmall << kStreamKindShift);
            ft.G = (int16_t)g.G;
            part[3].push_back(ft);
        }
        for (int mi = 2; mi >= 0; mi--)  // 16 nodes per lane first: the heaviest tiles lead
            for (int c = mi * 6; c < mi * 6 + 6; c++) {
                if (!eligible(c) || (kFastCAV[c] && cav_off)) continue;
                if (kFastCAV[c]) {
                    const int n = v ? b->n_fast_tiles[c] : b->n_stream_tiles[c];
                    n_cav_classes += n > 0;
                    for (int t = 0; t < n; t++) {
                        FastTile ft = b->h_tiles_cur[c][t];
                        ft.k = (int16_t)((ft.k & (0x1ff | kTileMixedBit | kTileChunkyBit)) | (mi << kStreamKindShift) | (kFastNM[c] ? kStreamNmBit : 0));
                        part[3].push_back(ft);
                    }
                    continue;
                }
                const int n = v ? b->n_fast_tiles[c] : b->n_stream_tiles[c];
                n_classes += n > 0;
                for (int t = 0; t < n; t++) {
                    FastTile ft = b->h_tiles_cur[c][t];
                    const bool chunks = (ft.k & kTileChunkyBit) != 0;
                    ft.k = (int16_t)((ft.k & (0x1ff | kTileMixedBit | kTileChunkyBit)) | (mi << kStreamKindShift) | (kFastNM[c] ? kStreamNmBit : 0));
                    part[mi == 2 ? 0 : (chunks ? 2 : 1)].push_back(ft);
                }
            }
        // worth it when it replaces two launches or more (a class on its own keeps its own persistent kernel)
        const bool use = !off && (n_classes + (ns > 0)) >= 2;
        // ... and the cavity part when it replaces two launches (glazing + walls with cavities, or two such classes)
        const bool use_cav = !off && !cav_off && (n_cav_classes + (nsc > 0)) >= 2;
        b->n_ulist[v] = 0;
        for (int c = 0; c < kNumFast; c++) b->in_ulist[v][c] = eligible(c) && (kFastCAV[c] ? use_cav : use);
        b->small_in_ulist[v] = use && ns > 0;
        b->smallcav_in_ulist[v] = use_cav && nsc > 0;
        for (int q = 0; q < kStreamVariants; q++) b->ulist_part[v][q][0] = b->ulist_part[v][q][1] = 0;
        if (!use) part[0].clear(), part[1].clear(), part[2].clear();
        if (!use_cav) part[3].clear();
        if (!use && !use_cav) continue;
        // Relative tile times (measured on MI355X, 1 M ragged walls / 100 k windows + 100 k Trombe walls; only their
        // ratios matter): a tile of eight massive nodes per lane 1, with facings 2, four nodes per lane 0.7 / 1.4, a tile
        // of small surfaces 3, of double glazing 12, a tile of walls with cavities 2.5.
        static const bool balance_off = getenv("HEAT_AMD_NO_BALANCE") != nullptr;  // measurement
        auto tile_cost = [&](const FastTile &ft, bool cav) -> float {
            const int kind = (ft.k >> kStreamKindShift) & 3;
            if (kind == kStreamKindSmall) return cav ? 12.f : 3.f;
            const float base = kind == 1 ? 1.f : 0.7f;
            if (cav) return 2.5f * base;
            return (ft.k & kStreamNmBit) ? 2.f * base : base;
        };
        if (use) {  // the small surfaces join the light part
            for (int j = 0; j < ns; j++) {
                const GeneralTile &g = b->h_gen_tiles_cur[j];
                FastTile ft;
                ft.node_base = g.node_base;
                ft.surf_base = g.surf_base;
                ft.k = (int16_t)(kStreamKindSmall << kStreamKindShift);
                ft.G = (int16_t)g.G;
                part[1].push_back(ft);
            }
        }
        for (int q : {1, 3}) {
            if (balance_off || part[q].empty()) continue;
            std::vector<float> cost(part[q].size());
            for (size_t t = 0; t < part[q].size(); t++) cost[t] = tile_cost(part[q][t], q == 3);
            part[q] = balanced_rounds(part[q], cost, q == 1 ? waves_light : waves_cav);
        }
        std::vector<FastTile> all;
        for (int q = 0; q < kStreamVariants; q++) {
            b->ulist_part[v][q][0] = (int)all.size();
            b->ulist_part[v][q][1] = (int)part[q].size();
            all.insert(all.end(), part[q].begin(), part[q].end());
        }
        if (all.size() > b->ucount_stride) return fail(HEAT_E_SIZE, "unified tile list grew beyond its counters");
        b->n_ulist[v] = (int)all.size();
        HIP_TRY(b->d_ulist[v].upload(all));
    }
    return HEAT_OK;
}

// iterate_surfaces for every group (model.rs:388-408), one sub-timestep.
// streamed_only: leave out the tiles owned by the cluster-resident march (enqueue_fused marches those).
void enqueue_surfaces(heat_batch *b, int step_fixed, bool streamed_only = false) {
    int nt[kNumFast];
    for (int c = 0; c < kNumFast; c++) nt[c] = streamed_only ? b->n_stream_tiles[c] : b->n_fast_tiles[c];
    // One launch for the palette-form fast classes and the cavity-free small surfaces (k_surfaces_stream); the
    // classes it does not hold follow on their own.
    const int ul = streamed_only ? 0 : 1;
    const bool unified = b->n_ulist[ul] > 0;
    // Zig-zag sweeps: consecutive sub-timesteps walk the batch in opposite directions. A sweep streams the whole state
    // through the 256 MB memory-side cache (MI355X: Infinity Cache in front of HBM); walked in the same direction every
    // time, nothing of it is left when its turn comes again — walked back, the last quarter of a 1 GB sweep is.
    static const bool zigzag_off = getenv("HEAT_AMD_NO_ZIGZAG") != nullptr;  // measurement
    const int rev = (!zigzag_off && (b->sweep_parity++ & 1)) ? 1 : 0;
    int n_small_plain = b->n_small_plain_tiles;
    if (unified) {
        for (int c = 0; c < kNumFast; c++) if (b->in_ulist[ul][c]) nt[c] = 0;
        if (b->small_in_ulist[ul]) n_small_plain = 0;
    }
    // The classes are independent (model.rs:102-180: surfaces never read what another surface wrote in the
    // same sub-timestep): spread them over the batch's stream and its side streams so that one class's
    // tail overlaps the next class's head.
    int n_launch = 0;
    for (int c = 0; c < kNumFast; c++) n_launch += nt[c] > 0;
    // small tiles with cavities: the streamed ones come first, the fused workgroups' after them
    int n_cav_tiles = streamed_only ? b->n_smallcav_stream_tiles : b->n_small_tiles - b->n_small_plain_tiles;
    if (unified && b->smallcav_in_ulist[ul]) n_cav_tiles = 0;
    n_launch += unified;
    n_launch += n_small_plain > 0;
    n_launch += n_cav_tiles > 0;
    n_launch += b->n_gen_tiles > b->n_small_tiles;
    static const bool no_fork = getenv("HEAT_AMD_NO_FORK") != nullptr;  // measurement: every class on the batch's stream
    // (not inside a stream capture: three of the fuzzer's cases — batches without palettes, whose two or three class launches
    // were forked onto side streams inside the captured sub-timestep — ended in a hang or a crash of the process inside the
    // HIP runtime at the SECOND capture of a batch (a march call of another length); captured, the launches follow each other
    // on the batch's stream, where a graph leaves no gap between them anyway)
    const bool fork = n_launch > 1 && b->side[0] != nullptr && !no_fork && !b->capturing;
    // Exactly the side streams that get work are forked, and every forked one is joined below: inside a stream capture a
    // side stream that waits for the fork event and is never joined leaves the capture unjoined — found by tools/fuzz.py
    // as a hang or a crash of the process some captures later (batches without palettes: two or three class launches on
    // three side streams).
    const int n_side = fork ? std::min(n_launch - 1, (int)heat_batch::kSideStreams) : 0;
    int slot = 0;
    auto next_stream = [&]() -> hipStream_t {
        if (n_side == 0) return b->stream;
        const int s = slot++ % (n_side + 1);
        return s == 0 ? b->stream : b->side[s - 1];
    };
    if (n_side > 0) {
        (void)hipEventRecord(b->ev_fork, b->stream);
        for (int i = 0; i < n_side; i++) (void)hipStreamWaitEvent(b->side[i], b->ev_fork, 0);
    }
    if (unified) {
        // the parts follow each other on ONE stream (a dependency between two streams costs more than the tail of a part)
        hipStream_t us = next_stream();
        // the light part first: its wavefronts are the latency-bound ones, the wide part's tail is the shorter
        static const int order_env = getenv("HEAT_AMD_STREAM_ORDER") ? atoi(getenv("HEAT_AMD_STREAM_ORDER")) : 0;  // measurement
        const int seq[2][kStreamVariants] = {{3, 1, 2, 0}, {0, 1, 2, 3}};
        for (int qi = 0; qi < kStreamVariants; qi++) {
            // (a reversed sweep takes the parts in the opposite order too, each from its end)
            const int q = seq[order_env ? 1 : 0][rev ? kStreamVariants - 1 - qi : qi];
            const int first = b->ulist_part[ul][q][0], n = b->ulist_part[ul][q][1];
            if (n > 0)
                launch_surfaces_stream(q, b->d_ulist[ul].p + first, n, b->na, b->gen_base, b->sa, b->d_weather.p, b->d_step.p,
                                       step_fixed, b->d_zone_T.p, b->d_flags.p,
                                       b->d_ucount.p + ul * b->ucount_stride + first, b->n_cu, us, rev);
        }
    }
    // work of each class in node slots, to size the persistent grids
    double work[kNumFast], total_work = 0.0;
    for (int c = 0; c < kNumFast; c++) {
        work[c] = (double)nt[c] * kFastM[c];
        total_work += work[c];
    }
    total_work += 2.0 * b->n_gen_tiles;  // small / general tiles: a few nodes per lane
    // biggest classes first
    int order[kNumFast];
    for (int c = 0; c < kNumFast; c++) order[c] = c;
    std::sort(order, order + kNumFast, [&](int x, int y) { return nt[x] > nt[y]; });
    for (int q = 0; q < kNumFast; q++) {
        const int c = order[q];
        if (nt[c] <= 0) continue;
        launch_surfaces_fast(kFastM[c], kFastNM[c] ? (b->class_has_chunks[c] ? 2 : 1) : 0, kFastPAL[c], kFastCAV[c], work[c] / total_work,
                             b->d_fast_tiles[c].p, nt[c], b->na,
                             b->sa, b->d_weather.p, b->d_step.p, step_fixed, b->d_zone_T.p, b->d_flags.p,
                             b->d_nomass_iters.p + b->nm_count_base[c], b->n_cu, next_stream(), rev);
    }
    unsigned long long *cnt = b->d_nomass_iters.p + b->nm_count_base[kNumFast];
    if (n_small_plain > 0)
        launch_surfaces_small(0, b->d_gen_tiles.p, n_small_plain, b->na, b->gen_base, b->sa, b->d_cavs.p,
                              b->d_weather.p, b->d_step.p, step_fixed, b->d_zone_T.p, b->d_flags.p, cnt,
                              next_stream());
    if (n_cav_tiles > 0)
        launch_surfaces_small(1, b->d_gen_tiles.p + b->n_small_plain_tiles, n_cav_tiles,
                              b->na, b->gen_base, b->sa, b->d_cavs.p, b->d_weather.p, b->d_step.p, step_fixed,
                              b->d_zone_T.p, b->d_flags.p, cnt + (size_t)b->n_small_plain_tiles * kWave,
                              next_stream());
    if (b->n_gen_tiles > b->n_small_tiles)
        launch_surfaces_general(b->d_gen_tiles.p + b->n_small_tiles, b->n_gen_tiles - b->n_small_tiles, b->na,
                                b->gen_base, b->sa, b->d_cavs.p, b->d_scratch.p, b->d_weather.p, b->d_step.p,
                                step_fixed, b->d_zone_T.p, b->d_flags.p, cnt + (size_t)b->n_small_tiles * kWave,
                                next_stream());
    for (int i = 0; i < n_side; i++) {
        (void)hipEventRecord(b->ev_join[i], b->side[i]);
        (void)hipStreamWaitEvent(b->stream, b->ev_join[i], 0);
    }
}

// mode 0 / 1 / 2 as k_zones; mode 3: as mode 0 (full update, advances the step counter) but only the zones no
// fused workgroup owns (the cluster-resident march balances its own zones in LDS).
void enqueue_zones(heat_batch *b, int mode) {
    const int32_t *zl = b->d_zlist.p;
    int nl = b->n_touched;
    if (mode == 3) { zl = b->d_stream_zones.p; nl = b->n_stream_zones; }
    if (mode == 5) { mode = 3; }  // sharded batch, nothing fused in this call: every zone it owns (d_zlist), full update
    if (mode == 4) { zl = b->d_zlist_stream.p; nl = b->n_touched_stream; mode = 2; }  // sharded, beside a fused march
    launch_zones(b->d_zone_off.p, b->d_zone_entries.p, b->d_zone_contrib.p, b->d_zone_a0.p, b->d_zone_b0.p,
                 b->d_zone_vol.p, b->d_zone_T.p, b->partial_ptr, (int)b->n_zones, b->dt, b->d_step.p,
                 b->d_flags.p, mode, zl, nl, b->d_slot_of.p, b->n_shared, b->zone_rows, b->stream);
}

struct TeamShape {
    int team_size = 0, room = 0, n_teams = 0;
};

// The shape of every class's team launch for a call of n_sub sub-timesteps, and the limits of the exchange tags. A call
// the teams cannot march is refused HERE, before anything of the call is on a stream: a refusal after the plain resident
// launches (or another class's teams) had started would leave part of the batch n_sub sub-timesteps ahead of the rest.
static int team_shapes(const heat_batch *b, int n_sub, TeamShape (&shape)[kNumFast]) {
    for (int c = 0; c < kNumFast; c++) {
        const int n_super = (int)b->h_team_supers[c].size();
        if (n_super == 0) continue;
        if (n_sub > 4095) return fail(HEAT_E_INVALID_ARG, "a march call of %d sub-timesteps: the team exchange tags 4095 at most", n_sub);
        // what the chip holds of this variant, less a margin (the hardware may admit a workgroup per compute unit fewer than
        // the occupancy arithmetic says); other kernels in flight only delay a member's start, they end by themselves
        // (at most two per compute unit whatever the query says: the variants hold 171-256 registers)
        static const int team_room_env = getenv("HEAT_AMD_TEAM_ROOM") ? atoi(getenv("HEAT_AMD_TEAM_ROOM")) : 0;  // measurement
        TeamShape &ts = shape[c];
        ts.room = team_room_env > 0 ? team_room_env : b->n_cu * std::min(2, fused_team_blocks_per_cu(kFastM[c], kFastNM[c], b->na.pal_stride));
        ts.team_size = 2;
        for (const FusedSuper &su : b->h_team_supers[c]) ts.team_size = std::max(ts.team_size, (int)su.n_members);
        ts.n_teams = std::min(n_super, std::max(0, ts.room - ts.room / 8) / ts.team_size);
        if (ts.n_teams >= 1 && (n_super + ts.n_teams - 1) / ts.n_teams > 1023)
            return fail(HEAT_E_SIZE, "%d clusters for %d teams: the exchange tags 1023 rounds per launch at most", n_super, ts.n_teams);
        if (ts.n_teams < 1) return fail(HEAT_E_DEVICE, "the device holds %d workgroups of the team variant: not one team", ts.room);
    }
    return HEAT_OK;
}

// The cluster-resident march: every fused workgroup marches n_sub sub-timesteps in one launch per class.
// streamed_beside: other surfaces of the batch are streamed on the batch's stream while this launch runs.
int enqueue_fused(heat_batch *b, int n_sub, hipStream_t st, bool streamed_beside = false) {
    TeamShape team_shape[kNumFast];
    {
        const int rc = team_shapes(b, n_sub, team_shape);
        if (rc) return rc;
    }
    FusedArgs fa{};
    {   // zig-zag over march calls (see enqueue_surfaces): what the last call wrote back last is this call's first read
        static const bool zigzag_off = getenv("HEAT_AMD_NO_ZIGZAG") != nullptr;  // measurement
        fa.reverse = (!zigzag_off && (b->fused_parity++ & 1)) ? 1 : 0;
    }
    fa.zones = b->d_fzones.p;
    fa.zone_eoff = b->d_fzone_eoff.p;
    fa.slots = b->d_fslots.p;
    fa.side_area = b->d_side_area.p;
    fa.side_lzone = b->d_side_lzone.p;
    fa.a0 = b->d_zone_a0.p;
    fa.b0 = b->d_zone_b0.p;
    fa.vol = b->d_zone_vol.p;
    fa.zone_T = b->d_zone_T.p;
    fa.dt = b->dt;
    fa.n_sub = n_sub;
    fa.gen_tiles = b->d_gen_tiles.p;
    fa.gen_base = b->gen_base;
    fa.small_iters = b->d_nomass_iters.p + b->nm_count_base[kNumFast];
    // Beside an exchange loop (sharded batch with shared zones) the fused launch must not take every wavefront slot
    // of the chip: the loop's small kernels and the collective would each wait tens of microseconds for a slot
    // (measured: 27-74 us instead of 5) and become the critical path. So the launch holds a few workgroups fewer
    // than the chip has room for, and its workgroups take their FusedBlocks from a queue.
    static const int reserve_env = getenv("HEAT_AMD_FUSED_RESERVE") ? atoi(getenv("HEAT_AMD_FUSED_RESERVE")) : -1;
    const bool beside_exchange = (b->comm != nullptr && b->shared_set && b->n_shared > 0) || reserve_env >= 0 || streamed_beside;
    // share of the batch's padded nodes that is streamed beside this launch: that much of the chip is left to it
    double streamed_share = 0.0;
    if (streamed_beside) {
        double ns = 4.0 * kWave * (b->n_gen_tiles - (b->n_small_tiles - b->n_small_plain_tiles - b->n_smallcav_stream_tiles)), nf = 0.0;
        for (int c = 0; c < kNumFast; c++) {
            ns += (double)b->n_stream_tiles[c] * kFastM[c] * kWave;
            nf += (double)(b->n_fast_tiles[c] - b->n_stream_tiles[c]) * kFastM[c] * kWave;
        }
        streamed_share = ns / std::max(ns + nf, 1.0);
    }
    // A list of more blocks than the chip holds at once is marched by exactly that many workgroups, which take their
    // blocks from the same queue — in calls of kFusedQueueMinSubsteps sub-timesteps or more: a workgroup that follows
    // another into its slot costs the write-back's acknowledgement, a dispatch and the kernel arguments before its first
    // load, a workgroup that stays two barriers and the ticket's round trip; the first is the dearer one only where the
    // blocks live long (0.5 us per sub-timestep won at 20 per call, 2 lost at 2).
    // HEAT_AMD_FUSED_PERSIST (measurement, tests): the call length from which on; 0: never.
    static const int persist_env = getenv("HEAT_AMD_FUSED_PERSIST") ? atoi(getenv("HEAT_AMD_FUSED_PERSIST")) : -1;
    const int persist_min = persist_env >= 0 ? persist_env : kFusedQueueMinSubsteps;
    const bool persist = persist_min > 0 && n_sub >= persist_min;
    const int n_cu = b->n_cu;
    if (b->d_fqueue.n == 0) HIP_TRY(b->d_fqueue.zeros(kNumFast * 4));
    for (int c = 0; c < kNumFast; c++)
        for (int g2 = 0; g2 < 4; g2++) {
            const int nb = (int)b->h_fblocks[c][g2].size();
            if (nb == 0) continue;
            fa.blocks = b->d_fblocks[c][g2].p;
            fa.n_blocks = nb;
            fa.queue = nullptr;
            int grid = nb;
            if (beside_exchange || persist) {
                const int fw = (g2 & 1) ? 8 : 4;
                static const int room_env = getenv("HEAT_AMD_FUSED_ROOM") ? atoi(getenv("HEAT_AMD_FUSED_ROOM")) : 0;  // tests
                const int room = room_env > 0 ? room_env : n_cu * fused_blocks_per_cu(kFastM[c], kFastCAV[c], g2 >> 1, fw, b->na.pal_stride);
                const int reserve = !beside_exchange ? 0 : reserve_env >= 0 ? reserve_env
                                                     : std::min(room / 2, std::max(fw == 4 ? 16 : 8, (int)(room * streamed_share)));
                if (nb > room - reserve) {
                    grid = std::max(1, room - reserve);
                    fa.queue = b->d_fqueue.p + c * 4 + g2;
                    fa.queue_base = b->fqueue_base[c * 4 + g2];
                }
            }
            static const bool trace = getenv("HEAT_AMD_TRACE") != nullptr;
            if (trace)
                fprintf(stderr, "heat_amd: fused launch%s: %d workgroups for %d blocks (class %d, list %d, %d sub-timesteps)\n",
                        fa.queue ? " on the work queue" : "", grid, nb, c, g2, n_sub);
            b->n_fused_launches++;
            // (a class whose walls hold no-mass chunks other than facings marches with the variant that carries the chunk loop)
            const int nm_variant = kFastNM[c] ? ((b->class_has_chunks[c] && !(g2 >> 1) && !kFastCAV[c] && kFastM[c] <= 8) ? 2 : 1) : 0;
            HIP_TRY(launch_surfaces_fused(kFastM[c], nm_variant, kFastCAV[c], g2 >> 1, (g2 & 1) ? 8 : 4, grid, b->d_fast_tiles[c].p, b->n_fast_tiles[c],
                                          b->na, b->sa, b->d_weather.p, b->d_flags.p,
                                          b->d_nomass_iters.p + b->nm_count_base[c], fa, st));
            if (fa.queue) b->fqueue_base[c * 4 + g2] += (unsigned int)nb;  // one ticket per block marched (layout.hpp)
        }
    // Teams (clusters larger than a workgroup): n_teams x kTeamMax workgroups, ALL of them on the chip at once — a member
    // waits for the others' zone sums, so no workgroup of the launch may have to wait for a slot a waiting one holds.
    for (int c = 0; c < kNumFast; c++) {
        const int n_super = (int)b->h_team_supers[c].size();
        if (n_super == 0) continue;
        const int team_size = team_shape[c].team_size, n_teams = team_shape[c].n_teams;  // (checked before the first launch)
        if (b->xbuf_teams < n_teams) {
            HIP_TRY(b->d_xbuf.zeros((size_t)n_teams * 2 * kTeamZones * kTeamMax * 4));
            b->xbuf_teams = n_teams;
        }
        b->team_epoch++;
        if ((b->team_epoch & 1023u) == 0) {  // the 10-bit launch number wraps: no granule of the launch 1024 before may survive
            HIP_TRY(hipMemsetAsync(b->d_xbuf.p, 0, b->d_xbuf.n * sizeof(unsigned long long), st));
            b->team_epoch++;
        }
        fa.blocks = b->d_team_blocks[c].p;
        fa.n_blocks = (int)b->h_team_blocks[c].size();
        fa.queue = nullptr;
        fa.supers = b->d_team_supers[c].p;
        fa.n_super = n_super;
        fa.team_zinfo = b->d_team_zinfo.p;
        fa.xbuf = b->d_xbuf.p;
        fa.tag_base = (b->team_epoch & 1023u) << 22;
        fa.team_size = team_size;
        static const bool trace = getenv("HEAT_AMD_TRACE") != nullptr;
        if (trace)
            fprintf(stderr, "heat_amd: team launch: %d teams of %d workgroups for %d clusters (class %d, %d sub-timesteps)\n",
                    n_teams, team_size, n_super, c, n_sub);
        b->n_fused_launches++;
        HIP_TRY(launch_surfaces_fused(kFastM[c], kFastNM[c], 0, 2, 4, n_teams * team_size, b->d_fast_tiles[c].p, b->n_fast_tiles[c], b->na,
                                      b->sa, b->d_weather.p, b->d_flags.p, b->d_nomass_iters.p + b->nm_count_base[c], fa, st));
    }
    return HEAT_OK;
}

hipEvent_t next_event(heat_batch *b) {
    if (b->ev_used == b->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        b->ev_pool.push_back(e);
    }
    return b->ev_pool[b->ev_used++];
}

// A march call that forks work onto the fused stream, or swaps the partials buffer, must leave the batch consistent
// on EVERY return path: an early error return would otherwise leave the side stream unjoined (a later download that
// synchronises only the batch's stream would race with the still-running launch) or the partials pointer swapped.
struct MarchGuard {
    heat_batch *b;
    double *saved_partial;
    bool forked = false, joined = false;
    explicit MarchGuard(heat_batch *b_) : b(b_), saved_partial(b_->partial_ptr) {}
    ~MarchGuard() {
        b->partial_ptr = saved_partial;
        if (forked && !joined && b->fused_stream) (void)hipStreamSynchronize(b->fused_stream);  // error path: wait it out
    }
};

// The per-call device buffers of a series go only when the batch's stream has run dry (declared after them: destroyed first).
struct SeriesDrain {
    heat_batch *b;
    ~SeriesDrain() { (void)hipStreamSynchronize(b->stream); }
};
#define SERIES_TRY(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

template <typename T>
int series_alloc(DevBuf<T> &buf, size_t count, const char *what, const T *src = nullptr) {
    hipError_t e = buf.alloc(count);
    if (e == hipSuccess && count > 0 && src) e = hipMemcpy(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess)
        return fail(HEAT_E_DEVICE, "series march: %s (%zu bytes) on the device: %s — nothing has been marched", what, count * sizeof(T),
                    hipGetErrorString(e));
    return HEAT_OK;
}
template <typename T>
int series_upload(DevBuf<T> &buf, const T *src, size_t count, const char *what) { return series_alloc(buf, count, what, src); }
template <typename T>
int series_upload(DevBuf<T> &buf, const std::vector<T> &src, const char *what) { return series_alloc(buf, src.size(), what, src.data()); }
// An in/out array of a call: absent (nullptr: no device copy), uploaded (resume), or allocated for the device to initialise.
template <typename T>
int report_array(DevBuf<T> &buf, const T *host, size_t count, bool upload, const char *what) {
    return host ? series_alloc(buf, count, what, upload ? host : nullptr) : HEAT_OK;
}
// Back to the host behind the stream's work (and the copy that gave e, if that went well); nothing where either side holds no copy.
template <typename T>
hipError_t series_fetch(T *host, const DevBuf<T> &buf, hipStream_t st, hipError_t e = hipSuccess) {
    return e != hipSuccess || !host || !buf.p ? e : hipMemcpyAsync(host, buf.p, buf.n * sizeof(T), hipMemcpyDeviceToHost, st);
}
// Row k of a buffer of rows of n values; nullptr where the buffer is absent.
template <typename T>
T *row(const DevBuf<T> &buf, int k, int64_t n) { return buf.p ? buf.p + (size_t)k * (size_t)n : nullptr; }
// dst[d] = src[orig_of[d]]: an array over the caller's surfaces, in the device's order.
template <typename T>
void to_device_order(heat_batch *b, const T *src, T *dst) {
    const int64_t *orig_of = b->h_orig_of.data();
    b->pool->run(b->n_surf, [&](int64_t d0, int64_t d1) { for (int64_t d = d0; d < d1; d++) dst[d] = src[orig_of[d]]; });
}
// The start of a fresh run's accumulator on the device (the step numbers start at -1, written as 0xff bytes).
inline hipError_t series_fill(const DevBuf<double> &d, double v, hipStream_t st) { launch_fill_f64(d.p, (int64_t)d.n, v, st); return hipSuccess; }
inline hipError_t series_fill(const DevBuf<int64_t> &d, int64_t v, hipStream_t st) {
    return d.p ? hipMemsetAsync(d.p, v < 0 ? 0xff : 0, d.n * sizeof(int64_t), st) : hipSuccess;
}
// An in/out accumulator: the caller's array, its device copy, a fresh run's start value and the device view's field for the copy.
template <typename T>
struct Acc {
    T *host = nullptr, **view = nullptr;
    T init = 0;
    DevBuf<T> dev;
    void bind(T *h, T v, T **field) { host = h, init = v, view = field; }
    // uploaded on resume, else allocated; nothing where the caller passes no array
    int stage(size_t n, bool resume, const char *w) { const int rc = report_array(dev, host, n, resume, w); *view = dev.p; return rc; }
    hipError_t start(hipStream_t st, hipError_t e = hipSuccess) { return e != hipSuccess ? e : series_fill(dev, init, st); }
    hipError_t fetch(hipStream_t st, hipError_t e = hipSuccess) { return series_fetch(host, dev, st, e); }
};
// start() or fetch() of every accumulator of a list, in order, up to the first error
template <typename A, size_t N>
hipError_t for_each_acc(A (&acc)[N], hipError_t (A::*what)(hipStream_t, hipError_t), hipStream_t st, hipError_t e = hipSuccess) {
    for (A &a : acc) e = (a.*what)(st, e);
    return e;
}
inline StepWeather to_step_weather(const heat_weather &w) {
    return StepWeather{w.dry_bulb, std::sqrt(w.wind_speed), std::sin(w.wind_direction), std::cos(w.wind_direction)};
}

// ---- the terms of a series march: each owns its host tables (prepare: no device call), its device buffers and view (upload:
// through the null stream) and its way back (fetch: asynchronous). Declared before the call's SeriesDrain: freed after the stream ran dry. ----

// The driven inputs: channel numbers and gains per DEVICE surface, structure of arrays; the own-face bits and face nodes.
// The gain arrays serve the sky, the solar gains and the room radiation too.
struct InputsTerm {
    const double *gain[4] = {nullptr, nullptr, nullptr, nullptr};
    bool driven = false;
    std::vector<int32_t> h_chan;
    std::vector<double> h_gain[4];
    std::vector<uint8_t> h_own;
    std::vector<uint32_t> h_face;
    DevBuf<int32_t> chan;
    DevBuf<double> d_gain[4];
    DevBuf<uint8_t> own;
    DevBuf<uint32_t> face;
    SeriesInputs view{};
    // gain[a] in device order, once: for whichever term drives input a first
    void need_gain(heat_batch *b, int a) {
        if (!gain[a] || !h_gain[a].empty()) return;
        h_gain[a].resize((size_t)b->n_surf);
        to_device_order(b, gain[a], h_gain[a].data());
    }
    void prepare(heat_batch *b, const heat_series *s) {
        const int64_t S = b->n_surf;
        const int32_t *src[4] = {s->solar_front_chan, s->solar_back_chan, s->ir_front_chan, s->ir_back_chan};
        const double *g[4] = {s->solar_front_gain, s->solar_back_gain, s->ir_front_gain, s->ir_back_gain};
        bool own_any = false;
        for (int a = 0; a < 4; a++) {
            gain[a] = g[a];
            for (int64_t q = 0; src[a] && q < S && !driven; q++) driven = src[a][q] >= 0;
        }
        for (int64_t q = 0; s->ir_own_face && q < S && !own_any; q++) own_any = (s->ir_own_face[q] & 3) != 0;
        if (!driven) return;
        h_chan.assign(4 * (size_t)S, -1);
        for (int a = 0; a < 4; a++) {
            if (!src[a]) continue;
            to_device_order(b, src[a], h_chan.data() + (size_t)a * S);
            need_gain(b, a);
        }
        if (!own_any) return;
        const int64_t *orig_of = b->h_orig_of.data();
        h_own.resize((size_t)S);
        h_face.resize(2 * (size_t)S);
        b->pool->run(S, [&](int64_t d0, int64_t d1) {
            for (int64_t d = d0; d < d1; d++) {
                const int64_t q = orig_of[d];
                h_own[d] = (uint8_t)(s->ir_own_face[q] & 3);
                h_face[d] = (uint32_t)node_slot_index(b->h_node_tile_base[q], b->h_node_geom[q], 0);
                h_face[S + d] = (uint32_t)node_slot_index(b->h_node_tile_base[q], b->h_node_geom[q], (int)b->h_node_count[q] - 1);
            }
        });
    }
    int upload() {
        SERIES_TRY(series_upload(chan, h_chan, "channel numbers"));
        for (int a = 0; a < 4; a++) SERIES_TRY(series_upload(d_gain[a], h_gain[a], "gains"));
        SERIES_TRY(series_upload(own, h_own, "own-face bits"));
        SERIES_TRY(series_upload(face, h_face, "face node table"));
        view.chan = chan.p, view.own_face = own.p, view.face = face.p;
        for (int a = 0; a < 4; a++) view.gain[a] = d_gain[a].p;
        return HEAT_OK;
    }
};

// The probes: (buffer, index) of every probed slot; the trace; the record of the first failed step.
struct ProbesTerm {
    int64_t P = 0;
    std::vector<uint8_t> h_buf;
    std::vector<uint32_t> h_idx;
    DevBuf<uint8_t> buf;
    DevBuf<uint32_t> idx;
    DevBuf<int> failed;  // the step, then the flags as they were after it
    DevBuf<double> trace;
    static void place(const heat_batch *b, int kind, int64_t index, int node, uint8_t &buf, uint32_t &idx) {
        if (kind == PROBE_ZONE) {
            buf = (uint8_t)kProbeBufZone, idx = (uint32_t)index;
        } else if (kind == PROBE_NODE) {
            buf = (uint8_t)kProbeBufT, idx = (uint32_t)node_slot_index(b->h_node_tile_base[index], b->h_node_geom[index], node);
        } else {  // hs front, hs back, flow front, flow back: SideOut record side * S + d, as doubles
            const int a = kind - PROBE_HS_FRONT;
            const int64_t rec = (int64_t)(a & 1) * b->n_surf + b->h_dev_of[index];
            buf = (uint8_t)kProbeBufOut, idx = (uint32_t)(2 * rec + (a >> 1));
        }
    }
    int prepare(heat_batch *b, const heat_series *s) {
        P = s->n_probes;
        h_buf.resize((size_t)P);
        h_idx.resize((size_t)P);
        for (int64_t p = 0; p < P; p++) {
            int kind = 0, node = 0;
            int64_t index = 0;
            if (!b->resolver->resolve(s->probe_slot[p], kind, index, node)) return fail(HEAT_E_SIZE, "probe %lld: slot not resolved", (long long)p);
            place(b, kind, index, node, h_buf[p], h_idx[p]);
        }
        return HEAT_OK;
    }
    int upload(const double *host_trace, int n_steps) {
        const int fail_init[5] = {-1, 0, 0, 0, 0};
        SERIES_TRY(series_upload(buf, h_buf, "probe table"));
        SERIES_TRY(series_upload(idx, h_idx, "probe table"));
        SERIES_TRY(series_upload(failed, fail_init, 5, "failed step"));
        return host_trace ? series_alloc(trace, (size_t)n_steps * P, "trace") : HEAT_OK;
    }
    hipError_t fetch(double *host_trace, hipStream_t st) { return series_fetch(host_trace, trace, st); }
};

// The zone loads: the term lists sorted by zone with CSR offsets (plan.hpp), the mode bytes in the caller's order, the applied rows.
struct LoadsTerm {
    bool on = false;
    int64_t NT = 0;
    ZoneLoadTables zt;
    std::vector<uint8_t> h_mode;
    DevBuf<int32_t> i32;
    DevBuf<double> f64, applied;
    DevBuf<uint8_t> mode;
    ZoneLoadsDev view{};
    void prepare(const heat_batch *b, const heat_zone_loads *l) {
        on = l && (l->n_gains > 0 || l->n_flows > 0 || l->n_thermostats > 0);
        if (!on) return;
        NT = l->n_thermostats;
        build_zone_load_tables(b->n_zones, l, zt);
        h_mode.assign((size_t)NT, 0);
        if (l->th_mode) std::copy(l->th_mode, l->th_mode + NT, h_mode.begin());
    }
    int upload(const double *host_applied, int n_steps) {
        if (!on) return HEAT_OK;
        // (packed into two uploads, not thirteen: each one is an allocation and a pageable copy in the call's set-up)
        const std::vector<int32_t> *a_i32[8] = {&zt.off, &zt.gain_chan, &zt.flow_volume_chan, &zt.flow_temp_chan, &zt.th_sensor,
                                                &zt.th_heat_chan, &zt.th_cool_chan, &zt.th_orig};
        const std::vector<double> *a_f64[5] = {&zt.gain_factor, &zt.flow_volume_gain, &zt.th_heat_power, &zt.th_cool_power, &zt.th_half_band};
        const int32_t **v_i32[8] = {&view.off, &view.gain_chan, &view.flow_volume_chan, &view.flow_temp_chan, &view.th_sensor,
                                    &view.th_heat_chan, &view.th_cool_chan, &view.th_orig};
        const double **v_f64[5] = {&view.gain_factor, &view.flow_volume_gain, &view.th_heat_power, &view.th_cool_power, &view.th_half_band};
        std::vector<int32_t> h_i32;
        std::vector<double> h_f64;
        for (auto *v : a_i32) h_i32.insert(h_i32.end(), v->begin(), v->end());
        for (auto *v : a_f64) h_f64.insert(h_f64.end(), v->begin(), v->end());
        SERIES_TRY(series_upload(i32, h_i32, "zone load tables"));
        SERIES_TRY(series_upload(f64, h_f64, "zone load tables"));
        SERIES_TRY(series_upload(mode, h_mode, "thermostat modes"));
        if (host_applied) SERIES_TRY(series_alloc(applied, (size_t)n_steps * NT, "applied powers"));
        for (size_t a = 0, at = 0; a < 8; at += a_i32[a++]->size()) *v_i32[a] = i32.p + at;
        for (size_t a = 0, at = 0; a < 5; at += a_f64[a++]->size()) *v_f64[a] = f64.p + at;
        view.th_mode = mode.p;
        return HEAT_OK;
    }
    hipError_t fetch(const heat_zone_loads *l, double *host_applied, hipStream_t st) {
        return on ? series_fetch(l->th_mode, mode, st, series_fetch(host_applied, applied, st)) : hipSuccess;
    }
};

// The report (heat_series_report): the group entries sorted into device order (buffer, index) and cut into segments
// (plan.hpp), the step's group sums, the group trace, the limits (always uploaded, never fetched), the accumulators.
struct ReportTerm {
    heat_series_report *r = nullptr;
    int64_t G = 0, Q = 0;
    bool th_stats = false, q_stats = false;
    GroupTables gt;
    std::vector<uint8_t> h_gbuf;
    std::vector<uint32_t> h_gidx;
    DevBuf<uint8_t> gbuf, prev;
    DevBuf<uint32_t> gidx, seg, part_off;
    DevBuf<double> gw, part, group_trace, applied_row, lo, hi;
    Acc<double> q_f64[5], th_f64[2];   // q_min, q_max, q_sum, q_deg_below, q_deg_above; th_sum_heating, th_sum_cooling
    Acc<int64_t> q_i64[4], th_i64[3];  // q_step_min, q_step_max, q_n_below, q_n_above; th_steps_heating, th_steps_cooling, th_switches
    SeriesGroupsDev groups{};
    SeriesStatsDev stats{};
    SeriesThStatsDev th{};
    void prepare(const heat_batch *b, heat_series_report *r_, int64_t P, const std::vector<ResolvedSlot> &entry) {
        r = r_;
        Q = P;
        if (!r) return;
        const double inf = std::numeric_limits<double>::infinity();
        q_f64[0].bind(r->q_min, inf, &stats.q_min), q_f64[1].bind(r->q_max, -inf, &stats.q_max), q_f64[2].bind(r->q_sum, 0.0, &stats.q_sum);
        q_f64[3].bind(r->q_deg_below, 0.0, &stats.q_deg_below), q_f64[4].bind(r->q_deg_above, 0.0, &stats.q_deg_above);
        q_i64[0].bind(r->q_step_min, -1, &stats.q_step_min), q_i64[1].bind(r->q_step_max, -1, &stats.q_step_max);
        q_i64[2].bind(r->q_n_below, 0, &stats.q_n_below), q_i64[3].bind(r->q_n_above, 0, &stats.q_n_above);
        th_f64[0].bind(r->th_sum_heating, 0.0, &th.sum_heating), th_f64[1].bind(r->th_sum_cooling, 0.0, &th.sum_cooling);
        th_i64[0].bind(r->th_steps_heating, 0, &th.steps_heating), th_i64[1].bind(r->th_steps_cooling, 0, &th.steps_cooling);
        th_i64[2].bind(r->th_switches, 0, &th.switches);
        th_stats = th_f64[0].host || th_f64[1].host || th_i64[0].host || th_i64[1].host || th_i64[2].host;
        G = r->n_groups;
        Q = P + G;
        if (G == 0) return;
        const int64_t n_entries = r->group_offset[G];
        std::vector<uint64_t> key((size_t)n_entries);
        for (int64_t i = 0; i < n_entries; i++) {
            uint8_t buf = 0;
            uint32_t idx = 0;
            ProbesTerm::place(b, entry[(size_t)i].kind, entry[(size_t)i].index, entry[(size_t)i].node, buf, idx);
            key[(size_t)i] = (uint64_t)buf << 32 | idx;
        }
        build_group_tables(G, r->group_offset, r->group_weight, key.data(), gt);
        h_gbuf.resize((size_t)n_entries);
        h_gidx.resize((size_t)n_entries);
        for (int64_t i = 0; i < n_entries; i++) h_gbuf[(size_t)i] = (uint8_t)(gt.key[(size_t)i] >> 32), h_gidx[(size_t)i] = (uint32_t)gt.key[(size_t)i];
    }
    int upload(int n_steps, const ProbesTerm &probes, const LoadsTerm &loads) {
        if (!r) return HEAT_OK;
        const bool resume = r->resume != 0;
        const size_t n_wave = gt.wave_seg.size() / 3, n_row = gt.row_seg.size() / 3;
        std::vector<uint32_t> h_seg(gt.wave_seg);
        h_seg.insert(h_seg.end(), gt.row_seg.begin(), gt.row_seg.end());
        SERIES_TRY(series_upload(gbuf, h_gbuf, "group tables"));
        SERIES_TRY(series_upload(gidx, h_gidx, "group tables"));
        SERIES_TRY(series_upload(gw, gt.weight, "group tables"));
        SERIES_TRY(series_upload(seg, h_seg, "group tables"));
        SERIES_TRY(series_upload(part_off, gt.part_off.data(), G > 0 ? gt.part_off.size() : 0, "group tables"));
        SERIES_TRY(series_alloc(part, n_wave + n_row, "group sums"));
        SERIES_TRY(report_array(group_trace, r->group_trace, (size_t)n_steps * G, false, "group trace"));
        for (auto &a : q_f64) SERIES_TRY(a.stage((size_t)Q, resume, "statistics"));
        SERIES_TRY(report_array(lo, r->q_lo, (size_t)Q, true, "statistics"));
        SERIES_TRY(report_array(hi, r->q_hi, (size_t)Q, true, "statistics"));
        for (auto &a : q_i64) SERIES_TRY(a.stage((size_t)Q, resume, "statistics"));
        groups.buf = gbuf.p, groups.idx = gidx.p, groups.weight = gw.p, groups.part = part.p;
        groups.wave_seg = seg.p, groups.row_seg = seg.p + 3 * n_wave, groups.n_wave = (int)n_wave, groups.n_row = (int)n_row;
        stats.n_probes = probes.P, stats.n_groups = G, stats.buf = probes.buf.p, stats.idx = probes.idx.p;
        stats.part = part.p, stats.part_off = part_off.p;
        // (a limit nothing is counted against is not read)
        stats.q_lo = stats.q_n_below || stats.q_deg_below ? lo.p : nullptr;
        stats.q_hi = stats.q_n_above || stats.q_deg_above ? hi.p : nullptr;
        q_stats = Q > 0 && (stats.q_min || stats.q_max || stats.q_sum || stats.q_n_below || stats.q_deg_below || stats.q_n_above ||
                            stats.q_deg_above || group_trace.p);
        if (!th_stats) return HEAT_OK;  // (check_series_report: only with thermostats)
        for (auto &a : th_f64) SERIES_TRY(a.stage((size_t)loads.NT, resume, "thermostat statistics"));
        for (auto &a : th_i64) SERIES_TRY(a.stage((size_t)loads.NT, resume, "thermostat statistics"));
        SERIES_TRY(series_upload(prev, loads.h_mode, "thermostat modes"));
        // (the powers of the step: a row of the applied buffer, or one row of scratch where the caller takes none)
        if (!loads.applied.p && (th_f64[0].host || th_f64[1].host)) SERIES_TRY(series_alloc(applied_row, (size_t)loads.NT, "applied powers"));
        th.prev = prev.p;
        return HEAT_OK;
    }
    // start (a fresh run: min = +inf, max = -inf, steps = -1, sums and counts 0) or fetch of the accumulators
    hipError_t each(hipError_t (Acc<double>::*f64)(hipStream_t, hipError_t), hipError_t (Acc<int64_t>::*i64)(hipStream_t, hipError_t), hipStream_t st,
                    hipError_t e = hipSuccess) {
        return for_each_acc(th_i64, i64, st, for_each_acc(th_f64, f64, st, for_each_acc(q_i64, i64, st, for_each_acc(q_f64, f64, st, e))));
    }
    hipError_t start(hipStream_t st) { return r && r->resume == 0 ? each(&Acc<double>::start, &Acc<int64_t>::start, st) : hipSuccess; }
    hipError_t fetch(hipStream_t st) {
        return r ? each(&Acc<double>::fetch, &Acc<int64_t>::fetch, st, series_fetch(r->group_trace, group_trace, st)) : hipSuccess;
    }
};

// The ideal loads (heat_ideal_loads): tables, the step's setpoints and q-sums, the ideal_q rows, the accumulators.
struct IdealTerm {
    heat_ideal_loads *il = nullptr;
    int64_t NI = 0;
    std::vector<int32_t> h_i32;  // load_of_zone [Z] | heat_chan [N] | cool_chan [N]
    std::vector<double> h_cap;   // heat_cap [N] | cool_cap [N]
    DevBuf<int32_t> i32;
    DevBuf<double> cap, step, q; // step: setpoint [2][N] | qsum [N]; q: ideal_q [n_steps][N]
    Acc<double> f64[4];          // sum_heating, sum_cooling, peak_heating, peak_cooling
    Acc<int64_t> i64[4];         // step_peak_heating, step_peak_cooling, n_sat_heating, n_sat_cooling
    IdealLoadsDev view{};
    void prepare(heat_ideal_loads *il_, const std::vector<int32_t> &load_of_zone) {
        il = il_;
        NI = il ? il->n_loads : 0;
        if (NI == 0) return;
        const double inf = std::numeric_limits<double>::infinity();
        h_i32 = load_of_zone;
        h_i32.insert(h_i32.end(), il->heat_chan, il->heat_chan + NI);
        h_i32.insert(h_i32.end(), il->cool_chan, il->cool_chan + NI);
        h_cap.assign(2 * (size_t)NI, inf);
        if (il->heat_cap) std::copy(il->heat_cap, il->heat_cap + NI, h_cap.begin());
        if (il->cool_cap) std::copy(il->cool_cap, il->cool_cap + NI, h_cap.begin() + NI);
        f64[0].bind(il->sum_heating, 0.0, &view.sum_heating), f64[1].bind(il->sum_cooling, 0.0, &view.sum_cooling);
        f64[2].bind(il->peak_heating, -inf, &view.peak_heating), f64[3].bind(il->peak_cooling, inf, &view.peak_cooling);
        i64[0].bind(il->step_peak_heating, -1, &view.step_peak_heating), i64[1].bind(il->step_peak_cooling, -1, &view.step_peak_cooling);
        i64[2].bind(il->n_sat_heating, 0, &view.n_sat_heating), i64[3].bind(il->n_sat_cooling, 0, &view.n_sat_cooling);
    }
    int upload(const heat_batch *b, const double *host_q, int n_steps) {
        if (NI == 0) return HEAT_OK;
        const bool resume = il->resume != 0;
        SERIES_TRY(series_upload(i32, h_i32, "ideal load tables"));
        SERIES_TRY(series_upload(cap, h_cap, "ideal load tables"));
        SERIES_TRY(series_alloc(step, 3 * (size_t)NI, "ideal load setpoints"));
        if (host_q) SERIES_TRY(series_alloc(q, (size_t)n_steps * NI, "ideal powers"));
        for (auto &a : f64) SERIES_TRY(a.stage((size_t)NI, resume, "ideal load accumulators"));
        for (auto &a : i64) SERIES_TRY(a.stage((size_t)NI, resume, "ideal load accumulators"));
        view.n_loads = (int)NI;
        view.load_of_zone = i32.p, view.heat_chan = i32.p + b->n_zones, view.cool_chan = i32.p + b->n_zones + NI;
        view.heat_cap = cap.p, view.cool_cap = cap.p + NI, view.setpoint = step.p, view.qsum = step.p + 2 * NI;
        return HEAT_OK;
    }
    hipError_t start(hipStream_t st) {
        return NI > 0 && il->resume == 0 ? for_each_acc(i64, &Acc<int64_t>::start, st, for_each_acc(f64, &Acc<double>::start, st)) : hipSuccess;
    }
    hipError_t fetch(double *host_q, hipStream_t st) {
        return for_each_acc(i64, &Acc<int64_t>::fetch, st, for_each_acc(f64, &Acc<double>::fetch, st, series_fetch(host_q, q, st)));
    }
};

// The sky (heat_sky): the mode bytes and normals per DEVICE surface, the record table as given (the solar gains and the
// shades read it too).
struct SkyTerm {
    unsigned bits = 0;
    std::vector<uint8_t> h_mode;
    std::vector<double> h_normal;
    DevBuf<uint8_t> mode;      // [S]
    DevBuf<double> normal;     // [3][S]
    DevBuf<SkyRecord> record;  // [n_steps][n_sites]
    SeriesSky view{};
    void prepare(heat_batch *b, const heat_sky *sky, InputsTerm &in) {
        if (!bits) return;
        const int64_t S = b->n_surf;
        const int64_t *orig_of = b->h_orig_of.data();
        h_mode.resize((size_t)S);
        h_normal.resize(3 * (size_t)S);
        b->pool->run(S, [&](int64_t d0, int64_t d1) {
            for (int64_t d = d0; d < d1; d++) {
                const int64_t q = orig_of[d];
                const bool on = sky->mode[q] != 0;  // (the normals of the other surfaces are not read, not even here)
                h_mode[d] = sky->mode[q];
                h_normal[d] = on ? sky->normal_x[q] : 0.0;
                h_normal[S + d] = on ? sky->normal_y[q] : 0.0;
                h_normal[2 * S + d] = on ? sky->normal_z[q] : 0.0;
            }
        });
        for (int a = 0; a < 4; a++) if (bits >> a & 1) in.need_gain(b, a);
    }
    // records_read: by the sky's own sides, by apertures or by shades
    int upload(const heat_batch *b, const heat_series *s, const heat_sky *sky, bool records_read, const InputsTerm &in) {
        if (records_read)
            SERIES_TRY(series_upload(record, reinterpret_cast<const SkyRecord *>(sky->record), (size_t)s->n_steps * b->n_sites, "sky records"));
        if (!bits) return HEAT_OK;
        SERIES_TRY(series_upload(mode, h_mode, "sky modes"));
        SERIES_TRY(series_upload(normal, h_normal, "sky normals"));
        view.mode = mode.p, view.normal = normal.p, view.site = b->n_sites > 1 ? b->d_site.p : nullptr;
        for (int a = 0; a < 4; a++) view.gain[a] = in.d_gain[a].p;
        return HEAT_OK;
    }
};
static_assert(sizeof(SkyRecord) == sizeof(heat_sky_record) && sizeof(heat_sky_record) == 64, "SkyRecord mirrors heat_sky_record");

// The shades (heat_shades): the table as structure of arrays (plan.hpp, ShadeTables), every shade's site and horizon, the horizon
// profiles, the step's sunlit fractions, the shade numbers of the sides per DEVICE surface and of the apertures, the sunlit rows.
struct ShadesTerm {
    int64_t NS = 0;
    ShadeTables sht;
    std::vector<int32_t> h_i32, h_side;
    DevBuf<double> tab, tan2, f, sunlit;  // [kShadeRows][NS], [NH][16], [NS], [n_steps][NS]
    DevBuf<double> eff;                   // [3][NS] the effective factors k_series_blinds writes; absent without blinds
    DevBuf<int32_t> i32, side, aperture;  // site [NS] | horizon [NS], [2][S], [NA]
    SeriesShades view{};
    // what a shaded consumer reads: the step's fractions, the diffuse and the ground factors (all NULL without shades) — with
    // blinds (heat_blinds) the effective ones of the step
    ShadeFactors factors() const {
        if (eff.p) return ShadeFactors{eff.p, eff.p + (size_t)NS, eff.p + 2 * (size_t)NS};
        return ShadeFactors{f.p, tab.p + (size_t)SH_FD * NS, tab.p + (size_t)SH_FG * NS};
    }
    void prepare(heat_batch *b, const heat_shades *shades, unsigned sky_bits) {
        NS = shades ? shades->n_shades : 0;  // (a side or aperture needs a shade to refer to: none is shaded without)
        if (NS == 0) return;
        build_shade_tables(shades, sht);
        h_i32.assign(2 * (size_t)NS, 0);
        for (int64_t j = 0; j < NS; j++) {
            h_i32[j] = b->h_site.empty() ? 0 : b->h_site[b->h_dev_of[shades->sh_surface[j]]];
            h_i32[NS + j] = sht.horizon[j];
        }
        if (!(sky_bits & 3) || !(shades->front_shade || shades->back_shade)) return;
        h_side.assign(2 * (size_t)b->n_surf, -1);
        if (shades->front_shade) to_device_order(b, shades->front_shade, h_side.data());
        if (shades->back_shade) to_device_order(b, shades->back_shade, h_side.data() + b->n_surf);
    }
    int upload(const heat_shades *shades, int64_t NA, const double *host_sunlit, int n_steps, bool blinds, SkyTerm &sky) {
        if (NS == 0) return HEAT_OK;
        if (blinds) SERIES_TRY(series_alloc(eff, 3 * (size_t)NS, "effective shade factors"));
        SERIES_TRY(series_upload(tab, sht.f64, "shade table"));
        SERIES_TRY(series_upload(i32, h_i32, "shade table"));
        SERIES_TRY(series_upload(tan2, shades->horizon_tan2, 16 * (size_t)shades->n_horizons, "horizon profiles"));
        SERIES_TRY(series_alloc(f, (size_t)NS, "sunlit fractions"));
        SERIES_TRY(series_upload(side, h_side, "shade numbers"));
        if (NA > 0 && shades->aperture_shade) SERIES_TRY(series_upload(aperture, shades->aperture_shade, (size_t)NA, "shade numbers"));
        if (host_sunlit) SERIES_TRY(series_alloc(sunlit, (size_t)n_steps * NS, "sunlit fractions"));
        view.n = (int)NS, view.site = i32.p, view.horizon = i32.p + NS, view.tab = tab.p, view.tan2 = tan2.p, view.f = f.p;
        sky.view.shade = side.p, sky.view.sf = factors();
        return HEAT_OK;
    }
    hipError_t fetch(double *host_sunlit, hipStream_t st) { return series_fetch(host_sunlit, sunlit, st); }
};

// The blinds (heat_blinds): the blind of every shade and the blinds as structures of arrays (plan.hpp, BlindTables), the state
// bytes, the accumulators (uploaded where the caller passes them), the position and blind_incident rows in the caller's order.
// It reads the shades' site numbers, table and fractions and writes the shades' effective factors: uploaded behind them.
struct BlindsTerm {
    heat_blinds *blinds = nullptr;
    int64_t NL = 0;
    BlindTables blt;
    std::vector<uint8_t> h_state;
    DevBuf<int32_t> of_shade, i32;       // [NS], [kBlindI32Rows][NL]
    DevBuf<double> f64, position, incident;  // [kBlindF64Rows][NL], [n_steps][NL], [n_steps][NL]
    DevBuf<uint8_t> state;               // [NL]
    Acc<double> sum_position;
    Acc<int64_t> steps_closed, switches;
    SeriesBlinds view{};
    void prepare(heat_blinds *blinds_, int64_t NS) {
        blinds = blinds_;
        NL = blinds ? blinds->n_blinds : 0;
        if (NL == 0) return;
        build_blind_tables(NS, blinds, blt);
        h_state.assign((size_t)NL, 0);
        if (blinds->state) std::copy(blinds->state, blinds->state + NL, h_state.begin());
        sum_position.bind(blinds->sum_position, 0.0, &view.sum_position), steps_closed.bind(blinds->steps_closed, 0, &view.steps_closed);
        switches.bind(blinds->switches, 0, &view.switches);
    }
    int upload(const ShadesTerm &shades, const double *host_position, const double *host_incident, int n_steps) {
        if (NL == 0) return HEAT_OK;
        SERIES_TRY(series_upload(of_shade, blt.blind_of_shade, "blind tables"));
        SERIES_TRY(series_upload(i32, blt.i32, "blind tables"));
        SERIES_TRY(series_upload(f64, blt.f64, "blind tables"));
        SERIES_TRY(series_upload(state, h_state, "blind states"));
        SERIES_TRY(sum_position.stage((size_t)NL, true, "blind accumulators"));
        SERIES_TRY(steps_closed.stage((size_t)NL, true, "blind accumulators"));
        SERIES_TRY(switches.stage((size_t)NL, true, "blind accumulators"));
        if (host_position) SERIES_TRY(series_alloc(position, (size_t)n_steps * NL, "blind positions"));
        if (host_incident) SERIES_TRY(series_alloc(incident, (size_t)n_steps * NL, "blind irradiances"));
        view.n_shades = (int)shades.NS, view.n_blinds = (int)NL, view.blind_of_shade = of_shade.p;
        view.site = shades.view.site, view.tab = shades.tab.p, view.f = shades.f.p;
        view.pos_chan = i32.p + BL_POS_CHAN * NL, view.zone = i32.p + BL_ZONE * NL, view.set_chan = i32.p + BL_SET_CHAN * NL;
        view.enable_chan = i32.p + BL_ENABLE_CHAN * NL;
        view.beam_closed = f64.p + BL_BEAM * NL, view.diffuse_closed = f64.p + BL_DIFFUSE * NL, view.ground_closed = f64.p + BL_GROUND * NL;
        view.irr_close = f64.p + BL_IRR_CLOSE * NL, view.irr_open = f64.p + BL_IRR_OPEN * NL, view.half_band = f64.p + BL_HALF_BAND * NL;
        view.state = state.p;
        view.eff_f = shades.eff.p, view.eff_diffuse = shades.eff.p + shades.NS, view.eff_ground = shades.eff.p + 2 * shades.NS;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_position, double *host_incident, hipStream_t st) {
        if (NL == 0) return hipSuccess;
        const hipError_t e = series_fetch(blinds->state, state, st, series_fetch(host_incident, incident, st, series_fetch(host_position, position, st)));
        return switches.fetch(st, steps_closed.fetch(st, sum_position.fetch(st, e)));
    }
};

// The solar gains (heat_solar_gains): the apertures as structure of arrays, the entries as sliced ELL over the receivers in
// device record order (plan.hpp, SolarGainTables), the step's (Pb, Pd), ap_sum (always uploaded) and the transmitted rows.
struct GainsTerm {
    int64_t NA = 0;
    std::vector<int32_t> h_ap_dev;
    std::vector<double> h_ap_f64;
    SolarGainTables gnt;
    DevBuf<int32_t> ap_dev, ap;                 // [NA]; the entries' apertures
    DevBuf<double> ap_f64, transmitted, share;  // normal [3][NA] | coef [6][NA] | tau_diffuse [NA] | scale [NA]; [n_steps][NA]
    DevBuf<double2> power;                      // [NA]
    DevBuf<uint32_t> rec;
    DevBuf<int64_t> slice_off;
    Acc<double> sum;
    SeriesApertures apertures{};
    SeriesGains view{};
    void prepare(heat_batch *b, const heat_solar_gains *gains, InputsTerm &in) {
        NA = gains ? gains->n_apertures : 0;  // (entries need an aperture: there are none without)
        if (NA == 0) return;
        const int64_t S = b->n_surf;
        h_ap_dev.resize((size_t)NA);
        h_ap_f64.resize(11 * (size_t)NA);
        for (int64_t a = 0; a < NA; a++) {
            h_ap_dev[a] = b->h_dev_of[gains->ap_surface[a]];
            h_ap_f64[a] = gains->ap_normal_x[a];
            h_ap_f64[NA + a] = gains->ap_normal_y[a];
            h_ap_f64[2 * NA + a] = gains->ap_normal_z[a];
            for (int j = 0; j < 6; j++) h_ap_f64[(3 + j) * NA + a] = gains->ap_tau_coef[6 * a + j];
            h_ap_f64[9 * NA + a] = gains->ap_tau_diffuse[a];
            h_ap_f64[10 * NA + a] = gains->ap_scale[a];
        }
        build_solar_gain_tables(S, b->h_dev_of.data(), gains, gnt);
        sum.bind(gains->ap_sum, 0.0, &apertures.sum);
        for (uint32_t r : gnt.rec) in.need_gain(b, r >= (uint64_t)S);  // the solar gain arrays of the sides that receive (once each)
    }
    int upload(const heat_batch *b, const double *host_transmitted, int n_steps, const ShadesTerm &shades, const InputsTerm &in) {
        if (NA == 0) return HEAT_OK;
        SERIES_TRY(series_upload(ap_dev, h_ap_dev, "aperture tables"));
        SERIES_TRY(series_upload(ap_f64, h_ap_f64, "aperture tables"));
        SERIES_TRY(series_alloc(power, (size_t)NA, "aperture powers"));
        SERIES_TRY(sum.stage((size_t)NA, true, "aperture sums"));
        if (host_transmitted) SERIES_TRY(series_alloc(transmitted, (size_t)n_steps * NA, "transmitted powers"));
        SERIES_TRY(series_upload(rec, gnt.rec, "solar gain tables"));
        SERIES_TRY(series_upload(slice_off, gnt.slice_off.data(), gnt.rec.empty() ? 0 : gnt.slice_off.size(), "solar gain tables"));
        SERIES_TRY(series_upload(ap, gnt.ap, "solar gain tables"));
        SERIES_TRY(series_upload(share, gnt.share, "solar gain tables"));
        apertures.n = (int)NA, apertures.dev = ap_dev.p, apertures.site = b->n_sites > 1 ? b->d_site.p : nullptr;
        apertures.normal = ap_f64.p, apertures.coef = ap_f64.p + 3 * NA, apertures.tau_scale = ap_f64.p + 9 * NA;
        apertures.power = power.p, apertures.shade = shades.aperture.p, apertures.sf = shades.factors();
        view.n_receivers = (int)gnt.rec.size();
        view.rec = rec.p, view.slice_off = slice_off.p, view.ap = ap.p, view.power = power.p;
        view.share = reinterpret_cast<const double2 *>(share.p);
        view.gain[0] = in.d_gain[0].p, view.gain[1] = in.d_gain[1].p;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_transmitted, hipStream_t st) { return sum.fetch(st, series_fetch(host_transmitted, transmitted, st)); }
};

// The room radiation (heat_room_radiation): the entries as CSR over the receivers (plan.hpp, RoomRadiationTables), the face node of
// every distinct emitter side and the step's emissions, the receivers' records, sum_irradiance (always uploaded), the irradiance rows.
struct RadiationTerm {
    int64_t NR = 0;
    RoomRadiationTables rrt;
    std::vector<uint32_t> h_face, h_rec;
    DevBuf<uint32_t> face, rec;                    // [NM], [NR]
    DevBuf<double> emission, factor, irradiance;   // [NM], [NE], [n_steps][NR]
    DevBuf<int32_t> off, src;                      // [NR + 1], [NE]
    Acc<double> sum;
    SeriesRoomRadiation view{};
    void prepare(heat_batch *b, heat_room_radiation *radiation, InputsTerm &in) {
        NR = radiation ? radiation->n_receivers : 0;  // (entries need a receiver: there are none without)
        if (NR == 0) return;
        const int64_t S = b->n_surf;
        build_room_radiation_tables(S, radiation, rrt);
        h_face.resize(rrt.emitter.size());
        for (size_t j = 0; j < rrt.emitter.size(); j++) {
            const int64_t side = rrt.emitter[j] >= S, q = rrt.emitter[j] - side * S;
            h_face[j] = (uint32_t)node_slot_index(b->h_node_tile_base[q], b->h_node_geom[q], side ? (int)b->h_node_count[q] - 1 : 0);
        }
        h_rec.resize((size_t)NR);
        for (int64_t r = 0; r < NR; r++) {
            const int side = radiation->rc_side[r];
            h_rec[r] = (uint32_t)((int64_t)side * S + b->h_dev_of[radiation->rc_surface[r]]);
            in.need_gain(b, 2 + side);  // the long-wave gain arrays of the sides that receive (once each)
        }
        sum.bind(radiation->sum_irradiance, 0.0, &view.sum);
    }
    int upload(const double *host_irradiance, int n_steps, const InputsTerm &in) {
        if (NR == 0) return HEAT_OK;
        SERIES_TRY(series_upload(face, h_face, "room radiation tables"));
        SERIES_TRY(series_alloc(emission, h_face.size(), "emissions"));
        SERIES_TRY(series_upload(rec, h_rec, "room radiation tables"));
        SERIES_TRY(series_upload(off, rrt.off, "room radiation tables"));
        SERIES_TRY(series_upload(src, rrt.src, "room radiation tables"));
        SERIES_TRY(series_upload(factor, rrt.factor, "room radiation tables"));
        SERIES_TRY(sum.stage((size_t)NR, true, "irradiance sums"));
        if (host_irradiance) SERIES_TRY(series_alloc(irradiance, (size_t)n_steps * NR, "irradiances"));
        view.n_emitters = (int)h_face.size(), view.n_receivers = (int)NR, view.face = face.p, view.emission = emission.p;
        view.rec = rec.p, view.off = off.p, view.src = src.p, view.factor = factor.p;
        view.gain[0] = in.d_gain[2].p, view.gain[1] = in.d_gain[3].p;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_irradiance, hipStream_t st) { return sum.fetch(st, series_fetch(host_irradiance, irradiance, st)); }
};

// The ambient drive (heat_ambient_drive), or one heat_batch_set_ambient: the sides' records and the back records that follow a front
// (plan.hpp, AmbientTables), the caller's lists, the mixing zones and factors only where a side mixes, sum_temperature, the ambient_t rows.
struct AmbientTerm {
    int64_t NB = 0;
    AmbientTables abt;
    std::vector<int32_t> h_zone;
    std::vector<double> h_mix;
    DevBuf<uint32_t> rec, peer;            // [N]
    DevBuf<int32_t> chan, zone;            // [N]
    DevBuf<double> gain, offset, mix, t;   // [N]; t: [n_steps][N], the setter: the temperatures [N]
    Acc<double> sum;
    SeriesAmbient view{};
    void prepare(const heat_batch *b, const int32_t *const side_kind[2], heat_ambient_drive *ambient) {
        NB = ambient ? ambient->n_sides : 0;
        if (NB == 0) return;
        build_ambient_tables(b->n_surf, b->h_dev_of.data(), side_kind, NB, ambient->surface, ambient->side, abt);
        sum.bind(ambient->sum_temperature, 0.0, &view.sum);
        bool mixes = false;
        for (int64_t i = 0; i < NB && ambient->mix_zone && !mixes; i++) mixes = ambient->mix_zone[i] >= 0;
        if (!mixes) return;
        h_zone.assign(ambient->mix_zone, ambient->mix_zone + NB);
        h_mix.assign((size_t)NB, 0.0);
        for (int64_t i = 0; i < NB; i++)
            if (h_zone[(size_t)i] >= 0) h_mix[(size_t)i] = ambient->mix[i];
    }
    int upload_tables() {
        SERIES_TRY(series_upload(rec, abt.rec, "ambient tables"));
        SERIES_TRY(series_upload(peer, abt.peer, "ambient tables"));
        view.rec = rec.p, view.peer = peer.p;
        return HEAT_OK;
    }
    int upload(const heat_ambient_drive *ambient, const double *host_t, int n_steps) {
        if (NB == 0) return HEAT_OK;
        SERIES_TRY(upload_tables());
        SERIES_TRY(series_upload(chan, ambient->chan, (size_t)NB, "ambient tables"));
        SERIES_TRY(report_array(gain, ambient->gain, (size_t)NB, true, "ambient tables"));
        SERIES_TRY(report_array(offset, ambient->offset, (size_t)NB, true, "ambient tables"));
        if (!h_zone.empty()) {
            SERIES_TRY(series_upload(zone, h_zone, "ambient tables"));
            SERIES_TRY(series_upload(mix, h_mix, "ambient tables"));
        }
        SERIES_TRY(sum.stage((size_t)NB, true, "ambient temperature sums"));
        if (host_t) SERIES_TRY(series_alloc(t, (size_t)n_steps * NB, "ambient temperatures"));
        view.n_sides = (int)NB, view.chan = chan.p, view.gain = gain.p, view.offset = offset.p, view.mix_zone = zone.p, view.mix = mix.p;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_t, hipStream_t st) { return sum.fetch(st, series_fetch(host_t, t, st)); }
};

// The air paths (heat_air_paths): the list sorted by target zone with CSR offsets (plan.hpp, AirPathTables), the state bytes,
// the accumulators (always uploaded) and the path_q rows in the caller's order.
struct AirTerm {
    heat_air_paths *air = nullptr;
    int64_t NP = 0;
    AirPathTables apt;
    std::vector<uint8_t> h_state;
    DevBuf<int32_t> i32;
    DevBuf<double> f64, path_q;  // path_q: [n_steps][NP]
    DevBuf<uint8_t> state;       // [NP]
    Acc<double> sum_q;
    Acc<int64_t> steps_open, switches;
    AirPathsDev view{};
    void prepare(const heat_batch *b, heat_air_paths *air_) {
        air = air_;
        NP = air ? air->n_paths : 0;
        if (NP == 0) return;
        build_air_path_tables(b->n_zones, air, apt);
        h_state.assign((size_t)NP, 0);
        if (air->state) std::copy(air->state, air->state + NP, h_state.begin());
        sum_q.bind(air->sum_q, 0.0, &view.sum_q), steps_open.bind(air->steps_open, 0, &view.steps_open);
        switches.bind(air->switches, 0, &view.switches);
    }
    int upload(const heat_batch *b, const double *host_q, int n_steps) {
        if (NP == 0) return HEAT_OK;
        SERIES_TRY(series_upload(i32, apt.i32, "air path tables"));
        SERIES_TRY(series_upload(f64, apt.f64, "air path tables"));
        SERIES_TRY(series_upload(state, h_state, "air path states"));
        SERIES_TRY(sum_q.stage((size_t)NP, true, "air path accumulators"));
        SERIES_TRY(steps_open.stage((size_t)NP, true, "air path accumulators"));
        SERIES_TRY(switches.stage((size_t)NP, true, "air path accumulators"));
        if (host_q) SERIES_TRY(series_alloc(path_q, (size_t)n_steps * NP, "air path powers"));
        const int32_t *list = i32.p + (b->n_zones + 1);
        view.off = i32.p, view.source = list, view.temp_chan = list + NP, view.volume_chan = list + 2 * NP, view.open_chan = list + 3 * NP;
        view.orig = list + 4 * NP, view.state = state.p;
        view.volume_gain = f64.p, view.sense = f64.p + NP, view.half_band = f64.p + 2 * NP, view.min_delta = f64.p + 3 * NP;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_q, hipStream_t st) {
        if (NP == 0) return hipSuccess;
        const hipError_t e = series_fetch(air->state, state, st, series_fetch(host_q, path_q, st));
        return switches.fetch(st, steps_open.fetch(st, sum_q.fetch(st, e)));
    }
};

// The air handlers (heat_air_handlers): the branches as CSR over the units and the supply branches as CSR over the zones
// (plan.hpp, HandlerTables), the units' rows, the step's scratch (Ts per unit, m per branch), the bypass bytes, the
// accumulators (always uploaded) and the four arrays of rows in the caller's order. Nothing of it exists on the device
// without units.
struct HandlersTerm {
    heat_air_handlers *ah = nullptr;
    int64_t NU = 0, NBR = 0;
    HandlerTables aht;
    std::vector<uint8_t> h_bypass;
    DevBuf<int32_t> unit_off, u_zone, u_chan, u_orig, zone_off, z_unit, z_orig, i32;
    DevBuf<uint8_t> u_kind, bypass;
    DevBuf<double> u_gain, f64, ts, m, supply_t, recovered, coil_q, branch_q;  // the last four: [n_steps][NU] thrice, [n_steps][NBR]
    Acc<double> unit_f64[3];   // sum_recovered, sum_heating, sum_cooling
    Acc<int64_t> unit_i64[4];  // steps_bypass, switches, steps_heat_saturated, steps_cool_saturated
    Acc<double> sum_branch_q;
    HandlersDev view{};
    void prepare(const heat_batch *b, heat_air_handlers *ah_) {
        ah = ah_;
        NU = ah ? ah->n_units : 0;
        if (NU == 0) return;
        NBR = ah->n_branches;
        build_air_handler_tables(b->n_zones, ah, aht);
        h_bypass.assign((size_t)NU, 0);
        if (ah->bypass) std::copy(ah->bypass, ah->bypass + NU, h_bypass.begin());
        unit_f64[0].bind(ah->sum_recovered, 0.0, &view.sum_recovered), unit_f64[1].bind(ah->sum_heating, 0.0, &view.sum_heating);
        unit_f64[2].bind(ah->sum_cooling, 0.0, &view.sum_cooling);
        unit_i64[0].bind(ah->steps_bypass, 0, &view.steps_bypass), unit_i64[1].bind(ah->switches, 0, &view.switches);
        unit_i64[2].bind(ah->steps_heat_saturated, 0, &view.steps_heat_saturated);
        unit_i64[3].bind(ah->steps_cool_saturated, 0, &view.steps_cool_saturated);
        sum_branch_q.bind(ah->sum_branch_q, 0.0, &view.sum_branch_q);
    }
    bool supplies() const { return !aht.z_orig.empty(); }
    int upload(const double *host_supply, const double *host_recovered, const double *host_coil, const double *host_branch, int n_steps) {
        if (NU == 0) return HEAT_OK;
        SERIES_TRY(series_upload(unit_off, aht.unit_off, "air handler tables"));
        SERIES_TRY(series_upload(u_zone, aht.u_zone, "air handler tables"));
        SERIES_TRY(series_upload(u_chan, aht.u_chan, "air handler tables"));
        SERIES_TRY(series_upload(u_orig, aht.u_orig, "air handler tables"));
        SERIES_TRY(series_upload(u_kind, aht.u_kind, "air handler tables"));
        SERIES_TRY(series_upload(u_gain, aht.u_gain, "air handler tables"));
        SERIES_TRY(series_upload(zone_off, aht.zone_off, "air handler tables"));
        SERIES_TRY(series_upload(z_unit, aht.z_unit, "air handler tables"));
        SERIES_TRY(series_upload(z_orig, aht.z_orig, "air handler tables"));
        SERIES_TRY(series_upload(i32, aht.i32, "air handler tables"));
        SERIES_TRY(series_upload(f64, aht.f64, "air handler tables"));
        SERIES_TRY(series_upload(bypass, h_bypass, "air handler bypass states"));
        SERIES_TRY(series_alloc(ts, (size_t)NU, "supply temperatures"));
        SERIES_TRY(series_alloc(m, (size_t)NBR, "branch mass flows"));
        for (auto &a : unit_f64) SERIES_TRY(a.stage((size_t)NU, true, "air handler accumulators"));
        for (auto &a : unit_i64) SERIES_TRY(a.stage((size_t)NU, true, "air handler accumulators"));
        SERIES_TRY(sum_branch_q.stage((size_t)NBR, true, "air handler accumulators"));
        if (host_supply) SERIES_TRY(series_alloc(supply_t, (size_t)n_steps * NU, "supply temperatures"));
        if (host_recovered) SERIES_TRY(series_alloc(recovered, (size_t)n_steps * NU, "recovered powers"));
        if (host_coil) SERIES_TRY(series_alloc(coil_q, (size_t)n_steps * NU, "coil powers"));
        if (host_branch) SERIES_TRY(series_alloc(branch_q, (size_t)n_steps * NBR, "branch powers"));
        view.n_units = (int)NU, view.unit_off = unit_off.p, view.u_zone = u_zone.p, view.u_chan = u_chan.p, view.u_orig = u_orig.p;
        view.u_kind = u_kind.p, view.u_gain = u_gain.p, view.zone_off = zone_off.p, view.z_unit = z_unit.p, view.z_orig = z_orig.p;
        view.outdoor_chan = i32.p + AH_OUTDOOR_CHAN * NU, view.eff_chan = i32.p + AH_EFF_CHAN * NU, view.bypass_chan = i32.p + AH_BYPASS_CHAN * NU;
        view.heat_chan = i32.p + AH_HEAT_CHAN * NU, view.cool_chan = i32.p + AH_COOL_CHAN * NU;
        view.eff_gain = f64.p + AH_EFF_GAIN * NU, view.half_band = f64.p + AH_HALF_BAND * NU, view.min_delta = f64.p + AH_MIN_DELTA * NU;
        view.heat_cap = f64.p + AH_HEAT_CAP * NU, view.cool_cap = f64.p + AH_COOL_CAP * NU;
        view.ts = ts.p, view.m = m.p, view.bypass = bypass.p;
        return HEAT_OK;
    }
    hipError_t fetch(double *host_supply, double *host_recovered, double *host_coil, double *host_branch, hipStream_t st) {
        if (NU == 0) return hipSuccess;
        hipError_t e = series_fetch(host_recovered, recovered, st, series_fetch(host_supply, supply_t, st));
        e = series_fetch(ah->bypass, bypass, st, series_fetch(host_branch, branch_q, st, series_fetch(host_coil, coil_q, st, e)));
        return sum_branch_q.fetch(st, for_each_acc(unit_i64, &Acc<int64_t>::fetch, st, for_each_acc(unit_f64, &Acc<double>::fetch, st, e)));
    }
};

// The anisotropic sky (heat_sky_aniso): the coefficient table as given, beside the record table, and the bands of the three
// consumers — the sides' per DEVICE surface, the apertures' and the shades' in the caller's order as their tables are; zeros
// where the caller gave none. Absent (every pointer NULL) without aniso: the isotropic kernels are launched.
struct AnisoTerm {
    const heat_sky_aniso *an = nullptr;
    std::vector<double> h_side;
    DevBuf<SkyCoef> coef;                  // [n_steps][n_sites]
    DevBuf<double> side, aperture, shade;  // [2][S], [NA], [NS]
    void prepare(heat_batch *b, const heat_sky_aniso *an_, unsigned sky_bits) {
        an = an_;
        if (!an || !(sky_bits & 3)) return;
        h_side.assign(2 * (size_t)b->n_surf, 0.0);
        if (an->front_band) to_device_order(b, an->front_band, h_side.data());
        if (an->back_band) to_device_order(b, an->back_band, h_side.data() + b->n_surf);
    }
    static int band(DevBuf<double> &buf, const double *src, int64_t n, const char *what) {
        if (n <= 0) return HEAT_OK;
        if (src) return series_upload(buf, src, (size_t)n, what);
        return series_upload(buf, std::vector<double>((size_t)n, 0.0), what);
    }
    int upload(const heat_batch *b, const heat_series *s, int64_t NA, int64_t NS) {
        if (!an) return HEAT_OK;
        SERIES_TRY(series_upload(coef, reinterpret_cast<const SkyCoef *>(an->coef), (size_t)s->n_steps * b->n_sites, "sky coefficients"));
        SERIES_TRY(series_upload(side, h_side, "side bands"));
        SERIES_TRY(band(aperture, an->aperture_band, NA, "aperture bands"));
        SERIES_TRY(band(shade, an->shade_band, NS, "shade bands"));
        return HEAT_OK;
    }
};
static_assert(sizeof(SkyCoef) == sizeof(heat_sky_coef) && sizeof(heat_sky_coef) == 16, "SkyCoef mirrors heat_sky_coef");

// Comfort (heat_comfort): the entries as CSR over the sensors with their face nodes and weights (plan.hpp, ComfortTables), the
// sensors' rows, the step's operative temperatures, the accumulators (uploaded on resume, else started on the device) and the
// operative / mrt rows; with a control sensor the control sensor of every zone and the step's control temperatures. Nothing of
// it exists on the device without sensors.
struct ComfortTerm {
    heat_comfort *cf = nullptr;
    int64_t NF = 0;
    ComfortTables cft;
    DevBuf<int32_t> off, i32, ctl;                    // [NF + 1], [kComfortI32Rows][NF], [Z]
    DevBuf<uint32_t> face;                            // [NE]
    DevBuf<double> weight, air_weight, top, control_T, operative, mrt;  // [NE], [NF], [NF], [Z], [n_steps][NF] twice
    Acc<double> f64[6];   // sum_operative, min_operative, max_operative, deg_below, deg_above, max_above
    Acc<int64_t> i64[6];  // n_occupied, step_min, step_max, n_below, n_above, step_max_above
    SeriesComfort view{};
    void prepare(const heat_batch *b, heat_comfort *cf_) {
        cf = cf_;
        NF = cf ? cf->n_sensors : 0;
        if (NF == 0) return;
        const double inf = std::numeric_limits<double>::infinity();
        build_comfort_tables(b->n_zones, cf, b->h_node_tile_base.data(), b->h_node_geom.data(), b->h_first_slot.data(), b->h_node_count.data(), cft);
        f64[0].bind(cf->sum_operative, 0.0, &view.sum_operative), f64[1].bind(cf->min_operative, inf, &view.min_operative);
        f64[2].bind(cf->max_operative, -inf, &view.max_operative), f64[3].bind(cf->deg_below, 0.0, &view.deg_below);
        f64[4].bind(cf->deg_above, 0.0, &view.deg_above), f64[5].bind(cf->max_above, -inf, &view.max_above);
        i64[0].bind(cf->n_occupied, 0, &view.n_occupied), i64[1].bind(cf->step_min, -1, &view.step_min);
        i64[2].bind(cf->step_max, -1, &view.step_max), i64[3].bind(cf->n_below, 0, &view.n_below);
        i64[4].bind(cf->n_above, 0, &view.n_above), i64[5].bind(cf->step_max_above, -1, &view.step_max_above);
    }
    int upload(const heat_batch *b, const double *host_operative, const double *host_mrt, int n_steps) {
        if (NF == 0) return HEAT_OK;
        const bool resume = cf->resume != 0;
        SERIES_TRY(series_upload(off, cft.off, "comfort tables"));
        SERIES_TRY(series_upload(face, cft.face, "comfort tables"));
        SERIES_TRY(series_upload(weight, cft.weight, "comfort tables"));
        SERIES_TRY(series_upload(i32, cft.i32, "comfort tables"));
        SERIES_TRY(series_upload(air_weight, cft.air_weight, "comfort tables"));
        SERIES_TRY(series_alloc(top, (size_t)NF, "operative temperatures"));
        if (cft.any_control) {
            SERIES_TRY(series_upload(ctl, cft.ctl_sensor, "comfort tables"));
            SERIES_TRY(series_alloc(control_T, (size_t)b->n_zones, "control temperatures"));
        }
        if (host_operative) SERIES_TRY(series_alloc(operative, (size_t)n_steps * NF, "operative temperatures"));
        if (host_mrt) SERIES_TRY(series_alloc(mrt, (size_t)n_steps * NF, "mean radiant temperatures"));
        for (auto &a : f64) SERIES_TRY(a.stage((size_t)NF, resume, "comfort accumulators"));
        for (auto &a : i64) SERIES_TRY(a.stage((size_t)NF, resume, "comfort accumulators"));
        view.n_sensors = (int)NF, view.off = off.p, view.face = face.p, view.weight = weight.p;
        view.zone = i32.p + CF_ZONE * NF, view.occ_chan = i32.p + CF_OCC_CHAN * NF, view.lo_chan = i32.p + CF_LO_CHAN * NF;
        view.hi_chan = i32.p + CF_HI_CHAN * NF, view.air_weight = air_weight.p, view.top = top.p;
        return HEAT_OK;
    }
    hipError_t start(hipStream_t st) {
        return NF > 0 && cf->resume == 0 ? for_each_acc(i64, &Acc<int64_t>::start, st, for_each_acc(f64, &Acc<double>::start, st)) : hipSuccess;
    }
    hipError_t fetch(double *host_operative, double *host_mrt, hipStream_t st) {
        if (NF == 0) return hipSuccess;
        const hipError_t e = series_fetch(host_mrt, mrt, st, series_fetch(host_operative, operative, st));
        return for_each_acc(i64, &Acc<int64_t>::fetch, st, for_each_acc(f64, &Acc<double>::fetch, st, e));
    }
};

// What heat_batch_march_series_call takes (the eleven positional entry points fill what they have) and, beside it, the comfort
// term and its two arrays of rows (heat_batch_march_series_comfort) and the air handlers with their four
// (heat_batch_march_series_handlers); filled by field name. no_trace_ok: a NULL trace records none.
struct SeriesCall {
    const heat_series *s = nullptr;
    const heat_sky *sky = nullptr;
    const heat_sky_aniso *aniso = nullptr;
    const heat_shades *shades = nullptr;
    const heat_solar_gains *gains = nullptr;
    const heat_zone_loads *l = nullptr;
    heat_air_paths *air = nullptr;
    heat_ideal_loads *il = nullptr;
    heat_series_report *r = nullptr;
    double *trace = nullptr, *applied = nullptr, *ideal_q = nullptr, *transmitted = nullptr, *path_q = nullptr, *sunlit = nullptr;
    heat_room_radiation *radiation = nullptr;
    double *irradiance = nullptr;
    heat_ambient_drive *ambient = nullptr;
    double *ambient_t = nullptr;
    heat_blinds *blinds = nullptr;
    double *position = nullptr, *blind_incident = nullptr;
    heat_comfort *comfort = nullptr;
    double *operative = nullptr, *mrt = nullptr;
    heat_air_handlers *handlers = nullptr;
    double *supply_t = nullptr, *recovered = nullptr, *coil_q = nullptr, *branch_q = nullptr;
    int32_t *failed_step = nullptr;
    bool no_trace_ok = false;
};

}  // namespace

// ===========================================================================
extern "C" {


int heat_batch_create(const heat_batch_desc *desc, heat_batch **out) {
    heat_batch_options opt;
    memset(&opt, 0, sizeof opt);
    opt.device = -1;
    opt.n_ranks = 1;
    return heat_batch_create_ex(desc, &opt, out);
}

static int create_impl(const heat_batch_desc *desc, const heat_batch_options *opt_in, int32_t n_sites,
                       const int32_t *site_of_surface, bool sites, heat_batch **out) {
    if (!out) return fail(HEAT_E_INVALID_ARG, "out is NULL");
    *out = nullptr;
    heat_batch_options opt;
    memset(&opt, 0, sizeof opt);
    opt.device = -1;
    opt.n_ranks = 1;
    if (opt_in) opt = *opt_in;
    if (sites) {  // (before any device work)
        std::string err;
        const int rc = check_sites(desc, opt, n_sites, site_of_surface, err);
        if (rc) return fail(rc, "%s", err.c_str());
    }
    if (opt.n_ranks < 1) opt.n_ranks = 1;
    if (opt.nodes_per_lane != 0 && opt.nodes_per_lane != 4 && opt.nodes_per_lane != 8 && opt.nodes_per_lane != 16)
        return fail(HEAT_E_INVALID_ARG, "nodes_per_lane must be 0, 4, 8 or 16");
    int rc;
    {
        std::string err;
        rc = check_desc(desc, err);
        if (rc) return fail(rc, "%s", err.c_str());
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(HEAT_E_DEVICE, "no HIP device available: this library has no CPU fallback");
    heat_batch *b = new heat_batch();
    if (opt.device >= 0) {
        b->device = opt.device;
    } else if (hipGetDevice(&b->device) != hipSuccess) {
        delete b;
        return fail(HEAT_E_DEVICE, "hipGetDevice failed");
    }
    b->n_ranks = opt.n_ranks;
    b->rank = opt.rank;
    b->use_graph = opt.use_graph != 0;
    b->fusion_on = opt.no_fusion != 1;
    rc = select_device(b);
    if (!rc) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, b->device) == hipSuccess && prop.multiProcessorCount > 0) b->n_cu = prop.multiProcessorCount;
    }
    if (!rc) {
        if (opt.stream) {
            b->stream = reinterpret_cast<hipStream_t>(opt.stream);
        } else {
            hipError_t e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
            if (e != hipSuccess) rc = fail(HEAT_E_DEVICE, "hipStreamCreate failed: %s", hipGetErrorString(e));
            b->own_stream = true;
        }
    }
    if (!rc) {
        for (int i = 0; i < heat_batch::kSideStreams && !rc; i++) {
            if (hipStreamCreateWithFlags(&b->side[i], hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&b->ev_join[i], hipEventDisableTiming) != hipSuccess)
                rc = fail(HEAT_E_DEVICE, "side stream creation failed");
        }
        if (!rc && hipStreamCreateWithFlags(&b->fused_stream, hipStreamNonBlocking) != hipSuccess)
            rc = fail(HEAT_E_DEVICE, "side stream creation failed");
        if (!rc && (hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&b->ev_fused, hipEventDisableTiming) != hipSuccess))
            rc = fail(HEAT_E_DEVICE, "event creation failed");
    }
    if (!rc) rc = build(b, desc, opt, n_sites, site_of_surface);
    if (rc) {
        delete b;
        return rc;
    }
    *out = b;
    return HEAT_OK;
}

int heat_batch_create_ex(const heat_batch_desc *desc, const heat_batch_options *opt, heat_batch **out) {
    return create_impl(desc, opt, 1, nullptr, false, out);
}

int heat_batch_create_sites(const heat_batch_desc *desc, const heat_batch_options *opt, int32_t n_sites,
                            const int32_t *site_of_surface, heat_batch **out) {
    return create_impl(desc, opt, n_sites, site_of_surface, true, out);
}

int32_t heat_batch_n_sites(const heat_batch *b) { return b ? b->n_sites : 0; }

int heat_batch_create_shard(const heat_batch_desc *desc, const heat_batch_options *opt, const int32_t *rank_of_surface,
                            heat_batch **out) {
    if (!desc || !opt || !rank_of_surface || !out) return fail(HEAT_E_INVALID_ARG, "NULL argument");
    {
        std::string err;
        const int rc = check_desc(desc, err);
        if (rc) return fail(rc, "%s", err.c_str());
    }
    for (int64_t s = 0; s < desc->n_surfaces; s++)
        if (rank_of_surface[s] < 0 || rank_of_surface[s] >= std::max(opt->n_ranks, 1))
            return fail(HEAT_E_SIZE, "surface %lld: rank %d outside [0, %d)", (long long)s, rank_of_surface[s], std::max(opt->n_ranks, 1));
    ShardDesc sh;
    sh.build(desc, rank_of_surface, opt->rank);
    int rc = heat_batch_create_ex(&sh.desc, opt, out);
    if (rc) return rc;
    heat_batch *b = *out;
    // Zones by the ranks that face them: a zone nobody faces falls to rank z % n_ranks (it still follows a0 / b0,
    // model.rs:410-423); when no zone is faced from two ranks the batch marches without any exchange.
    const int64_t Z = desc->n_zones;
    const int n_ranks = std::max(opt->n_ranks, 1);
    std::vector<int32_t> first(Z, -1);
    std::vector<uint8_t> shared(Z, 0), owned(Z, 0);
    auto touch = [&](int32_t z, int32_t rk) {
        if (first[z] < 0) first[z] = rk;
        else if (first[z] != rk) shared[z] = 1;
    };
    for (int64_t s = 0; s < desc->n_surfaces; s++) {
        if (desc->front_kind[s] == HEAT_BOUNDARY_SPACE) touch(desc->front_zone[s], rank_of_surface[s]);
        if (desc->back_kind[s] == HEAT_BOUNDARY_SPACE) touch(desc->back_zone[s], rank_of_surface[s]);
    }
    int64_t n_shared = 0;
    for (int64_t z = 0; z < Z; z++) {
        n_shared += shared[z];
        owned[z] = (first[z] < 0 && z % n_ranks == opt->rank) ? 1 : 0;
    }
    rc = heat_batch_set_owned_zones(b, owned.data());
    if (!rc && n_ranks > 1 && n_shared == 0) rc = heat_batch_set_shared_zones(b, nullptr, 0);
    if (rc) {
        heat_batch_destroy(b);
        *out = nullptr;
    }
    return rc;
}

void heat_batch_destroy(heat_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    delete b;
}

int64_t heat_batch_n_surfaces(const heat_batch *b) { return b ? b->n_surf : 0; }
int64_t heat_batch_n_nodes(const heat_batch *b) { return b ? b->n_nodes : 0; }
int64_t heat_batch_n_zones(const heat_batch *b) { return b ? b->n_zones : 0; }
int64_t heat_batch_algorithmic_bytes(const heat_batch *b) { return b ? b->algorithmic_bytes : 0; }
int heat_batch_class_counts(const heat_batch *b, int64_t counts[5]) {
    if (!b || !counts) return fail(HEAT_E_INVALID_ARG, "NULL argument");
    for (int i = 0; i < 5; i++) counts[i] = b->class_counts[i];
    return HEAT_OK;
}

static int transfer_in(heat_batch *b, const double *state, size_t n_state, bool full) {
    if (!b || !state) return fail(HEAT_E_INVALID_ARG, "NULL argument");
    if ((int64_t)n_state != b->n_state) return fail(HEAT_E_SIZE, "n_state %zu, batch was created for %lld", n_state, (long long)b->n_state);
    int rc = select_device(b);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->d_state.p, state, n_state * sizeof(double), hipMemcpyHostToDevice));
    if (full) {
        for (int c = 0; c < kNumFast; c++)
            launch_nodes_fast(kFastM[c], b->d_fast_tiles[c].p, b->n_fast_tiles[c], b->d_T.p, b->d_meta.p,
                              b->d_first_slot.p, b->d_state.p, 0, b->d_cls.p, b->stream);
        launch_nodes_general(b->d_gen_tiles.p, b->n_gen_tiles, b->d_T.p, b->d_meta.p, b->d_first_slot.p,
                             b->d_state.p, 0, b->stream);
    }
    launch_surf_scalars((int)b->n_surf, b->sl, b->d_side_dyn.p, b->d_side_out.p, b->d_side_alpha.p, b->d_state.p, 0,
                        full ? 3 : 1, b->stream);
    launch_zone_scalars((int)b->n_zones, b->d_zone_slot.p, b->d_zone_T.p, b->d_state.p, 0, b->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
    return HEAT_OK;
}

int heat_batch_upload_state(heat_batch *b, const double *state, size_t n_state) {
    const int rc = transfer_in(b, state, n_state, true);
    if (rc == HEAT_OK) b->host_zones_stale = false;
    return rc;
}
// Only what other modules write between two marches (surface_trait.rs:81-125's irradiance slots, the zones'
// dry-bulb slots): gathered on the host into pinned memory, one copy, converted on the device.
int heat_batch_upload_inputs(heat_batch *b, const double *state, size_t n_state) {
    if (!b || !state) return fail(HEAT_E_INVALID_ARG, "NULL argument");
    if ((int64_t)n_state != b->n_state) return fail(HEAT_E_SIZE, "n_state %zu, batch was created for %lld", n_state, (long long)b->n_state);
    int rc = select_device(b);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));  // (the staging buffer may still feed the previous call's copy)
    const int64_t S = b->n_surf, Z = b->n_zones;
    double *pin = b->h_pin;
    const int64_t *slots = b->h_in_slots.data();
    // gathered by the thread pool and copied in pieces: the copy of one piece travels while the next is gathered
    const int64_t total = 4 * S;
    const int n_pieces = total >= (int64_t)1 << 20 ? 4 : 1;
    for (int pc = 0; pc < n_pieces; pc++) {
        const int64_t a = total * pc / n_pieces, e = total * (pc + 1) / n_pieces;
        b->pool->run(e - a, [&](int64_t i0, int64_t i1) {
            for (int64_t i = a + i0; i < a + i1; i++) pin[i] = state[slots[i]];
        });
        if (e > a)
            HIP_TRY(hipMemcpyAsync(b->d_compact.p + a, pin + a, (size_t)(e - a) * sizeof(double), hipMemcpyHostToDevice, b->stream));
    }
    // The zones' dry-bulb slots are taken from the caller's state only while that state holds what this path last
    // computed: after a march whose outputs left HEAT_OUT_ZONE_TEMPERATURES out (heat_batch_march_ex, or a resident march
    // without a download) the caller's zone slots are OLDER than the device's — taking them would set the zones back by a
    // call (found by tools/fuzz.py). heat_batch_upload_state always takes everything.
    const bool take_zones = Z > 0 && !b->host_zones_stale;
    if (take_zones) {
        for (int64_t z = 0; z < Z; z++) pin[4 * S + z] = state[b->h_zone_slot_h[z]];
        HIP_TRY(hipMemcpyAsync(b->d_compact.p + 4 * S, pin + 4 * S, (size_t)Z * sizeof(double), hipMemcpyHostToDevice, b->stream));
    }
    launch_inputs_compact((int)S, take_zones ? (int)Z : 0, b->d_compact.p, b->d_side_alpha.p, b->d_side_dyn.p, b->d_zone_T.p, b->sl,
                          b->direct_runs.empty() ? nullptr : b->d_state.p, b->stream);
    HIP_TRY(hipGetLastError());
    return HEAT_OK;
}

int heat_batch_download_state(heat_batch *b, double *state, size_t n_state) {
    return heat_batch_download_outputs(b, state, n_state, HEAT_OUT_ALL);
}

// The outputs of this path into the caller's state: gathered on the device into a compact buffer in the caller's
// surface order, copied through two pinned staging halves (the copy of one piece runs while the thread pool
// scatters the piece before it), only the slots the path owns are written.
static int download_impl(heat_batch *b, double *state, size_t n_state, int32_t what, bool inputs_fresh);

int heat_batch_download_outputs(heat_batch *b, double *state, size_t n_state, int32_t what) {
    return download_impl(b, state, n_state, what, false);
}

// inputs_fresh: the irradiance slots of `state` were uploaded from this very array in the same call (heat_batch_march):
// the mirror then equals the caller's state on every slot of the direct runs that is not an output, and whole runs can
// be copied back.
static int download_impl(heat_batch *b, double *state, size_t n_state, int32_t what, bool inputs_fresh) {
    if (!b || !state) return fail(HEAT_E_INVALID_ARG, "NULL argument");
    if ((int64_t)n_state != b->n_state) return fail(HEAT_E_SIZE, "n_state %zu, batch was created for %lld", n_state, (long long)b->n_state);
    int rc = select_device(b);
    if (rc) return rc;
    const int64_t S = b->n_surf, Z = b->n_zones, N = b->n_nodes;
    const bool delivers_zones = (what & HEAT_OUT_ZONE_TEMPERATURES) != 0;
    bool nodes = (what & HEAT_OUT_NODE_TEMPERATURES) != 0;
    bool scalars = (what & (HEAT_OUT_SURFACE_SCALARS | HEAT_OUT_ZONE_TEMPERATURES)) != 0;
    if (nodes && (what & HEAT_OUT_SURFACE_SCALARS) && inputs_fresh && !b->direct_runs.empty()) {
        // Direct: node temperatures, hs and heat flows go into the mirror; its runs — outputs and the inputs this call
        // uploaded, nothing else — are copied straight into the caller's array (pageable or not: 56 GB/s either way on
        // this platform, tools/pcie_bw.py). The zones follow through the staged path below.
        for (int c = 0; c < kNumFast; c++)
            launch_nodes_fast(kFastM[c], b->d_fast_tiles[c].p, b->n_fast_tiles[c], b->d_T.p, b->d_meta.p,
                              b->d_first_slot.p, b->d_state.p, 1, b->d_cls.p, b->stream);
        launch_nodes_general(b->d_gen_tiles.p, b->n_gen_tiles, b->d_T.p, b->d_meta.p, b->d_first_slot.p, b->d_state.p, 1,
                             b->stream);
        launch_surf_scalars((int)S, b->sl, b->d_side_dyn.p, b->d_side_out.p, b->d_side_alpha.p, b->d_state.p, 1, 2, b->stream);
        HIP_TRY(hipGetLastError());
        for (auto &r : b->direct_runs)
            HIP_TRY(hipMemcpyAsync(state + r.first, b->d_state.p + r.first, (size_t)(r.second - r.first) * sizeof(double),
                                   hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        nodes = false;
        what &= ~(HEAT_OUT_NODE_TEMPERATURES | HEAT_OUT_SURFACE_SCALARS);
        scalars = (what & HEAT_OUT_ZONE_TEMPERATURES) != 0;
        if (!scalars) return HEAT_OK;
    }
    if (nodes) {
        for (int c = 0; c < kNumFast; c++)
            launch_nodes_fast(kFastM[c], b->d_fast_tiles[c].p, b->n_fast_tiles[c], b->d_T.p, b->d_meta.p,
                              b->d_compact_off.p, b->d_compact.p, 1, b->d_cls.p, b->stream);
        launch_nodes_general(b->d_gen_tiles.p, b->n_gen_tiles, b->d_T.p, b->d_meta.p, b->d_compact_off.p, b->d_compact.p,
                             1, b->stream);
    }
    if (scalars)
        launch_outputs_compact((int)S, (int)Z, b->d_side_out.p, b->d_orig_of32.p, b->d_zone_T.p, b->d_compact.p + N, b->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
    const size_t half = b->pin_doubles / 2;
    // the scalar part first (one piece), then the node pieces; piece i uses staging half i % 2
    struct Piece { int64_t off, count, s0, s1; bool is_nodes; };
    std::vector<Piece> pieces;
    // (zones alone: only the tail of the scalar part travels)
    const int64_t sc_off = (what & HEAT_OUT_SURFACE_SCALARS) ? 0 : 4 * S;
    if (scalars) pieces.push_back({N + sc_off, 4 * S + Z - sc_off, 0, S, false});
    if (nodes)
        for (auto &ch : b->out_chunks)
            pieces.push_back({b->h_node_off[ch.first], b->h_node_off[ch.second] - b->h_node_off[ch.first], ch.first, ch.second, true});
    auto issue = [&](size_t i) -> hipError_t {
        const Piece &p = pieces[i];
        // (the scalar piece may be longer than a half: it is alone in the buffer then — the node pieces start after it)
        double *dst = b->h_pin + (i % 2) * half;
        hipError_t e = hipMemcpyAsync(dst, b->d_compact.p + p.off, (size_t)p.count * sizeof(double), hipMemcpyDeviceToHost, b->copy_stream);
        if (e != hipSuccess) return e;
        return hipEventRecord(b->ev_copy[i % 2], b->copy_stream);
    };
    const bool big_scalars = scalars && (size_t)(4 * S + Z) > half;
    for (size_t i = 0; i < pieces.size(); i++) {
        if (i == 0) HIP_TRY(issue(0));
        HIP_TRY(hipEventSynchronize(b->ev_copy[i % 2]));
        // the next copy runs while this piece is scattered (not into a buffer the scalar piece spills over)
        const bool overlap = i + 1 < pieces.size() && !(big_scalars && i == 0);
        if (overlap) HIP_TRY(issue(i + 1));
        const Piece &p = pieces[i];
        const double *src = b->h_pin + (i % 2) * half;
        if (p.is_nodes) {
            const int64_t base = p.off;
            b->pool->run(p.s1 - p.s0, [&](int64_t q0, int64_t q1) {
                for (int64_t s = p.s0 + q0; s < p.s0 + q1; s++)
                    memcpy(state + b->h_first_slot[s], src + (b->h_node_off[s] - base), (size_t)b->h_node_count[s] * sizeof(double));
            });
        } else {
            if (what & HEAT_OUT_SURFACE_SCALARS)
                b->pool->run(S, [&](int64_t s0, int64_t s1) {
                    for (int64_t s = s0; s < s1; s++) {
                        const double *v = src + 4 * s;  // hs_f, hs_b, flow_f, flow_b
                        state[b->h_out_slots[0][s]] = v[0];
                        state[b->h_out_slots[1][s]] = v[1];
                        state[b->h_out_slots[2][s]] = v[2];
                        state[b->h_out_slots[3][s]] = v[3];
                    }
                });
            if (what & HEAT_OUT_ZONE_TEMPERATURES)
                for (int64_t z = 0; z < Z; z++)
                    if (b->h_owned[z]) state[b->h_zone_slot_h[z]] = src[4 * S - sc_off + z];
        }
        if (!overlap && i + 1 < pieces.size()) HIP_TRY(issue(i + 1));
    }
    if (delivers_zones) b->host_zones_stale = false;  // (the caller's zone slots are the device's again)
    return HEAT_OK;
}

// Room for the weather of a march call of n_sub sub-timesteps, in pinned and in device memory (heat_batch_set_weather; the
// series march sizes it once, before its first step).
static int grow_weather(heat_batch *b, int32_t n_sub) {
    if ((size_t)n_sub <= b->weather_cap) return HEAT_OK;
    const size_t n_sites = (size_t)b->n_sites;
    HIP_TRY(hipStreamSynchronize(b->stream));  // kernels in flight read the device array that is about to go
    if (b->h_weather) HIP_TRY(hipHostFree(b->h_weather));
    b->h_weather = nullptr;
    // (per site; several sites: exactly the call's length — the head kernel copies every site's records, padding
    // included, so a batch whose calls keep one length copies nothing it does not use)
    const size_t cap = n_sites > 1 ? (size_t)n_sub : std::max<size_t>((size_t)n_sub, 64);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&b->h_weather), n_sites * cap * sizeof(StepWeather)));
    HIP_TRY(b->d_weather.alloc(n_sites * cap));
    b->weather_cap = cap;
    b->sa.wstride = (int32_t)cap;
    if (b->graph_exec) {  // the captured graph holds the old pointer (and the old stride)
        (void)hipGraphExecDestroy(b->graph_exec);
        b->graph_exec = nullptr;
    }
    return HEAT_OK;
}

int heat_batch_set_weather(heat_batch *b, const heat_weather *weather, int32_t n_sub, const double *zone_a0,
                           const double *zone_b0) {
    if (!b || (!weather && n_sub > 0)) return fail(HEAT_E_INVALID_ARG, "NULL argument");
    if (n_sub < 0) return fail(HEAT_E_INVALID_ARG, "n_sub < 0");
    int rc = select_device(b);
    if (rc) return rc;
    // The pinned staging buffers are free again once the previous call's copies have run — they sit at the head of
    // that call's work, so this does not wait for the march itself: consecutive marches queue up back to back.
    const size_t n_sites = (size_t)b->n_sites;
    // (weather sites: n_sub * n_sites records in pinned and device memory, 32 bytes each)
    constexpr int64_t kMaxWeatherRecords = (int64_t)1 << 24;
    if (n_sites > 1 && (int64_t)n_sub * (int64_t)n_sites > kMaxWeatherRecords)
        return fail(HEAT_E_INVALID_ARG, "n_sub %d x %d sites = %lld weather records, more than %lld per call", n_sub, (int)n_sites,
                    (long long)n_sub * (long long)n_sites, (long long)kMaxWeatherRecords);
    if (b->staged) HIP_TRY(hipEventSynchronize(b->ev_staged));
    {
        const int rc2 = grow_weather(b, n_sub);
        if (rc2) return rc2;
    }
    // sin/cos of the wind direction as is_windward takes them (surface.rs:40). The caller's records are sub-timestep-major
    // ([k * n_sites + s]); the device's are site-major ([s * weather_cap + k], layout.hpp).
    for (size_t st = 0; st < n_sites; st++)
        for (int i = 0; i < n_sub; i++) {
            const heat_weather &w = weather[(size_t)i * n_sites + st];
            b->h_weather[st * b->weather_cap + i] = to_step_weather(w);
        }
    b->n_weather = n_sub;
    const int64_t Z = b->n_zones;
    for (int64_t z = 0; z < Z; z++) {
        b->h_zone_ab[z] = zone_a0 ? zone_a0[z] : 0.0;
        b->h_zone_ab[Z + z] = zone_b0 ? zone_b0[z] : 0.0;
    }
    // weather, a0, b0 and the sub-timestep counter in one launch that reads the pinned buffers itself. Many sites' records
    // (1 MB and more) go by DMA ahead of it: measured on MI355X (tools/sites.py, copy + head kernel + one round trip), 82 000
    // records took 73 and 93 us by DMA (two runs) against 84 us read by the kernel, 5 000 records 29 against 22 us.
    // HEAT_AMD_WEATHER_KERNEL_COPY=1 (measurement) keeps every copy in the kernel.
    static const bool kernel_copy = getenv("HEAT_AMD_WEATHER_KERNEL_COPY") != nullptr;
    constexpr int kDmaMinRecords = 32768;
    int n_records = n_sub > 0 ? (int)((n_sites - 1) * b->weather_cap) + n_sub : 0;
    if (n_sites > 1 && n_records >= kDmaMinRecords && !kernel_copy) {
        HIP_TRY(hipMemcpyAsync(b->d_weather.p, b->h_weather, (size_t)n_records * sizeof(StepWeather), hipMemcpyHostToDevice,
                               b->stream));
        n_records = 0;
    }
    launch_begin_march(b->h_weather, b->d_weather.p, n_sub, n_records, b->h_zone_ab, b->d_zone_a0.p, b->d_zone_b0.p, (int)Z, b->d_step.p,
                       b->stream);
    if (!b->ev_staged) HIP_TRY(hipEventCreateWithFlags(&b->ev_staged, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(b->ev_staged, b->stream));
    b->staged = true;
    HIP_TRY(hipGetLastError());
    return HEAT_OK;
}

int heat_batch_step_surfaces(heat_batch *b, int32_t sub_step) {
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    if (sub_step < 0 || sub_step >= b->n_weather) return fail(HEAT_E_INVALID_ARG, "sub_step %d outside the weather set (%d)", sub_step, b->n_weather);
    int rc = select_device(b);
    if (rc) return rc;
    b->host_zones_stale = true;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    if (b->timing) {
        e0 = next_event(b); e1 = next_event(b); e2 = next_event(b);
        if (!e0 || !e1 || !e2) return fail(HEAT_E_DEVICE, "hipEventCreate failed");
        HIP_TRY(hipEventRecord(e0, b->stream));
    }
    enqueue_surfaces(b, sub_step);
    if (b->timing) HIP_TRY(hipEventRecord(e1, b->stream));
    enqueue_zones(b, b->shared_set ? 2 : 1);  // partial (a, b) of this rank's surfaces
    if (b->timing) {
        HIP_TRY(hipEventRecord(e2, b->stream));
        b->ev_triples.push_back({e0, e1, e2});
    }
    HIP_TRY(hipGetLastError());
    return HEAT_OK;
}

double *heat_batch_zone_partials(heat_batch *b) { return b ? b->partial_ptr : nullptr; }

int heat_batch_use_partials(heat_batch *b, double *partials_dev) {
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    b->partial_ptr = partials_dev ? partials_dev : b->d_partial.p;
    return HEAT_OK;
}

int heat_batch_touched_zones(const heat_batch *b, uint8_t *mask) {
    if (!b || (!mask && b->n_zones > 0)) return fail(HEAT_E_INVALID_ARG, "NULL argument");
    for (int64_t z = 0; z < b->n_zones; z++) mask[z] = b->h_touched[z];
    return HEAT_OK;
}

int heat_batch_set_shared_zones(heat_batch *b, const int32_t *shared_zone, int32_t n_shared) {
    static const int32_t none = 0;
    if (n_shared == 0 && !shared_zone) shared_zone = &none;
    if (!b || n_shared < 0 || !shared_zone) return fail(HEAT_E_INVALID_ARG, "bad argument");
    int rc = select_device(b);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    std::vector<int32_t> slot(b->n_zones, -1), zl, sz(shared_zone, shared_zone + n_shared);
    for (int32_t i = 0; i < n_shared; i++) {
        if (sz[i] < 0 || sz[i] >= b->n_zones) return fail(HEAT_E_SIZE, "shared zone %d out of range", sz[i]);
        slot[sz[i]] = i;
    }
    for (int64_t z = 0; z < b->n_zones; z++) if (b->h_owned[z]) zl.push_back((int32_t)z);
    HIP_TRY(b->d_slot_of.upload(slot));
    HIP_TRY(b->d_zlist.upload(zl));
    HIP_TRY(b->d_shared_zone.upload(sz));
    b->n_touched = (int)zl.size();
    b->n_shared = n_shared;
    b->shared_set = true;
    if (b->comm) HIP_TRY(b->d_gathered.zeros((size_t)b->n_ranks * 2 * std::max(n_shared, 1)));
    if (b->partial_ptr == b->d_partial.p && (size_t)2 * n_shared > b->d_partial.n)
        return fail(HEAT_E_SIZE, "partials buffer too small");

    // ---- cluster-resident march: demote the workgroups that own a shared zone (from the create-time plan) ----
    // A demoted workgroup's tiles move, as descriptors, behind the streamed tiles of their class; the remaining
    // workgroups keep their slot lists (those are relative to the block's first tile).
    b->any_fused = false;
    int64_t n_fused_now = 0;
    std::vector<uint8_t> zone_fused(b->n_zones, 0);
    auto owns_shared_zone = [&](const FusedBlock &fb) {
        for (int j = 0; j < fb.n_zones; j++)
            if (slot[b->h_fzones[fb.first_zone + j]] >= 0) return true;
        return false;
    };
    // small-surface tiles of the workgroups (general layout): [plain | streamed with cavities | DEMOTED | kept | catch-all]
    std::vector<int32_t> new_first_small(b->h_gen_tiles0.size() + 1, 0);
    {
        const std::vector<GeneralTile> &g0 = b->h_gen_tiles0;
        const int head = b->n_small_plain_tiles + b->n_smallcav_stream_tiles0;
        std::vector<GeneralTile> g(g0.begin(), g0.begin() + head);
        int n_demoted = 0;
        for (int pass = 0; pass < 2; pass++)
            for (int c = 0; c < kNumFast; c++)
                for (int g2 = 0; g2 < 4; g2++)
                    for (const FusedBlock &fb : b->h_fblocks0[c][g2]) {
                        if (fb.n_small <= 0 || (pass == 0) != owns_shared_zone(fb)) continue;
                        new_first_small[fb.first_small] = (int32_t)g.size();
                        g.insert(g.end(), g0.begin() + fb.first_small, g0.begin() + fb.first_small + fb.n_small);
                        if (pass == 0) n_demoted += fb.n_small;
                    }
        g.insert(g.end(), g0.begin() + b->n_small_tiles, g0.end());
        b->n_smallcav_stream_tiles = b->n_smallcav_stream_tiles0 + n_demoted;
        HIP_TRY(b->d_gen_tiles.upload(g));
        b->h_gen_tiles_cur = g;
    }
    // (teams are never demoted: a zone shared with another rank cannot also be exchanged inside a team)
    for (int c = 0; c < kNumFast; c++)
        for (const FusedBlock &fb : b->h_team_blocks0[c])
            if (owns_shared_zone(fb))
                return fail(HEAT_E_INVALID_ARG, "zone shared between ranks belongs to a cluster marched by a team of workgroups "
                                                "(create the batch with no_fusion = 1, or do not share that zone)");
    for (int c = 0; c < kNumFast; c++) {
        const std::vector<FastTile> &t0 = b->h_tiles0[c];
        bool any = !b->h_team_blocks0[c].empty();
        for (int g2 = 0; g2 < 4; g2++) any = any || !b->h_fblocks0[c][g2].empty();
        if (!any) continue;
        std::vector<FastTile> t(t0.begin(), t0.begin() + b->n_stream_tiles0[c]);
        std::vector<FusedBlock> keep[4];
        for (int pass = 0; pass < 2; pass++)          // pass 0: demoted blocks' tiles, pass 1: kept blocks' tiles
            for (int g2 = 0; g2 < 4; g2++)
                for (const FusedBlock &fb : b->h_fblocks0[c][g2]) {
                    if ((pass == 0) != owns_shared_zone(fb)) continue;
                    FusedBlock nb = fb;
                    nb.first_tile = (int32_t)t.size();
                    if (fb.n_small > 0) nb.first_small = new_first_small[fb.first_small];
                    t.insert(t.end(), t0.begin() + fb.first_tile, t0.begin() + fb.first_tile + fb.n_tiles);
                    if (pass == 1) {
                        keep[g2].push_back(nb);
                        for (int j = 0; j < fb.n_zones; j++) zone_fused[b->h_fzones[fb.first_zone + j]] = 1;
                        for (int q = 0; q < fb.n_small; q++) n_fused_now += b->h_gen_tiles0[fb.first_small + q].G;
                    }
                }
        int n_kept_tiles = 0;
        {   // the teams' tiles stay where they are in the order of things: behind the kept workgroups' tiles
            std::vector<FusedBlock> tb = b->h_team_blocks0[c];
            for (FusedBlock &fb : tb) {
                const int first = (int)t.size();
                t.insert(t.end(), t0.begin() + fb.first_tile, t0.begin() + fb.first_tile + fb.n_tiles);
                fb.first_tile = first;
                n_kept_tiles += fb.n_tiles;
                for (int j = 0; j < fb.n_zones; j++) zone_fused[b->h_fzones[fb.first_zone + j]] = 1;
                for (int q = 0; q < fb.n_tiles; q++) n_fused_now += t[fb.first_tile + q].G;
            }
            b->h_team_blocks[c] = tb;
            HIP_TRY(b->d_team_blocks[c].upload(tb));
            b->any_fused = b->any_fused || !tb.empty();
        }
        for (int g2 = 0; g2 < 4; g2++) {
            for (const FusedBlock &fb : keep[g2]) {
                n_kept_tiles += fb.n_tiles;
                for (int q = 0; q < fb.n_tiles; q++) n_fused_now += t[fb.first_tile + q].G;
            }
            b->h_fblocks[c][g2] = keep[g2];
            HIP_TRY(b->d_fblocks[c][g2].upload(keep[g2]));
            b->any_fused = b->any_fused || !keep[g2].empty();
        }
        b->n_stream_tiles[c] = (int)t.size() - n_kept_tiles;
        HIP_TRY(b->d_fast_tiles[c].upload(t));
        b->h_tiles_cur[c] = t;
    }
    {
        std::vector<int32_t> szl, tz;
        for (int64_t z = 0; z < b->n_zones; z++) {
            b->h_zone_block[z] = zone_fused[z] ? 0 : -1;
            if (!zone_fused[z] && b->h_owned[z]) szl.push_back((int32_t)z);
        }
        b->n_stream_zones = (int)szl.size();
        HIP_TRY(b->d_stream_zones.upload(szl));
        for (int32_t z : zl) if (!zone_fused[z]) tz.push_back(z);
        b->n_touched_stream = (int)tz.size();
        HIP_TRY(b->d_zlist_stream.upload(tz));
    }
    b->n_fused_surfaces = n_fused_now;
    rc = rebuild_unified(b);
    if (rc) return rc;
    if (b->graph_exec) {  // the captured sub-timestep graph holds the old tile counts
        HIP_TRY(hipStreamSynchronize(b->stream));
        (void)hipGraphExecDestroy(b->graph_exec);
        b->graph_exec = nullptr;
    }
    HIP_TRY(hipDeviceSynchronize());  // (the uploads above went through the null stream; the batch's streams do not wait for it)
    return HEAT_OK;
}

int heat_comm_available(void) {
    if (rccl()) return HEAT_OK;
    return fail(HEAT_E_COMM, "cannot load librccl.so.1: %s", rccl_error().c_str());
}

int heat_comm_unique_id(uint8_t id[HEAT_COMM_ID_BYTES]) {
    if (!id) return fail(HEAT_E_INVALID_ARG, "NULL argument");
    Rccl *r = rccl();
    if (!r) return fail(HEAT_E_COMM, "cannot load librccl.so.1: %s", rccl_error().c_str());
    static_assert(sizeof(ncclUniqueId) == HEAT_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    RCCL_TRY(r, r->GetUniqueId(&u));
    memcpy(id, &u, sizeof u);
    return HEAT_OK;
}

int heat_batch_set_owned_zones(heat_batch *b, const uint8_t *owned) {
    if (!b || (!owned && b->n_zones > 0)) return fail(HEAT_E_INVALID_ARG, "NULL argument");
    for (int64_t z = 0; z < b->n_zones; z++) b->h_owned[z] = (owned[z] || b->h_touched[z]) ? 1 : 0;
    if (b->shared_set) {  // the zone lists follow
        std::vector<int32_t> sz;
        int rc = select_device(b);
        if (rc) return rc;
        HIP_TRY(hipMemcpy((sz.resize(b->n_shared), sz.data()), b->d_shared_zone.p, (size_t)b->n_shared * sizeof(int32_t),
                          hipMemcpyDeviceToHost));
        return heat_batch_set_shared_zones(b, sz.data(), b->n_shared);
    }
    std::vector<int32_t> szl;
    for (int64_t z = 0; z < b->n_zones; z++)
        if (b->h_zone_block[z] < 0 && b->h_owned[z]) szl.push_back((int32_t)z);
    b->n_stream_zones = (int)szl.size();
    HIP_TRY(b->d_stream_zones.upload(szl));
    return HEAT_OK;
}

int heat_batch_comm_init(heat_batch *b, const uint8_t id[HEAT_COMM_ID_BYTES]) {
    return heat_batch_comm_init_ex(b, id, nullptr, 0);
}

int heat_batch_comm_init_ex(heat_batch *b, const uint8_t id[HEAT_COMM_ID_BYTES], const int32_t *extra_shared,
                            int32_t n_extra) {
    if (!b || !id || n_extra < 0 || (n_extra > 0 && !extra_shared)) return fail(HEAT_E_INVALID_ARG, "bad argument");
    if (b->comm) return fail(HEAT_E_INVALID_ARG, "the batch already has a communicator");
    const int64_t Z = b->n_zones;
    // (checked before anything collective happens: a bad list must not leave this rank outside a communicator the
    // other ranks have already agreed on)
    for (int32_t i = 0; i < n_extra; i++)
        if (extra_shared[i] < 0 || extra_shared[i] >= Z) return fail(HEAT_E_SIZE, "shared zone %d out of range", extra_shared[i]);
    Rccl *r = rccl();
    if (!r) return fail(HEAT_E_COMM, "cannot load librccl.so.1: %s", rccl_error().c_str());
    int rc = select_device(b);
    if (rc) return rc;
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    RCCL_TRY(r, r->CommInitRank(&b->comm, b->n_ranks, u, b->rank));
    // From here on a failure returns the batch to "sharded batch without a communicator": the communicator goes, so
    // that a retry is possible and a march cannot take the no-exchange path on zones other ranks share.
    const std::vector<uint8_t> owned_before = b->h_owned;
    auto agree = [&]() -> int {
        // agree on the zones more than one rank touches: sum of the touched masks
        std::vector<int32_t> mask(std::max<int64_t>(Z, 1), 0);
        for (int64_t z = 0; z < Z; z++) mask[z] = b->h_touched[z];
        DevBuf<int32_t> d_mask;
        HIP_TRY(d_mask.upload(mask));
        RCCL_TRY(r, r->AllReduce(d_mask.p, d_mask.p, mask.size(), ncclInt32, ncclSum, b->comm, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        HIP_TRY(hipMemcpy(mask.data(), d_mask.p, mask.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<uint8_t> is_shared(std::max<int64_t>(Z, 1), 0);
        for (int64_t z = 0; z < Z; z++) {
            is_shared[z] = mask[z] >= 2;
            // a zone no rank faces is finished by rank z % n_ranks (it still follows a0 / b0: model.rs:410-423)
            b->h_owned[z] = (b->h_touched[z] || (mask[z] == 0 && z % b->n_ranks == b->rank)) ? 1 : 0;
        }
        for (int32_t i = 0; i < n_extra; i++) is_shared[extra_shared[i]] = 1;  // (tests, rehearsals of the exchange)
        std::vector<int32_t> shared;
        for (int64_t z = 0; z < Z; z++) if (is_shared[z]) shared.push_back((int32_t)z);
        return heat_batch_set_shared_zones(b, shared.data(), (int32_t)shared.size());
    };
    rc = agree();
    if (rc) {
        const std::string why = heat::last_error();
        (void)r->CommDestroy(b->comm);
        b->comm = nullptr;
        b->shared_set = false;
        b->n_shared = 0;
        b->h_owned = owned_before;
        return fail(rc, "%s", why.c_str());
    }
    return HEAT_OK;
}

int32_t heat_batch_n_shared_zones(const heat_batch *b) { return (b && b->shared_set) ? b->n_shared : 0; }

int32_t heat_batch_comm_ranks(const heat_batch *b) { return (b && b->comm) ? b->n_ranks : 0; }

int heat_batch_comm_destroy(heat_batch *b) {
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    if (!b->comm) return HEAT_OK;
    int rc = select_device(b);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    Rccl *r = rccl();
    if (r) (void)r->CommDestroy(b->comm);
    b->comm = nullptr;
    // back to "sharded batch without a communicator": the caller agrees on the shared zones again by its own means
    // (heat_batch_set_owned_zones / heat_batch_set_shared_zones) or gives the batch a new communicator
    b->shared_set = false;
    b->n_shared = 0;
    b->d_gathered.release();
    return HEAT_OK;
}

int heat_batch_step_zones(heat_batch *b, const double *gathered_dev, int32_t n_blocks) {
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    if (n_blocks < 1) return fail(HEAT_E_INVALID_ARG, "n_blocks < 1");
    int rc = select_device(b);
    if (rc) return rc;
    const double *g = gathered_dev ? gathered_dev : b->partial_ptr;
    if (b->shared_set)
        launch_zone_update_shared(g, n_blocks, b->d_shared_zone.p, b->n_shared, b->d_zone_a0.p, b->d_zone_b0.p,
                                  b->d_zone_vol.p, b->d_zone_T.p, b->dt, b->d_flags.p, b->stream);
    else
        launch_zone_update(g, n_blocks, b->d_zone_a0.p, b->d_zone_b0.p, b->d_zone_vol.p, b->d_zone_T.p,
                           (int)b->n_zones, b->dt, b->d_step.p, b->d_flags.p, b->stream);
    HIP_TRY(hipGetLastError());
    return HEAT_OK;
}

static int march_body(heat_batch *b, int32_t n_sub);

int heat_batch_march_resident(heat_batch *b, const heat_weather *weather, int32_t n_sub, const double *zone_a0,
                              const double *zone_b0) {
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    // A sharded batch needs a collective only for zones it shares with another rank: a partition along the clusters
    // (heat_partition) shares none, and every rank then marches on its own.
    const bool exchange = b->shared_set && b->n_shared > 0;
    if (b->n_ranks > 1 && !b->comm && (exchange || !b->shared_set))
        return fail(HEAT_E_INVALID_ARG, "sharded batch without a communicator: call heat_batch_comm_init, or drive it "
                                        "with heat_batch_step_surfaces / heat_batch_step_zones and your own collective "
                                        "(a batch that shares no zone — heat_batch_set_shared_zones(b, NULL, 0) — needs neither)");
    const int rc = heat_batch_set_weather(b, weather, n_sub, zone_a0, zone_b0);
    if (rc) return rc;
    return march_body(b, n_sub);
}

// The body of a march call: the n_sub sub-timesteps whose weather, zone terms and counter the head has put on the device
// (heat_batch_set_weather for heat_batch_march_resident; the head of a series step for heat_batch_march_series).
static int march_body(heat_batch *b, int32_t n_sub) {
    const bool exchange = b->shared_set && b->n_shared > 0;
    int rc = HEAT_OK;
    // A march of no sub-timestep (model.rs:369: the loop body never runs) is the head kernel and nothing else: the
    // graph branch below must never capture or replay an empty graph.
    if (n_sub == 0) return HEAT_OK;
    b->host_zones_stale = true;  // (until a download delivers the zones again)
    if (b->comm && exchange) {
        // Sharded sub-timestep, everything in order on the batch's stream (no cross-queue dependency anywhere):
        // this rank's surfaces -> zones only this rank touches finished, partial (a, b) of the shared zones ->
        // RCCL all-gather of the [2][n_shared] blocks over xGMI -> shared zones updated from the blocks, summed
        // in rank order (identical bits on every rank).
        Rccl *r = rccl();
        if (!r) return fail(HEAT_E_COMM, "RCCL is not loaded");
        MarchGuard guard(b);
        b->partial_ptr = b->d_partial.p;
        // The clusters that own no shared zone march beside the exchange loop, in one launch per class on a side
        // stream: only the few surfaces around the shared zones go through kernel -> all-gather -> kernel every
        // sub-timestep, and that chain is shorter than the fused march it runs next to.
        const bool fused = b->any_fused && b->fusion_on && n_sub >= (b->n_surf <= 8192 ? 1 : kFusedMinSubsteps) &&
                           b->fused_stream != nullptr;
        if (fused) {
            hipStream_t fs = b->fused_stream;
            HIP_TRY(hipEventRecord(b->ev_fork, b->stream));
            HIP_TRY(hipStreamWaitEvent(fs, b->ev_fork, 0));
            guard.forked = true;
            hipEvent_t f0 = nullptr, f1 = nullptr;
            if (b->timing) {
                f0 = next_event(b); f1 = next_event(b);
                if (!f0 || !f1) return fail(HEAT_E_DEVICE, "hipEventCreate failed");
                HIP_TRY(hipEventRecord(f0, fs));
            }
            rc = enqueue_fused(b, n_sub, fs);
            if (rc) return rc;
            if (b->timing) {
                HIP_TRY(hipEventRecord(f1, fs));
                b->ev_fused_pairs.push_back({f0, f1, n_sub});
            }
            HIP_TRY(hipEventRecord(b->ev_fused, fs));
        }
        for (int i = 0; i < n_sub; i++) {
            hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
            if (b->timing) {
                e0 = next_event(b); e1 = next_event(b); e2 = next_event(b);
                if (!e0 || !e1 || !e2) return fail(HEAT_E_DEVICE, "hipEventCreate failed");
                HIP_TRY(hipEventRecord(e0, b->stream));
            }
            enqueue_surfaces(b, i, fused);
            if (b->timing) HIP_TRY(hipEventRecord(e1, b->stream));
            enqueue_zones(b, fused ? 4 : 2);
            if (b->n_shared > 0) {
                RCCL_TRY(r, r->AllGather(b->d_partial.p, b->d_gathered.p, (size_t)2 * b->n_shared, ncclDouble, b->comm,
                                         b->stream));
                launch_zone_update_shared(b->d_gathered.p, b->n_ranks, b->d_shared_zone.p, b->n_shared, b->d_zone_a0.p,
                                          b->d_zone_b0.p, b->d_zone_vol.p, b->d_zone_T.p, b->dt, b->d_flags.p, b->stream);
            }
            if (b->timing) {
                HIP_TRY(hipEventRecord(e2, b->stream));
                b->ev_triples.push_back({e0, e1, e2});
            }
        }
        if (fused) {
            HIP_TRY(hipStreamWaitEvent(b->stream, b->ev_fused, 0));
            guard.joined = true;
        }
        HIP_TRY(hipGetLastError());
        return HEAT_OK;
    }
    // Cluster-resident march: the fused workgroups march all n_sub sub-timesteps in one launch per class (on a
    // side stream when other surfaces are streamed beside them); whatever is not fused is streamed as before.
    // (a resident call costs about 150 us + 59 us per sub-timestep at 1 M x 32 — round 3, tools/short_calls.py: 262 / 144 / 108 /
    // 88 us per sub-timestep at 1 / 2 / 3 / 5 per call against 206 for the same batch streamed: resident from two on)
    const bool fused = b->any_fused && b->fusion_on && n_sub >= (b->n_surf <= 8192 ? 1 : kFusedMinSubsteps);
    bool streamed = !fused;
    if (fused) {
        for (int c = 0; c < kNumFast; c++) streamed = streamed || b->n_stream_tiles[c] > 0;
        streamed = streamed || b->n_gen_tiles > 0 || b->n_stream_zones > 0;
    }
    hipStream_t fs = b->stream;
    MarchGuard guard(b);
    if (fused) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        // A small batch runs its streamed remainder beside the fused launch (both are latency-bound and leave the chip
        // mostly empty); a large one runs them one after the other on the batch's stream: side by side the streamed
        // kernels wait for wavefront slots the fused launch holds for its whole duration.
        if (streamed && b->fused_stream != nullptr && b->n_surf <= 8192) {
            fs = b->fused_stream;
            HIP_TRY(hipEventRecord(b->ev_fork, b->stream));
            HIP_TRY(hipStreamWaitEvent(fs, b->ev_fork, 0));
            guard.forked = true;
        }
        if (b->timing) {
            e0 = next_event(b); e1 = next_event(b);
            if (!e0 || !e1) return fail(HEAT_E_DEVICE, "hipEventCreate failed");
            HIP_TRY(hipEventRecord(e0, fs));
        }
        rc = enqueue_fused(b, n_sub, fs, streamed && fs != b->stream);
        if (rc) return rc;
        if (b->timing) {
            HIP_TRY(hipEventRecord(e1, fs));
            b->ev_fused_pairs.push_back({e0, e1, n_sub});
        }
    }
    // (a sharded batch finishes the zones it owns only; beside a cluster-resident march only the zones no workgroup owns)
    const int zmode = fused ? 3 : (b->n_ranks > 1 ? 5 : 0);
    if (!streamed) {
        // nothing to stream
    } else if (b->timing && (b->timing_calls++ % b->timing_every) == 0) {
        for (int i = 0; i < n_sub; i++) {
            hipEvent_t e0 = next_event(b), e1 = next_event(b), e2 = next_event(b);
            if (!e0 || !e1 || !e2) return fail(HEAT_E_DEVICE, "hipEventCreate failed");
            HIP_TRY(hipEventRecord(e0, b->stream));
            enqueue_surfaces(b, -1, fused);
            HIP_TRY(hipEventRecord(e1, b->stream));
            enqueue_zones(b, zmode);
            HIP_TRY(hipEventRecord(e2, b->stream));
            b->ev_triples.push_back({e0, e1, e2});
        }
    } else if (b->use_graph) {
        // One graph holds a whole march call's sub-timesteps (up to 32; the usual call — ThermalModel::march runs a fixed
        // dt_subdivisions of them — replays it once): inside a graph consecutive kernels follow each other closer than
        // consecutive graph launches do. A call of another length re-captures; longer ones replay blocks.
        static const int per_graph_env = getenv("HEAT_AMD_GRAPH_SUBSTEPS") ? atoi(getenv("HEAT_AMD_GRAPH_SUBSTEPS")) : 0;
        // (a caller whose calls keep changing length gets the one-sub-timestep graph, which fits every length)
        const int want = std::max(1, b->graph_recaptures > 8 ? 1 : (per_graph_env > 0 ? std::min(per_graph_env, n_sub) : std::min(n_sub, 32)));
        if (!b->graph_exec || b->graph_fused != fused || b->graph_subs <= 0 || (b->graph_subs != want && n_sub % b->graph_subs != 0)) {
            if (b->graph_exec && b->graph_fused == fused) b->graph_recaptures++;
            // (a call of another length: the graph of the calls before may still be running — it goes only when it is done)
            if (b->graph_exec) HIP_TRY(hipStreamSynchronize(b->stream));
            if (b->graph_exec) { (void)hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
            if (b->graph) { (void)hipGraphDestroy(b->graph); b->graph = nullptr; }
            HIP_TRY(hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal));
            b->capturing = true;
            for (int i = 0; i < want; i++) {
                enqueue_surfaces(b, -1, fused);
                enqueue_zones(b, zmode);
            }
            b->capturing = false;
            HIP_TRY(hipStreamEndCapture(b->stream, &b->graph));
            HIP_TRY(hipGraphInstantiate(&b->graph_exec, b->graph, nullptr, nullptr, 0));
            b->graph_fused = fused;
            b->graph_subs = want;
        }
        int done = 0;
        for (; done + b->graph_subs <= n_sub; done += b->graph_subs) HIP_TRY(hipGraphLaunch(b->graph_exec, b->stream));
        for (; done < n_sub; done++) {  // (a remainder shorter than the graph: plain launches)
            enqueue_surfaces(b, -1, fused);
            enqueue_zones(b, zmode);
        }
    } else {
        for (int i = 0; i < n_sub; i++) {
            enqueue_surfaces(b, -1, fused);
            enqueue_zones(b, zmode);
        }
    }
    if (fused && fs != b->stream) {
        HIP_TRY(hipEventRecord(b->ev_fused, fs));
        HIP_TRY(hipStreamWaitEvent(b->stream, b->ev_fused, 0));
        guard.joined = true;
    }
    HIP_TRY(hipGetLastError());
    return HEAT_OK;
}

// The body of a step of a series with ideal loads (heat_ideal_loads): every sub-timestep streamed — the surface kernels, the
// zone sums as partials (k_zones, mode 1), the zone update with the rule (k_zone_update_ideal) — in plain launches on the
// batch's stream. The cluster-resident march balances its zones in LDS and cannot host the rule; the batch's fusion setting
// and the graph cache of the plain calls are not touched.
static int march_body_ideal(heat_batch *b, int32_t n_sub, const IdealLoadsDev &ild) {
    if (n_sub == 0) return HEAT_OK;
    b->host_zones_stale = true;
    MarchGuard guard(b);
    b->partial_ptr = b->d_partial.p;  // (a caller's buffer, heat_batch_use_partials, is left alone; restored by the guard)
    for (int i = 0; i < n_sub; i++) {
        enqueue_surfaces(b, -1);
        enqueue_zones(b, 1);
        launch_zone_update_ideal(b->d_partial.p, b->d_zone_a0.p, b->d_zone_b0.p, b->d_zone_vol.p, b->d_zone_T.p, (int)b->n_zones, b->dt,
                                 b->d_step.p, b->d_flags.p, ild, b->stream);
    }
    HIP_TRY(hipGetLastError());
    return HEAT_OK;
}

int heat_batch_synchronize(heat_batch *b) {
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    int rc = select_device(b);
    if (rc) return rc;
    // The failure flags travel to pinned memory at the end of the stream's work, so that ONE wait covers march and flags
    // (a synchronous copy behind the stream's wait is a second round trip to the device: 10-20 us of every short call).
    if (!b->h_flags) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&b->h_flags), 4 * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(b->h_flags, b->d_flags.p, 4 * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    int f[4] = {b->h_flags[0], b->h_flags[1], b->h_flags[2], b->h_flags[3]};
    if (f[0]) {
        unsigned long long where;
        memcpy(&where, f + 2, sizeof where);
        HIP_TRY(hipMemset(b->d_flags.p, 0, 2 * sizeof(int)));
        HIP_TRY(hipMemset(b->d_flags.p + 2, 0xff, 2 * sizeof(int)));
        HIP_TRY(hipStreamSynchronize(nullptr));  // (the batch's streams do not wait for the null stream)
        // the first place (smallest number) and the kind that was seen there
        const int kinds = (int)(where & 0xff);
        const int64_t idx = (int64_t)(where >> 8);
        const bool zone = (kinds & FLAG_NAN_ZONE) && !(kinds & (FLAG_NAN_HS | FLAG_NAN_NOMASS | FLAG_UNREACHABLE));
        b->fail_kind = flags_to_status(kinds ? kinds : f[0]);
        b->fail_index = zone ? idx : ((idx >= 0 && idx < (int64_t)b->h_orig_of.size()) ? b->h_orig_of[idx] : -1);
        const int rc2 = flags_to_status(f[0]);
        const std::string what = heat::last_error();
        return fail(rc2, "%s; first seen at %s %lld", what.c_str(), zone ? "zone" : "surface", (long long)b->fail_index);
    }
    return HEAT_OK;
}

int heat_batch_failed_surface(const heat_batch *b, int64_t *index, int32_t *kind) {
    if (!b || !index || !kind) return fail(HEAT_E_INVALID_ARG, "NULL argument");
    *index = b->fail_index;
    *kind = b->fail_kind;
    return HEAT_OK;
}

int heat_batch_march(heat_batch *b, double *state, size_t n_state, const heat_weather *weather, int32_t n_sub,
                     const double *zone_a0, const double *zone_b0) {
    return heat_batch_march_ex(b, state, n_state, weather, n_sub, zone_a0, zone_b0, HEAT_OUT_ALL);
}

int heat_batch_march_ex(heat_batch *b, double *state, size_t n_state, const heat_weather *weather, int32_t n_sub,
                        const double *zone_a0, const double *zone_b0, int32_t what) {
    int rc = heat_batch_upload_inputs(b, state, n_state);
    if (rc) return rc;
    rc = heat_batch_march_resident(b, weather, n_sub, zone_a0, zone_b0);
    if (rc) return rc;
    rc = heat_batch_synchronize(b);
    if (rc) return rc;
    return download_impl(b, state, n_state, what, true);
}

// heat_batch_march_series*: the table of contents of a series march. A term that is absent (its argument NULL, or naming
// nothing: loads without a term, no ideal load, no mode bit, no aperture, no path, no shade, no receiver, no driven side) is
// the series without it: the same launches. no_trace_ok: a NULL trace means "record none" instead of a refusal.
static int march_series_impl(heat_batch *b, const SeriesCall &c) {
    if (c.failed_step) *c.failed_step = -1;
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    const heat_series *s = c.s;
    // ---- everything that needs no device (heat_series_check's checks, on the batch's own copies of the slots) ----
    SeriesModel m;
    m.n_surfaces = b->n_surf, m.n_zones = b->n_zones;
    m.first_node_slot = b->h_first_slot.data(), m.node_count = b->h_node_count.data();
    for (int a = 0; a < 4; a++) m.out_slot[a] = b->h_out_slots[a].data();
    m.zone_slot = b->h_zone_slot_h.data();
    if (!b->resolver) b->resolver = new SlotResolver(m);
    std::vector<ResolvedSlot> group_entry;
    std::vector<int32_t> load_of_zone;
    const int32_t *const side_kind[2] = {b->h_kind[0].data(), b->h_kind[1].data()};
    SkyTerm sky;
    int rc;
    if ((rc = check_series(m, *b->resolver, b->n_sites, s, heat::last_error()))) return rc;
    if ((rc = check_zone_loads(b->n_zones, s->n_channels, c.l, heat::last_error()))) return rc;
    if ((rc = check_series_report(*b->resolver, c.l, c.r, heat::last_error(), &group_entry))) return rc;
    if ((rc = check_ideal_loads(b->n_zones, s->n_channels, c.il, heat::last_error(), &load_of_zone))) return rc;
    if ((rc = check_sky(b->n_surf, s, c.sky, heat::last_error(), &sky.bits))) return rc;
    if (b->n_ranks > 1) return fail(HEAT_E_INVALID_ARG, "a sharded batch (n_ranks = %d) cannot march a series", b->n_ranks);
    // (behind the shard's refusal: the gains number the surfaces of the caller's model, a shard holds some of them)
    if ((rc = check_solar_gains(b->n_surf, s, c.sky, c.gains, heat::last_error()))) return rc;
    if ((rc = check_shades(b->n_surf, s, c.sky, c.gains, c.shades, heat::last_error()))) return rc;
    if ((rc = check_sky_aniso(b->n_surf, s, c.sky, c.gains, c.shades, c.aniso, heat::last_error()))) return rc;
    if ((rc = check_blinds(b->n_zones, s, c.shades, c.blinds, heat::last_error()))) return rc;
    if ((rc = check_air_paths(b->n_zones, s->n_channels, c.air, heat::last_error()))) return rc;
    if ((rc = check_room_radiation(b->n_surf, s, c.sky, c.radiation, heat::last_error()))) return rc;
    if ((rc = check_ambient(b->n_surf, side_kind, b->n_zones, s, c.ambient, heat::last_error()))) return rc;
    if ((rc = check_comfort(b->n_surf, b->n_zones, s, c.comfort, heat::last_error()))) return rc;
    if ((rc = check_air_handlers(b->n_zones, s->n_channels, c.handlers, heat::last_error()))) return rc;
    const int64_t S = b->n_surf, Z = b->n_zones, P = s->n_probes, n_sites = b->n_sites;
    const int n_steps = s->n_steps, n_sub = s->n_sub, NC = s->n_channels;
    if (!c.trace && !c.no_trace_ok && (int64_t)n_steps * P > 0) return fail(HEAT_E_INVALID_ARG, "trace is NULL");
    if (n_steps == 0) return HEAT_OK;
    if ((rc = select_device(b))) return rc;
    if ((rc = grow_weather(b, n_sub))) return rc;  // (once, before the first step: the pointers a captured graph holds stay valid)
    b->n_weather = n_sub;
    // ---- the terms: host tables first; on the device for the duration of the call, freed on every return path behind the drain ----
    // The schedules: a step's weather records exactly as heat_batch_set_weather lays them out in d_weather (site-major,
    // weather_cap apart); the zone terms as rows of [a0[Z] | b0[Z]] as k_begin_march reads them (no rows given: one of zeros)
    const size_t cap = b->weather_cap, n_rec = n_sub > 0 ? (size_t)(n_sites - 1) * cap + (size_t)n_sub : 0;
    const int zrows = std::max(s->n_zone_term_steps, 1);
    std::vector<StepWeather> h_w((size_t)n_steps * n_rec, StepWeather{0.0, 0.0, 0.0, 0.0});
    std::vector<double> h_zab((size_t)zrows * 2 * Z, 0.0);
    for (int k = 0; k < n_steps; k++)
        for (int64_t st = 0; st < n_sites; st++)
            for (int i = 0; i < n_sub; i++)
                h_w[(size_t)k * n_rec + st * cap + i] = to_step_weather(s->weather[((size_t)k * n_sub + i) * n_sites + st]);
    for (int64_t i = 0; i < (int64_t)zrows * Z && s->n_zone_term_steps > 0; i++) {
        if (s->zone_a0) h_zab[(size_t)(i / Z * 2 * Z + i % Z)] = s->zone_a0[i];
        if (s->zone_b0) h_zab[(size_t)((i / Z * 2 + 1) * Z + i % Z)] = s->zone_b0[i];
    }
    DevBuf<StepWeather> d_w;
    DevBuf<double> d_zab, d_channel;
    InputsTerm in; ProbesTerm probes; LoadsTerm loads; ReportTerm report; IdealTerm ideal;
    ShadesTerm shades; BlindsTerm blinds; GainsTerm gains; RadiationTerm radiation; AmbientTerm ambient; AirTerm air; AnisoTerm aniso;
    ComfortTerm comfort;
    HandlersTerm handlers;
    in.prepare(b, s);
    sky.prepare(b, c.sky, in);
    gains.prepare(b, c.gains, in);
    shades.prepare(b, c.shades, sky.bits);
    blinds.prepare(c.blinds, shades.NS);
    aniso.prepare(b, c.aniso, sky.bits);
    radiation.prepare(b, c.radiation, in);
    ambient.prepare(b, side_kind, c.ambient);
    if ((rc = probes.prepare(b, s))) return rc;
    report.prepare(b, c.r, P, group_entry);
    loads.prepare(b, c.l);
    ideal.prepare(c.il, load_of_zone);
    air.prepare(b, c.air);
    comfort.prepare(b, c.comfort);
    handlers.prepare(b, c.handlers);
    const int64_t NT = loads.NT, NI = ideal.NI, NA = gains.NA, NS = shades.NS, NR = radiation.NR, NB = ambient.NB, NP = air.NP, G = report.G;
    const int64_t NL = blinds.NL, NF = comfort.NF, NU = handlers.NU, NBR = handlers.NBR;
    SeriesDrain drain{b};
    if ((rc = series_upload(d_w, h_w, "weather schedule"))) return rc;
    if ((rc = series_upload(d_zab, h_zab, "zone terms"))) return rc;
    if ((rc = series_upload(d_channel, s->channel, (size_t)n_steps * NC, "channel table"))) return rc;
    if ((rc = in.upload())) return rc;
    if ((rc = probes.upload(c.trace, n_steps))) return rc;
    if ((rc = loads.upload(c.applied, n_steps))) return rc;
    if ((rc = report.upload(n_steps, probes, loads))) return rc;
    if ((rc = ideal.upload(b, c.ideal_q, n_steps))) return rc;
    if ((rc = sky.upload(b, s, c.sky, sky.bits || NA > 0 || NS > 0, in))) return rc;
    if ((rc = shades.upload(c.shades, NA, c.sunlit, n_steps, NL > 0, sky))) return rc;
    if ((rc = blinds.upload(shades, c.position, c.blind_incident, n_steps))) return rc;
    if ((rc = gains.upload(b, c.transmitted, n_steps, shades, in))) return rc;
    if ((rc = aniso.upload(b, s, NA, NS))) return rc;
    if ((rc = radiation.upload(c.irradiance, n_steps, in))) return rc;
    if ((rc = ambient.upload(c.ambient, c.ambient_t, n_steps))) return rc;
    if ((rc = air.upload(b, c.path_q, n_steps))) return rc;
    if ((rc = comfort.upload(b, c.operative, c.mrt, n_steps))) return rc;
    if ((rc = handlers.upload(c.supply_t, c.recovered, c.coil_q, c.branch_q, n_steps))) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (the uploads went through the null stream; the batch's streams do not wait for it)
    HIP_TRY(report.start(b->stream));
    HIP_TRY(ideal.start(b->stream));
    HIP_TRY(comfort.start(b->stream));
    // what the thermostats, the air paths' e and the blinds sense: the zone temperatures, or with a control sensor the step's Tc
    const double *control_T = comfort.control_T.p ? comfort.control_T.p : b->d_zone_T.p;
    double *mirror = b->direct_runs.empty() ? nullptr : b->d_state.p;
    // ---- the steps, enqueued without waiting: head -> comfort -> control temperatures -> zone loads -> thermostat statistics -> air paths -> air handlers -> ambient drive ->
    // driven inputs -> shades -> blinds -> sky -> solar gains -> room radiation -> the body of a march call of n_sub -> probes -> report ----
    for (int k = 0; k < n_steps; k++) {
        const double *channel = row(d_channel, k, NC);
        const SkyRecord *record = row(sky.record, k, n_sites);
        const SkyCoef *coef = row(aniso.coef, k, n_sites);  // (nullptr without aniso: the isotropic kernels)
        // (the powers of the step: a row of the applied buffer, or one row of scratch where the caller takes none)
        double *applied = loads.applied.p ? row(loads.applied, k, NT) : report.applied_row.p;
        launch_begin_march(row(d_w, k, (int64_t)n_rec), b->d_weather.p, n_sub, (int)n_rec, row(d_zab, std::min(k, zrows - 1), 2 * Z), b->d_zone_a0.p, b->d_zone_b0.p, (int)Z, b->d_step.p, b->stream);
        if (NF > 0) {
            launch_series_comfort(comfort.view, channel, b->d_T.p, b->d_zone_T.p, row(comfort.operative, k, NF), row(comfort.mrt, k, NF),
                                  c.comfort->step_base + k, b->stream);
            if (comfort.control_T.p) launch_series_control_T((int)Z, comfort.ctl.p, comfort.top.p, b->d_zone_T.p, comfort.control_T.p, b->stream);
        }
        if (loads.on)
            launch_series_zone_loads((int)Z, loads.view, channel, control_T, b->d_zone_a0.p, b->d_zone_b0.p, applied, b->d_flags.p, b->stream);
        if (report.th_stats) launch_series_th_stats((int)NT, report.th, loads.mode.p, applied, b->stream);
        if (NP > 0)
            launch_series_air_paths((int)Z, air.view, channel, b->d_zone_T.p, control_T, b->d_zone_a0.p, b->d_zone_b0.p, row(air.path_q, k, NP), b->d_flags.p,
                                    b->stream);
        if (NU > 0) {
            double *branch_row = row(handlers.branch_q, k, NBR);
            launch_series_handler_units(handlers.view, channel, b->d_zone_T.p, row(handlers.supply_t, k, NU), row(handlers.recovered, k, NU),
                                        row(handlers.coil_q, k, NU), branch_row, b->stream);
            if (handlers.supplies())
                launch_series_handler_supply((int)Z, handlers.view, b->d_zone_T.p, b->d_zone_a0.p, b->d_zone_b0.p, branch_row, b->d_flags.p, b->stream);
        }
        if (NB > 0) launch_series_ambient(ambient.view, channel, b->d_zone_T.p, b->d_side_const.p, row(ambient.t, k, NB), b->stream);
        if (in.driven)
            launch_series_inputs((int)S, channel, in.view, b->d_T.p, b->d_side_alpha.p, b->d_side_dyn.p, b->sl, mirror, b->stream);
        if (NS > 0) launch_series_shading(record, shades.view, row(shades.sunlit, k, NS), b->stream);
        if (NL > 0)
            launch_series_blinds(record, blinds.view, channel, control_T, row(blinds.position, k, NL), row(blinds.incident, k, NL), coef,
                                 aniso.shade.p, b->stream);
        if (sky.bits) launch_series_sky((int)S, record, sky.view, b->d_side_alpha.p, b->d_side_dyn.p, b->sl, mirror, coef, aniso.side.p, b->stream);
        if (NA > 0) {
            launch_series_apertures(record, gains.apertures, row(gains.transmitted, k, NA), coef, aniso.aperture.p, b->stream);
            launch_series_solar_gains((int)S, gains.view, b->d_side_alpha.p, b->d_side_dyn.p, b->sl, mirror, b->stream);
        }
        if (NR > 0) {
            launch_series_emission(radiation.view, b->d_T.p, b->stream);
            launch_series_room_radiation((int)S, radiation.view, channel, b->d_side_dyn.p, b->sl, mirror, row(radiation.irradiance, k, NR),
                                         b->stream);
        }
        if (NI > 0) {
            launch_series_ideal_begin(ideal.view, channel, b->stream);
            rc = march_body_ideal(b, n_sub, ideal.view);
        } else {
            rc = march_body(b, n_sub);
        }
        if (rc) return rc;
        if (NI > 0) launch_series_ideal_end(ideal.view, row(ideal.q, k, NI), c.il->step_base + k, b->stream);
        // (without a trace: no probe is copied, lane 0 still watches the failure flags)
        launch_series_probe(probes.trace.p ? P : 0, probes.buf.p, probes.idx.p, b->d_T.p, b->d_side_out.p, b->d_zone_T.p,
                            row(probes.trace, k, P), b->d_flags.p, probes.failed.p, k, b->stream);
        if (report.q_stats) {  // (a report that asks nothing of its quantities launches nothing here)
            launch_series_groups(report.groups, b->d_T.p, b->d_side_out.p, b->d_zone_T.p, b->stream);
            launch_series_stats(report.stats, b->d_T.p, b->d_side_out.p, b->d_zone_T.p, row(report.group_trace, k, G), c.r->step_base + k,
                                b->stream);
        }
    }
    HIP_TRY(hipGetLastError());
    // ---- one wait: the rows, the accumulators and the record of the first failure travel at the end of the stream's work ----
    int first_failed[5] = {-1, 0, 0, 0, 0};
    HIP_TRY(probes.fetch(c.trace, b->stream));
    HIP_TRY(loads.fetch(c.l, c.applied, b->stream));
    HIP_TRY(report.fetch(b->stream));
    HIP_TRY(ideal.fetch(c.ideal_q, b->stream));
    HIP_TRY(gains.fetch(c.transmitted, b->stream));
    HIP_TRY(air.fetch(c.path_q, b->stream));
    HIP_TRY(shades.fetch(c.sunlit, b->stream));
    HIP_TRY(blinds.fetch(c.position, c.blind_incident, b->stream));
    HIP_TRY(radiation.fetch(c.irradiance, b->stream));
    HIP_TRY(ambient.fetch(c.ambient_t, b->stream));
    HIP_TRY(comfort.fetch(c.operative, c.mrt, b->stream));
    HIP_TRY(handlers.fetch(c.supply_t, c.recovered, c.coil_q, c.branch_q, b->stream));
    HIP_TRY(hipMemcpyAsync(first_failed, probes.failed.p, sizeof first_failed, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (first_failed[0] < 0) return HEAT_OK;  // (the flags were clear after the last step: nothing to report)
    // A numerical failure: reported as heat_batch_synchronize reports it, from the flags as they were after the step that
    // set them (the steps enqueued behind it marched on and may have added to them).
    if (c.failed_step) *c.failed_step = first_failed[0];
    HIP_TRY(hipMemcpy(b->d_flags.p, first_failed + 1, 4 * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return heat_batch_synchronize(b);
}

int heat_batch_march_series(heat_batch *b, const heat_series *s, double *trace, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.trace = trace, c.failed_step = failed_step;
    return march_series_impl(b, c);
}

int heat_batch_march_series_loads(heat_batch *b, const heat_series *s, const heat_zone_loads *l, double *trace, double *applied,
                                  int32_t *failed_step) {
    SeriesCall c; c.s = s, c.l = l, c.trace = trace, c.applied = applied, c.failed_step = failed_step;
    return march_series_impl(b, c);
}

int heat_batch_march_series_report(heat_batch *b, const heat_series *s, const heat_zone_loads *l, heat_series_report *r, double *trace,
                                   double *applied, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.l = l, c.r = r, c.trace = trace, c.applied = applied, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_ideal(heat_batch *b, const heat_series *s, const heat_zone_loads *l, heat_ideal_loads *il,
                                  heat_series_report *r, double *trace, double *applied, double *ideal_q, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.l = l, c.il = il, c.r = r, c.trace = trace, c.applied = applied, c.ideal_q = ideal_q;
    c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_sky(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_zone_loads *l, heat_ideal_loads *il,
                                heat_series_report *r, double *trace, double *applied, double *ideal_q, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.l = l, c.il = il, c.r = r, c.trace = trace, c.applied = applied, c.ideal_q = ideal_q;
    c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_gains(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_solar_gains *gains,
                                  const heat_zone_loads *l, heat_ideal_loads *il, heat_series_report *r, double *trace, double *applied,
                                  double *ideal_q, double *transmitted, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.gains = gains, c.l = l, c.il = il, c.r = r, c.trace = trace, c.applied = applied;
    c.ideal_q = ideal_q, c.transmitted = transmitted, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_air(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_solar_gains *gains,
                                const heat_zone_loads *l, heat_air_paths *air, heat_ideal_loads *il, heat_series_report *r, double *trace,
                                double *applied, double *ideal_q, double *transmitted, double *path_q, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.gains = gains, c.l = l, c.air = air, c.il = il, c.r = r, c.trace = trace, c.applied = applied;
    c.ideal_q = ideal_q, c.transmitted = transmitted, c.path_q = path_q, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_shaded(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_shades *shades,
                                   const heat_solar_gains *gains, const heat_zone_loads *l, heat_air_paths *air, heat_ideal_loads *il,
                                   heat_series_report *r, double *trace, double *applied, double *ideal_q, double *transmitted,
                                   double *path_q, double *sunlit, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.shades = shades, c.gains = gains, c.l = l, c.air = air, c.il = il, c.r = r, c.trace = trace;
    c.applied = applied, c.ideal_q = ideal_q, c.transmitted = transmitted, c.path_q = path_q, c.sunlit = sunlit;
    c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_radiation(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_shades *shades,
                                      const heat_solar_gains *gains, const heat_zone_loads *l, heat_air_paths *air, heat_ideal_loads *il,
                                      heat_series_report *r, double *trace, double *applied, double *ideal_q, double *transmitted,
                                      double *path_q, double *sunlit, heat_room_radiation *radiation, double *irradiance,
                                      int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.shades = shades, c.gains = gains, c.l = l, c.air = air, c.il = il, c.r = r, c.trace = trace;
    c.applied = applied, c.ideal_q = ideal_q, c.transmitted = transmitted, c.path_q = path_q, c.sunlit = sunlit, c.radiation = radiation;
    c.irradiance = irradiance, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_ambient(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_shades *shades,
                                    const heat_solar_gains *gains, const heat_zone_loads *l, heat_air_paths *air, heat_ideal_loads *il,
                                    heat_series_report *r, double *trace, double *applied, double *ideal_q, double *transmitted,
                                    double *path_q, double *sunlit, heat_room_radiation *radiation, double *irradiance,
                                    heat_ambient_drive *ambient, double *ambient_t, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.shades = shades, c.gains = gains, c.l = l, c.air = air, c.il = il, c.r = r, c.trace = trace;
    c.applied = applied, c.ideal_q = ideal_q, c.transmitted = transmitted, c.path_q = path_q, c.sunlit = sunlit, c.radiation = radiation;
    c.irradiance = irradiance, c.ambient = ambient, c.ambient_t = ambient_t, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_blinds(heat_batch *b, const heat_series *s, const heat_sky *sky, const heat_shades *shades,
                                   const heat_solar_gains *gains, const heat_zone_loads *l, heat_air_paths *air, heat_ideal_loads *il,
                                   heat_series_report *r, double *trace, double *applied, double *ideal_q, double *transmitted,
                                   double *path_q, double *sunlit, heat_room_radiation *radiation, double *irradiance,
                                   heat_ambient_drive *ambient, double *ambient_t, heat_blinds *blinds, double *position,
                                   double *blind_incident, int32_t *failed_step) {
    SeriesCall c; c.s = s, c.sky = sky, c.shades = shades, c.gains = gains, c.l = l, c.air = air, c.il = il, c.r = r, c.trace = trace;
    c.applied = applied, c.ideal_q = ideal_q, c.transmitted = transmitted, c.path_q = path_q, c.sunlit = sunlit, c.radiation = radiation;
    c.irradiance = irradiance, c.ambient = ambient, c.ambient_t = ambient_t, c.blinds = blinds, c.position = position;
    c.blind_incident = blind_incident, c.failed_step = failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

// heat_batch_march_series_call, heat_batch_march_series_comfort and heat_batch_march_series_handlers: the struct's fields by
// name, then the comfort term, then the air handlers (`more`: what the last of them adds, or nullptr).
static int march_series_call(heat_batch *b, const heat_series_call *call, heat_comfort *comfort, double *operative, double *mrt,
                             const SeriesCall *more = nullptr) {
    if (const int rc = check_series_call(call, heat::last_error())) return rc;  // (a struct of another size is not read further)
    SeriesCall c;
    if (more) c = *more;
    c.comfort = comfort, c.operative = operative, c.mrt = mrt; c.s = call->s, c.sky = call->sky, c.aniso = call->aniso, c.shades = call->shades, c.gains = call->gains, c.l = call->l;
    c.air = call->air, c.il = call->il, c.r = call->r, c.radiation = call->radiation, c.ambient = call->ambient, c.blinds = call->blinds;
    c.trace = call->trace, c.applied = call->applied, c.ideal_q = call->ideal_q, c.transmitted = call->transmitted, c.path_q = call->path_q;
    c.sunlit = call->sunlit, c.irradiance = call->irradiance, c.ambient_t = call->ambient_t, c.position = call->position;
    c.blind_incident = call->blind_incident, c.failed_step = call->failed_step, c.no_trace_ok = true;
    return march_series_impl(b, c);
}

int heat_batch_march_series_call(heat_batch *b, const heat_series_call *call) { return march_series_call(b, call, nullptr, nullptr, nullptr); }

int heat_batch_march_series_comfort(heat_batch *b, const heat_series_call *call, heat_comfort *c, double *operative, double *mrt) {
    return march_series_call(b, call, c, operative, mrt);
}

int heat_batch_march_series_handlers(heat_batch *b, const heat_series_call *call, heat_comfort *c, double *operative, double *mrt,
                                     heat_air_handlers *h, double *supply_t, double *recovered, double *coil_q, double *branch_q) {
    SeriesCall more; more.handlers = h, more.supply_t = supply_t, more.recovered = recovered, more.coil_q = coil_q, more.branch_q = branch_q;
    return march_series_call(b, call, c, operative, mrt, &more);
}

// The ambient temperature of the listed sides from the next march on: k_series_ambient with the temperatures as its row
// (lane i takes row[i]; no gain, offset or mix), on the batch's stream behind earlier work. The tables and the values are
// per-call device buffers: the call waits for its own kernel before it frees them, so the caller's arrays are free too.
int heat_batch_set_ambient(heat_batch *b, int64_t n, const int64_t *surface, const uint8_t *side, const double *temperature) {
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    // ---- everything that needs no device ----
    // (a shard holds some of the caller's surfaces under numbers of its own: out of scope, as for the series)
    if (b->n_ranks > 1) return fail(HEAT_E_INVALID_ARG, "a sharded batch (n_ranks = %d) cannot set ambient temperatures", b->n_ranks);
    if (n > 0 && !temperature) return fail(HEAT_E_INVALID_ARG, "entry 0: temperature is NULL (count %lld)", (long long)n);
    const int32_t *const side_kind[2] = {b->h_kind[0].data(), b->h_kind[1].data()};
    int rc = check_ambient_sides(b->n_surf, side_kind, n, surface, side, "entry", heat::last_error());
    if (rc) return rc;
    if (n == 0) return HEAT_OK;
    AmbientTerm abd;
    build_ambient_tables(b->n_surf, b->h_dev_of.data(), side_kind, n, surface, side, abd.abt);
    rc = select_device(b);
    if (rc) return rc;
    SeriesDrain drain{b};
    if ((rc = abd.upload_tables())) return rc;
    if ((rc = series_upload(abd.t, temperature, (size_t)n, "ambient temperatures"))) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (the uploads went through the null stream; the batch's streams do not wait for it)
    abd.view.n_sides = (int)n;
    launch_series_ambient(abd.view, abd.t.p, b->d_zone_T.p, b->d_side_const.p, nullptr, b->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
    return HEAT_OK;
}

int64_t heat_batch_nomass_iterations(heat_batch *b) {
    if (!b) return 0;
    if (hipSetDevice(b->device) != hipSuccess) return -1;
    if (hipStreamSynchronize(b->stream) != hipSuccess) return -1;
    std::vector<unsigned long long> h(b->d_nomass_iters.n);
    if (hipMemcpy(h.data(), b->d_nomass_iters.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) !=
        hipSuccess)
        return -1;
    unsigned long long v = 0;
    for (unsigned long long x : h) v += x;
    if (b->d_ucount.n) {
        h.resize(b->d_ucount.n);
        if (hipMemcpy(h.data(), b->d_ucount.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
            return -1;
        for (unsigned long long x : h) v += x;
    }
    return (int64_t)v;
}

int heat_batch_set_timing(heat_batch *b, int32_t enabled) {
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    b->timing = enabled != 0;
    b->timing_every = enabled > 1 ? enabled : 1;
    b->timing_calls = 0;
    b->ev_used = 0;
    b->ev_triples.clear();
    b->ev_fused_pairs.clear();
    return HEAT_OK;
}

int heat_batch_get_timing(heat_batch *b, double *surf_us, double *substep_us, int64_t *n_samples) {
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    int rc = select_device(b);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    double s_surf = 0, s_all = 0, s_fused = 0;
    int64_t n_fused_steps = 0;
    const size_t n = b->ev_triples.size();
    for (const auto &t : b->ev_triples) {
        float ms1 = 0, ms2 = 0;
        HIP_TRY(hipEventElapsedTime(&ms1, t.e0, t.e1));
        HIP_TRY(hipEventElapsedTime(&ms2, t.e0, t.e2));
        s_surf += ms1;
        s_all += ms2;
    }
    for (const auto &p : b->ev_fused_pairs) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p.e0, p.e1));
        s_fused += ms;
        n_fused_steps += p.n_sub;
    }
    const double stream_surf = n ? s_surf * 1000.0 / (double)n : 0.0;
    const double stream_all = n ? s_all * 1000.0 / (double)n : 0.0;
    const double fused_us = n_fused_steps ? s_fused * 1000.0 / (double)n_fused_steps : 0.0;
    // With a cluster-resident march the surface kernel of a sub-timestep is 1/n_sub of the fused launch (the
    // streamed remainder, if any, runs beside it on another stream).
    if (surf_us) *surf_us = n_fused_steps ? fused_us : stream_surf;
    // (a large batch runs its streamed remainder after the fused launch, a small one beside it)
    if (substep_us) *substep_us = n_fused_steps ? (b->n_surf > 8192 ? fused_us + stream_all : std::max(fused_us, stream_all)) : stream_all;
    if (n_samples) *n_samples = n_fused_steps ? n_fused_steps : (int64_t)n;
    b->ev_used = 0;
    b->ev_triples.clear();
    b->ev_fused_pairs.clear();
    return HEAT_OK;
}

int heat_batch_set_fusion(heat_batch *b, int32_t enabled) {
    if (!b) return fail(HEAT_E_INVALID_ARG, "NULL batch");
    b->fusion_on = enabled != 0;
    return HEAT_OK;
}

int64_t heat_batch_n_fused_surfaces(const heat_batch *b) { return b ? b->n_fused_surfaces : 0; }
int64_t heat_batch_n_fused_launches(const heat_batch *b) { return b ? b->n_fused_launches : 0; }

}  // extern "C"
