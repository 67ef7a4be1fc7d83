// plan.cpp — host-only planner of a heat batch (plan.hpp). Compiled into libheat_amd.so by hipcc and, on its own, by
// g++ for the sanitizer tests: no HIP here.
#include "plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>

namespace heat {

const int kFastM[kNumFast] = {4, 4, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8, 16, 16, 16, 16, 16, 16};
const int kFastNM[kNumFast] = {0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1};
const int kFastPAL[kNumFast] = {0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1};
const int kFastCAV[kNumFast] = {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};

namespace {

int failp(std::string &err, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

struct Placed {
    int64_t s;   // original surface index
    int n;       // node count
    int cls;     // 0..kNumFast-1 fast classes, kGeneral = catch-all
    int k;       // lanes per surface (fast)
    int blk;     // cluster-resident march: workgroup number, -1 = streamed
    int site;    // weather site (0 in a single-site batch)
};

// Tiles of a cluster-resident workgroup: its surfaces are packed into wavefronts whatever their lane counts (a
// mixed tile carries a lane table, layout.hpp), in ascending order of k — what the tiling below does.
int tiles_needed_packed(const int (&cnt)[kWave + 1]) {
    int tiles = 0, lanes = 0;
    for (int k = 1; k <= kWave; k++)
        for (int q = 0; q < cnt[k]; q++) {
            if (lanes + k > kWave) { tiles++; lanes = 0; }
            lanes += k;
        }
    return tiles + (lanes > 0);
}

// What kind of kernel a surface needs (before the blocking factor M is chosen).
struct Category {
    int kind;  // kSmall, kSmallCav, kGeneral, or 0 = fast path
    int nm;    // fast: has no-mass chunks (one or two nodes each, between massive nodes and / or a face)
    int ncav;  // fast: gas cavities between massive nodes
    int pal;   // fast: the per-node constants fit a palette
    int m_ok;  // fast: blocking factors whose lanes hold every chunk whole (bit 0: 4, bit 1: 8, bit 2: 16 nodes per lane)
    int chunky = 0;  // fast: has chunks other than one-node facings (inside the wall, or of two nodes)
    int wide = 0;    // fast, palette form: needs the wide palette (more than 8 V or 4 U entries, with the 0.0 of entry 0)
    int tiny = 0;    // fast, palette form: fits the tiny palette (4 V and 4 U entries at most)
};
inline int m_bit(int M) { return M == 4 ? 1 : (M == 8 ? 2 : 4); }

// Decides whether a surface can take the register-resident fast path:
// solid conductances only, solar absorbed at the two faces only, every interior node massive; the
// face nodes may be no-mass facings (each then is an isolated one-node no-mass chunk).
Category categorize(const heat_batch_desc *d, int64_t s, int n, const heat_batch_options &opt) {
    Category r{kGeneral, 0, 0, 0, 7};
    if (opt.force_general) return r;
    const int64_t o = d->node_offset[s];
    if (n <= 4) {
        bool all_nomass = true;
        for (int i = 0; i < n; i++) all_nomass = all_nomass && (d->mass[o + i] < kMassThreshold);
        bool has_cav = false;
        for (int i = 0; i < n; i++)
            has_cav = has_cav || (d->seg_cavity && d->n_cavities > 0 && d->seg_cavity[o + i] >= 0);
        if (all_nomass) {
            r.kind = has_cav ? kSmallCav : kSmall;
            return r;
        }
    }
    if (n < 2) return r;
    int nm = 0, ncav = 0, m_ok = 7;
    bool facings_only = true;
    auto is_cav = [&](int i) { return d->seg_cavity && d->n_cavities > 0 && d->seg_cavity[o + i] >= 0; };
    for (int i = 0; i < n; i++) {
        if (is_cav(i)) {
            // a cavity on the fast path sits between two massive nodes (its conductance is then needed
            // once per sub-timestep, not once per pass of a no-mass loop)
            if (i + 1 >= n || d->mass[o + i] < kMassThreshold || d->mass[o + i + 1] < kMassThreshold) return r;
            if (++ncav > 2) return r;
        }
        if (i > 0 && d->front_alpha[o + i] != 0.0) return r;           // solar absorbed inside
        if (i < n - 1 && d->back_alpha[o + i] != 0.0) return r;
    }
    // No-mass chunks (get_chunks, discretization.rs:144-160): one or two nodes each — a thin facing, two light
    // layers at a face, two light layers inside a cavity wall; longer runs go to the catch-all kernel. A two-node
    // chunk has to sit in one lane, and a lane solves two chunks at most.
    for (int i = 0; i < n;) {
        if (d->mass[o + i] >= kMassThreshold) { i++; continue; }
        int e = i;
        while (e < n && d->mass[o + e] < kMassThreshold) e++;
        if (e - i > 2) return r;
        nm = 1;
        if (!(e - i == 1 && (i == 0 || i == n - 1))) facings_only = false;
        for (int M : {4, 8, 16})
            if (e - i == 2 && i / M != (i + 1) / M) m_ok &= ~m_bit(M);
        i = e;
    }
    for (int M : {4, 8, 16}) {
        int in_lane = 0, lane = -1;
        for (int i = 0; i < n; i++) {
            const bool start = d->mass[o + i] < kMassThreshold && (i == 0 || d->mass[o + i - 1] >= kMassThreshold);
            if (i / M != lane) { lane = i / M; in_lane = 0; }
            if (start && ++in_lane > 2) m_ok &= ~m_bit(M);
        }
    }
    if (m_ok == 0) return r;
    // Palette form when the wall has few distinct constants (entry 0 of each palette is 0.0).
    int pal = opt.no_palette ? 0 : 1;
    int nu = 1, nv = 1;
    if (pal) {
        double vv[kPalV], uu[kPalU];
        vv[0] = 0.0;
        uu[0] = 0.0;
        for (int i = 0; i < n && pal; i++) {
            const double mass = d->mass[o + i];
            const double v = (mass >= kMassThreshold) ? d->dt / mass : 0.0;
            const double u = is_cav(i) ? 0.0 : d->uvalue[o + i];
            int f = -1;
            for (int q = 0; q < nv; q++) if (vv[q] == v) f = q;
            if (f < 0) { if (nv == kPalVMark1) pal = 0; else vv[nv++] = v; }  // (indices 14, 15 are chunk marks)
            f = -1;
            for (int q = 0; q < nu; q++) if (uu[q] == u) f = q;
            if (f < 0) { if (nu == kPalU) pal = 0; else uu[nu++] = u; }
        }
    }
    if (ncav > 0 && !pal) return r;  // the cavity variant exists in palette form only
    if (nm && !facings_only && !pal) return r;  // chunks other than one-node facings are marked in the class bytes
    r.kind = 0;
    r.nm = nm;
    r.ncav = ncav;
    r.pal = pal;
    r.m_ok = m_ok;
    r.chunky = (nm && !facings_only) ? 1 : 0;
    r.wide = (pal && (nv > kPalVNarrow || nu > kPalUNarrow)) ? 1 : 0;
    r.tiny = (pal && nv <= kPalVTiny && nu <= kPalUTiny) ? 1 : 0;
    return r;
}

// Nodes are padded to a multiple of M inside the last lane. Measured cost per padded node
// (1 M x 32 and 1 M x 20 nodes, profiles/README.md): M = 16 : 8 : 4 = 1.00 : 1.03 : 1.30 — larger blocks
// amortise the per-surface boundary work over more nodes.
double padded_cost(int n, int M) {
    const double w = (M == 4) ? 1.30 : (M == 8 ? 1.03 : 1.00);
    return (double)((n + M - 1) / M * M) * w;
}

// nm: the wall has a no-mass facing. Its 16-node variant (k_surfaces_fast<16, 1, 1, 0>) needs 266 registers — one
// wavefront per SIMD, 3.1 TB/s against 6.2 for the all-massive walls (profiles/README.md, round 2) — so walls with
// facings take 8 nodes per lane at most.
int choose_M(int n, int nm, int m_ok, const heat_batch_options &opt) {
    if (opt.nodes_per_lane != 0) return (m_ok & m_bit(opt.nodes_per_lane)) ? opt.nodes_per_lane : 0;
    int M = 0;
    for (int m : {4, 8, 16}) {
        if ((nm && m == 16 && (m_ok & 3)) || !(m_ok & m_bit(m))) continue;
        if (M == 0 || padded_cost(n, m) < padded_cost(n, M)) M = m;
    }
    return M;  // 0: no blocking factor holds the wall's chunks -> catch-all
}

int fast_class(int M, const Category &c) { return (M == 4 ? 0 : (M == 8 ? 6 : 12)) + c.nm * 3 + (c.ncav > 0 ? 2 : c.pal); }


}  // namespace

int check_desc(const heat_batch_desc *d, std::string &err) {
    if (!d) return failp(err, HEAT_E_INVALID_ARG, "descriptor is NULL");
    if (d->abi_version != HEAT_AMD_ABI_VERSION)
        return failp(err, HEAT_E_INVALID_ARG, "abi_version %d, library is %d", d->abi_version, HEAT_AMD_ABI_VERSION);
    if (d->n_surfaces < 0 || d->n_zones < 0 || d->n_cavities < 0 || d->n_state < 0)
        return failp(err, HEAT_E_INVALID_ARG, "negative count in descriptor");
    if (!(d->dt > 0.0)) return failp(err, HEAT_E_INVALID_ARG, "dt must be positive");
    const void *need[] = {d->node_offset, d->mass, d->uvalue, d->front_alpha, d->back_alpha, d->front_kind,
                          d->back_kind, d->front_zone, d->back_zone, d->front_ambient, d->back_ambient,
                          d->front_emissivity, d->back_emissivity, d->area, d->perimeter, d->cos_tilt,
                          d->normal_x, d->normal_y, d->wind_modifier, d->first_node_slot, d->hs_front_slot,
                          d->hs_back_slot, d->flow_front_slot, d->flow_back_slot, d->solar_front_slot,
                          d->solar_back_slot, d->ir_front_slot, d->ir_back_slot};
    if (d->n_surfaces > 0)
        for (const void *p : need)
            if (!p) return failp(err, HEAT_E_INVALID_ARG, "a required per-surface array is NULL");
    if (d->n_zones > 0 && (!d->zone_volume || !d->zone_slot))
        return failp(err, HEAT_E_INVALID_ARG, "zone arrays are NULL");
    if (d->n_cavities > 0 && (!d->cavities || !d->seg_cavity))
        return failp(err, HEAT_E_INVALID_ARG, "cavity arrays are NULL");
    if ((d->front_hs_fix == nullptr) != (d->back_hs_fix == nullptr))
        return failp(err, HEAT_E_INVALID_ARG, "front_hs_fix and back_hs_fix must both be given or both be NULL");
    const int64_t ns = d->n_state;
    auto slot_ok = [&](int64_t v) { return v >= 0 && v < ns; };
    for (int64_t z = 0; z < d->n_zones; z++)
        if (!slot_ok(d->zone_slot[z])) return failp(err, HEAT_E_SIZE, "zone %lld: slot out of range", (long long)z);
    if (d->n_surfaces > 0 && d->node_offset[0] != 0) return failp(err, HEAT_E_INVALID_ARG, "node_offset[0] != 0");
    for (int64_t s = 0; s < d->n_surfaces; s++) {
        const int64_t n = d->node_offset[s + 1] - d->node_offset[s];
        if (n < 1) return failp(err, HEAT_E_INVALID_ARG, "surface %lld has %lld nodes", (long long)s, (long long)n);
        if (n > kMaxNodesGeneral)
            return failp(err, HEAT_E_TOO_MANY_NODES, "surface %lld has %lld nodes (max %d)", (long long)s, (long long)n,
                        kMaxNodesGeneral);
        const int fk = d->front_kind[s], bk = d->back_kind[s];
        if (fk == HEAT_BOUNDARY_GROUND || bk == HEAT_BOUNDARY_GROUND)
            return failp(err, HEAT_E_GROUND_BOUNDARY, "surface %lld: Ground boundary is not supported (reference panics)", (long long)s);
        if (fk < 0 || fk > 2 || bk < 0 || bk > 2)
            return failp(err, HEAT_E_INVALID_ARG, "surface %lld: unknown boundary kind", (long long)s);
        if (fk == HEAT_BOUNDARY_SPACE && (d->front_zone[s] < 0 || d->front_zone[s] >= d->n_zones))
            return failp(err, HEAT_E_SIZE, "surface %lld: front zone out of range", (long long)s);
        if (bk == HEAT_BOUNDARY_SPACE && (d->back_zone[s] < 0 || d->back_zone[s] >= d->n_zones))
            return failp(err, HEAT_E_SIZE, "surface %lld: back zone out of range", (long long)s);
        if (d->first_node_slot[s] < 0 || d->first_node_slot[s] + n > ns)
            return failp(err, HEAT_E_SIZE, "surface %lld: node slots out of range", (long long)s);
        if (!slot_ok(d->hs_front_slot[s]) || !slot_ok(d->hs_back_slot[s]) || !slot_ok(d->flow_front_slot[s]) ||
            !slot_ok(d->flow_back_slot[s]) || !slot_ok(d->solar_front_slot[s]) || !slot_ok(d->solar_back_slot[s]) ||
            !slot_ok(d->ir_front_slot[s]) || !slot_ok(d->ir_back_slot[s]))
            return failp(err, HEAT_E_SIZE, "surface %lld: scalar slot out of range", (long long)s);
        const int64_t o = d->node_offset[s];
        for (int64_t i = 0; i < n; i++) {
            const bool cav = d->seg_cavity && d->n_cavities > 0 && d->seg_cavity[o + i] >= 0;
            if (cav && d->seg_cavity[o + i] >= d->n_cavities)
                return failp(err, HEAT_E_SIZE, "surface %lld: cavity index out of range", (long long)s);
            if (!cav && std::isnan(d->uvalue[o + i]))
                return failp(err, HEAT_E_UVALUE_NONE, "surface %lld node %lld: UValue::None", (long long)s, (long long)i);
            // (a node is massive iff mass >= 1e-5, discretization.rs:149,155: a NaN is neither massive nor no-mass — the
            // reference's chunks would silently leave the node out; here it is refused. Found by tools/fuzz_desc.py as an
            // endless loop of the planner.)
            if (std::isnan(d->mass[o + i]))
                return failp(err, HEAT_E_INVALID_ARG, "surface %lld node %lld: thermal mass is NaN", (long long)s, (long long)i);
        }
    }
    return HEAT_OK;
}

int check_sites(const heat_batch_desc *d, const heat_batch_options &opt, int32_t n_sites, const int32_t *site_of_surface,
                std::string &err) {
    if (n_sites < 1 || n_sites > kMaxSites)
        return failp(err, HEAT_E_INVALID_ARG, "n_sites = %d outside [1, %d]", n_sites, kMaxSites);
    if (opt.n_ranks > 1) return failp(err, HEAT_E_INVALID_ARG, "a batch of weather sites cannot be sharded (n_ranks = %d)", opt.n_ranks);
    if (!d) return failp(err, HEAT_E_INVALID_ARG, "NULL descriptor");
    if (d->n_surfaces > 0 && !site_of_surface) return failp(err, HEAT_E_INVALID_ARG, "NULL site_of_surface");
    for (int64_t s = 0; s < d->n_surfaces; s++)
        if (site_of_surface[s] < 0 || site_of_surface[s] >= n_sites)
            return failp(err, HEAT_E_SIZE, "surface %lld: site %d outside [0, %d)", (long long)s, site_of_surface[s], n_sites);
    return HEAT_OK;
}

int make_plan(const heat_batch_desc *d, const heat_batch_options &opt, Plan &p, std::string &err, int32_t n_sites,
              const int32_t *site_of_surface) {
    int rc = check_desc(d, err);
    if (rc) return rc;
    if (n_sites != 1 || site_of_surface) {
        rc = check_sites(d, opt, n_sites, site_of_surface, err);
        if (rc) return rc;
    }
    // (one site: the plan of a batch without sites, whatever the array says — it can only say 0)
    if (n_sites == 1) site_of_surface = nullptr;
    // (heat_batch_create_ex refuses these before it comes here; heat_plan_check comes straight)
    if (opt.nodes_per_lane != 0 && opt.nodes_per_lane != 4 && opt.nodes_per_lane != 8 && opt.nodes_per_lane != 16)
        return failp(err, HEAT_E_INVALID_ARG, "nodes_per_lane must be 0, 4, 8 or 16");
    if (opt.n_ranks > 1 && (opt.rank < 0 || opt.rank >= opt.n_ranks))
        return failp(err, HEAT_E_INVALID_ARG, "rank %d outside [0, %d)", opt.rank, opt.n_ranks);
    const int64_t S = d->n_surfaces, Z = d->n_zones;
    p = Plan();
    p.n_surf = S;
    p.n_zones = Z;
    p.n_state = d->n_state;
    p.n_cav = d->n_cavities;
    p.dt = d->dt;
    p.n_nodes = S > 0 ? d->node_offset[S] : 0;
    p.algorithmic_bytes = 32 * p.n_nodes + 152 * S;  // 32 n + 152 bytes per surface per sub-timestep
    p.n_sites = n_sites;
    auto site_of = [&](int64_t s) { return site_of_surface ? site_of_surface[s] : 0; };

    // ---- classify ----
    std::vector<Placed> placed(S);
    std::vector<Category> cat(S);
    for (int64_t s = 0; s < S; s++) {
        const int n = (int)(d->node_offset[s + 1] - d->node_offset[s]);
        cat[s] = categorize(d, s, n, opt);
        int cls = cat[s].kind, k = 1;
        if (cat[s].kind == 0) {
            const int M = choose_M(n, cat[s].nm, cat[s].m_ok, opt);
            k = M ? (n + M - 1) / M : kWave + 1;
            cls = (k > kWave) ? kGeneral : fast_class(M, cat[s]);
            if (k > kWave) { cat[s].kind = kGeneral; k = 1; }
        }
        placed[s] = Placed{s, n, cls, k, -1, site_of(s)};
    }
    if (opt.nodes_per_lane == 0) {
        // A class of few surfaces is a launch of its own that cannot fill the chip (1 M ragged walls: the two 4-node
        // classes, 6 % of the surfaces, took 10 us each — as long as classes ten times their size). A blocking
        // factor that holds less than a twelfth of the fast-path nodes hands its walls to the 8-node classes.
        double nodes_by_M[3] = {0, 0, 0}, all_nodes = 0;
        for (int64_t s = 0; s < S; s++)
            if (placed[s].cls < kNumFast) {
                nodes_by_M[placed[s].cls / 6] += placed[s].n;
                all_nodes += placed[s].n;
            }
        for (int mi : {0, 2}) {
            if (nodes_by_M[mi] == 0 || nodes_by_M[mi] * 12 >= all_nodes || nodes_by_M[1] == 0) continue;
            for (int64_t s = 0; s < S; s++)
                if (placed[s].cls < kNumFast && placed[s].cls / 6 == mi && (placed[s].n + 7) / 8 <= kWave && (cat[s].m_ok & m_bit(8))) {
                    placed[s].k = (placed[s].n + 7) / 8;
                    placed[s].cls = fast_class(8, cat[s]);
                }
        }
    }

    // ---- cluster-resident march: zone-connected clusters -> workgroups (layout.hpp, FusedBlock) ----
    // A cluster is a connected component of the graph "zone - surface facing it"; its surfaces exchange heat
    // only through its own zones (model.rs:556-590), so a workgroup that holds all of them can march any number
    // of sub-timesteps without leaving the chip. A cluster is fused when every surface of it is a palette-form
    // fast-path wall without cavities and it fits kFusedMaxWaves tiles / kFusedMaxZones zones; its surfaces then
    // share one blocking factor (4 or 8: the 16-node variant does not fit the register file with the state that
    // lives across sub-timesteps). Surfaces that face no zone at all are clusters of one and are packed freely.
    // mixed: holds small-surface tiles too. super >= 0: member `member` of a team (layout.hpp, FusedSuper); zinfo: per
    // zone of the block its exchange slot | members << 16
    struct BlockPlan { int cls; bool mixed; std::vector<int32_t> zones; int super = -1; int member = 0; std::vector<uint32_t> zinfo; };
    int n_supers = 0;
    std::vector<BlockPlan> blocks;
    // no_fusion: 0 = fuse the clusters the cost model below expects to gain, 1 = never, 2 = every cluster that can be
    const bool fuse = opt.no_fusion != 1 && !opt.force_general && !opt.no_palette;
    const bool fuse_always = opt.no_fusion == 2;
    const std::vector<Placed> placed_streamed = placed;  // the plan without any cluster-resident march
    if (fuse && S > 0) {
        auto is_small = [&](int64_t s) { return cat[s].kind == kSmall || cat[s].kind == kSmallCav; };
        // (walls with no-mass chunks other than one-node facings: with 8 or 4 nodes per lane, not beside small surfaces or
        // gas cavities — the variants that carry the chunk loop, kernels.hip)
        auto fusable = [&](int64_t s) { return (cat[s].kind == 0 && cat[s].pal) || is_small(s); };
        auto zone_of_side = [&](int64_t s, int side) -> int32_t {
            const int kind = side ? d->back_kind[s] : d->front_kind[s];
            return kind == HEAT_BOUNDARY_SPACE ? (side ? d->back_zone[s] : d->front_zone[s]) : -1;
        };
        std::vector<int32_t> uf(Z);
        std::iota(uf.begin(), uf.end(), 0);
        auto find = [&](int32_t x) {
            while (uf[x] != x) { uf[x] = uf[uf[x]]; x = uf[x]; }
            return x;
        };
        for (int64_t s = 0; s < S; s++) {
            const int32_t zf = zone_of_side(s, 0), zb = zone_of_side(s, 1);
            if (zf >= 0 && zb >= 0) {
                const int32_t a = find(zf), c = find(zb);
                if (a != c) uf[std::max(a, c)] = std::min(a, c);
            }
        }
        // per cluster (root zone): its surfaces (CSR), whether all of them are fusable
        std::vector<int64_t> coff(Z + 1, 0);
        std::vector<uint8_t> cok(Z, 1);
        auto root_of = [&](int64_t s) -> int32_t {
            const int32_t zf = zone_of_side(s, 0), zb = zone_of_side(s, 1);
            return zf >= 0 ? find(zf) : (zb >= 0 ? find(zb) : -1);
        };
        std::vector<int32_t> sroot(S);
        for (int64_t s = 0; s < S; s++) {
            sroot[s] = root_of(s);
            if (sroot[s] >= 0) {
                coff[sroot[s] + 1]++;
                if (!fusable(s)) cok[sroot[s]] = 0;
            }
        }
        for (int64_t z = 0; z < Z; z++) coff[z + 1] += coff[z];
        std::vector<int64_t> csurf(Z > 0 ? coff[Z] : 0), ccur(coff.begin(), coff.end() - 1);
        for (int64_t s = 0; s < S; s++)
            if (sroot[s] >= 0) csurf[ccur[sroot[s]]++] = s;
        std::vector<std::vector<int32_t>> czones(Z);  // zones of each root
        for (int64_t z = 0; z < Z; z++) czones[find((int32_t)z)].push_back((int32_t)z);

        // open workgroup per class: surfaces per k, zones so far
        struct Open { int blk = -1; int cnt[kWave + 1] = {}; int nsmall = 0; int nz = 0; int ne = 0; };
        // [site][class][mixed]: clusters of different weather sites never share a workgroup
        std::map<std::pair<int32_t, int>, Open> open;
        auto new_block = [&](int cls, bool mixed) {
            blocks.push_back(BlockPlan{cls, mixed, {}, -1, 0, {}});
            return (int)blocks.size() - 1;
        };
        auto small_tiles = [](int n_small) { return (n_small + kWave - 1) / kWave; };
        // Cost model (measured on MI355X, profiles/README.md): what the cluster-resident march of a cluster costs by
        // blocking factor and tile count (below) against what streaming it costs — its algorithmic bytes at the
        // ~5.5 TB/s the streamed kernels sustain, plus k_zones' share. The cheapest blocking factor is taken.
        constexpr double kStreamBytesPerNs = 5500.0, kZoneNs = 1.8;
        // ns per cluster and sub-timestep. Up to four tiles (two or three workgroups per compute unit): per tile —
        // 16 nodes per lane 2.05 (1 M x 32: 82 us / 40 000 tiles), 8: 1.8 (1 M x 13: 72 us), 4: 1.15 (1 M x 8: 46 us).
        // Five to eight tiles (a workgroup has a compute unit to itself, however many of its wavefronts work): per
        // workgroup — 16: 16.5 (1 M x 48: 165 us / 10 000), 8: 14.8 (1 M x 32: 148 us), 4: 12 (1 M x 10: 118 us).
        auto cluster_ns = [](int m, int tiles) {
            if (tiles <= 4) return tiles * (m == 16 ? 2.05 : (m == 8 ? 1.8 : 1.15));
            return m == 16 ? 16.5 : (m == 8 ? 14.8 : 12.0);
        };
        auto tile_ns = [](int m) { return m == 16 ? 2.05 : (m == 8 ? 1.8 : 1.15); };  // (surfaces that face no zone)
        auto fused_cost = [&](int n, int m) {  // (explicit nodes_per_lane, lone surfaces: lanes of the surface)
            return (double)((n + m - 1) / m);
        };
        const int ms_all[3] = {4, 8, 16};
        // LDS: with wide palettes (layout.hpp) a workgroup of eight 16-node wavefronts would need 180 KB
        bool wide_batch = false;
        for (int64_t s = 0; s < S; s++) wide_batch = wide_batch || (cat[s].kind == 0 && cat[s].wide);
        auto max_tiles = [&](int m) { return (m == 16 && wide_batch) ? 4 : kFusedMaxWaves; };
        for (int64_t r = 0; r < Z; r++) {
            if (find((int32_t)r) != r || !cok[r] || coff[r + 1] == coff[r]) continue;
            // a cluster whose surfaces belong to more than one weather site is streamed: a workgroup (and a team) reads
            // one site's weather
            const int32_t csite = placed[csurf[coff[r]]].site;
            bool one_site = true;
            for (int64_t q = coff[r]; q < coff[r + 1]; q++) one_site = one_site && placed[csurf[q]].site == csite;
            if (!one_site) continue;
            // one blocking factor for the cluster: the cheapest that keeps every surface at two lanes or more
            // (gas cavities: 4 or 8 nodes per lane only — the 16-node cavity variant does not fit the registers)
            // Small all-no-mass surfaces (glazing, thin walls) of the cluster get wavefronts of their own in the
            // workgroup (one lane per surface); such a "mixed" workgroup runs the universal kernel variant of its
            // blocking factor: no-mass facings allowed, gas cavities allowed (up to 8 nodes per lane).
            bool any_cav = false, any_chunky = false;
            int n_small = 0;
            for (int64_t q = coff[r]; q < coff[r + 1]; q++) {
                if (is_small(csurf[q])) n_small++;
                else {
                    any_cav = any_cav || cat[csurf[q]].ncav > 0;
                    any_chunky = any_chunky || cat[csurf[q]].chunky != 0;
                }
            }
            const bool mixed = n_small > 0;
            int M = opt.nodes_per_lane;
            if (M == 16 && (any_cav || any_chunky)) continue;  // streamed
            if (any_chunky && (mixed || any_cav)) continue;     // streamed
            if (M == 0) {
                double best_cost = 0.0;
                for (int m : ms_all) {  // cheapest tiles win; on a tie the larger lanes
                    if (m == 16 && (any_cav || any_chunky)) continue;
                    int c_k[kWave + 1] = {};
                    bool ok = true;
                    for (int64_t q = coff[r]; q < coff[r + 1] && ok; q++) {
                        if (is_small(csurf[q])) continue;
                        const int kk = (placed[csurf[q]].n + m - 1) / m;
                        ok = kk >= ((m == 8 && !any_cav && !mixed) ? 1 : 2) && kk <= kWave &&  // (single-lane surfaces: 8 nodes per lane, no cavities)
                             (cat[csurf[q]].m_ok & m_bit(m)) != 0;                              // (no-mass chunks whole in their lanes)
                        if (ok) c_k[kk]++;
                    }
                    if (!ok) continue;
                    const int nt_m = tiles_needed_packed(c_k) + small_tiles(n_small);
                    if (nt_m > max_tiles(m)) continue;
                    const double t = cluster_ns(m, nt_m);
                    if (M == 0 || t <= best_cost) { M = m; best_cost = t; }
                }
                if (M == 0) M = 4;
            }
            int nm = 0, cnt[kWave + 1] = {}, ne = 0;
            bool fits = true;
            for (int64_t q = coff[r]; q < coff[r + 1]; q++) {
                const Placed &pl = placed[csurf[q]];
                ne += (zone_of_side(csurf[q], 0) >= 0) + (zone_of_side(csurf[q], 1) >= 0);
                if (is_small(csurf[q])) continue;
                const int k = (pl.n + M - 1) / M;
                if (k > kWave || k < ((M == 8 && !any_cav && !mixed) ? 1 : 2) || !(cat[csurf[q]].m_ok & m_bit(M))) { fits = false; break; }
                cnt[k]++;
                nm |= cat[csurf[q]].nm;
            }
            const int nz = (int)czones[r].size();
            if (!fits || tiles_needed_packed(cnt) + small_tiles(n_small) > max_tiles(M) || nz > kFusedMaxZones ||
                ne > kFusedMaxEntries) {
                // Too large for one workgroup: a TEAM of up to kTeamMax workgroups of four wavefronts (layout.hpp). The
                // cluster's walls are dealt to the members room by room (by the smaller zone they face), so that most
                // zones are faced from one member only; a zone faced from several is balanced from their partial sums.
                static const bool teams_off = getenv("HEAT_AMD_NO_TEAMS") != nullptr;
                if (teams_off || opt.n_ranks > 1 || mixed || any_cav || any_chunky || nz > kTeamZones) continue;  // streamed
                int Mt = opt.nodes_per_lane;
                if (Mt == 0) {
                    double best = 0.0;
                    for (int m : ms_all) {
                        bool ok = true;
                        double c = 0.0;
                        for (int64_t q = coff[r]; q < coff[r + 1] && ok; q++) {
                            const int kk = (placed[csurf[q]].n + m - 1) / m;
                            ok = kk >= (m == 8 ? 1 : 2) && kk <= kWave && (cat[csurf[q]].m_ok & m_bit(m)) != 0;
                            c += padded_cost(placed[csurf[q]].n, m);
                        }
                        if (ok && (Mt == 0 || c < best)) { Mt = m; best = c; }
                    }
                    if (Mt == 0) continue;  // streamed
                }
                std::vector<int64_t> walls(csurf.begin() + coff[r], csurf.begin() + coff[r + 1]);
                auto room_of = [&](int64_t s) {
                    const int32_t zf = zone_of_side(s, 0), zb = zone_of_side(s, 1);
                    return zf < 0 ? zb : (zb < 0 ? zf : std::min(zf, zb));
                };
                std::stable_sort(walls.begin(), walls.end(), [&](int64_t x, int64_t y) { return room_of(x) < room_of(y); });
                struct Member { std::vector<int64_t> walls; std::vector<int32_t> zones; int cnt[kWave + 1] = {}; int ne = 0; int lanes = 0; };
                std::vector<Member> mem(1);
                bool ok = true;
                int nm_t = 0;
                // even shares: as few members as the lanes need, each filled to the same level (a member of one tile
                // beside two of four holds a workgroup slot for a quarter of the work)
                int64_t all_lanes = 0;
                for (int64_t s : walls) all_lanes += (placed[s].n + Mt - 1) / Mt;
                const int want_members = (int)std::max<int64_t>(2, (all_lanes + 4 * kWave - 1) / (4 * kWave));
                const int lane_target = (int)std::min<int64_t>(4 * kWave, (all_lanes + want_members - 1) / want_members + kWave / 4);
                for (int64_t s : walls) {
                    const int kk = (placed[s].n + Mt - 1) / Mt;
                    if (kk > kWave || kk < (Mt == 8 ? 1 : 2) || !(cat[s].m_ok & m_bit(Mt))) { ok = false; break; }
                    nm_t |= cat[s].nm;
                    for (int attempt = 0; attempt < 2; attempt++) {
                        Member &me = mem.back();
                        int zadd = 0;
                        for (int side = 0; side < 2; side++) {
                            const int32_t z = zone_of_side(s, side);
                            if (z >= 0 && std::find(me.zones.begin(), me.zones.end(), z) == me.zones.end() &&
                                !(side == 1 && z == zone_of_side(s, 0))) zadd++;
                        }
                        const int eadd = (zone_of_side(s, 0) >= 0) + (zone_of_side(s, 1) >= 0);
                        me.cnt[kk]++;
                        const bool fits_m = tiles_needed_packed(me.cnt) <= 4 && (int)me.zones.size() + zadd <= kFusedMaxZones &&
                                            me.ne + eadd <= kFusedMaxEntries &&
                                            (me.lanes + kk <= lane_target || (int)mem.size() >= want_members);
                        if (!fits_m) {
                            me.cnt[kk]--;
                            if (attempt == 1 || me.walls.empty()) { ok = false; break; }
                            mem.emplace_back();
                            continue;
                        }
                        me.walls.push_back(s);
                        me.ne += eadd;
                        me.lanes += kk;
                        for (int side = 0; side < 2; side++) {
                            const int32_t z = zone_of_side(s, side);
                            if (z >= 0 && std::find(me.zones.begin(), me.zones.end(), z) == me.zones.end()) me.zones.push_back(z);
                        }
                        break;
                    }
                    if (!ok || (int)mem.size() > kTeamMax) { ok = false; break; }
                }
                if (!ok || mem.size() < 2) continue;  // streamed
                if (!fuse_always && S > 8192) {
                    // tiles, plus what the exchange costs a member per sub-timestep (it waits ~3 us of a 512-workgroup chip)
                    constexpr double kTeamExchangeNs = 6.0;
                    double t = 0.0, bytes = 0.0;
                    for (const Member &me : mem) t += cluster_ns(Mt, tiles_needed_packed(me.cnt)) + kTeamExchangeNs;
                    for (int64_t s : walls) bytes += 32.0 * placed[s].n + 152.0;
                    if (t > 0.85 * (bytes / kStreamBytesPerNs + kZoneNs * nz)) continue;  // streamed
                }
                const int cls_t = fast_class(Mt, Category{0, nm_t, 0, 1, 7});
                // exchange slot of a zone = its number in the cluster; members that face it
                std::vector<uint32_t> zmask(nz, 0);
                auto slot_of = [&](int32_t z) { return (int)(std::lower_bound(czones[r].begin(), czones[r].end(), z) - czones[r].begin()); };
                for (size_t m = 0; m < mem.size(); m++)
                    for (int32_t z : mem[m].zones) zmask[slot_of(z)] |= 1u << m;
                for (size_t m = 0; m < mem.size(); m++) {
                    BlockPlan bp{cls_t, false, mem[m].zones, n_supers, (int)m, {}};
                    for (int32_t z : mem[m].zones) bp.zinfo.push_back((uint32_t)slot_of(z) | (zmask[slot_of(z)] << 16));
                    blocks.push_back(bp);
                    for (int64_t s : mem[m].walls) {
                        placed[s].blk = (int)blocks.size() - 1;
                        placed[s].cls = cls_t;
                        placed[s].k = (placed[s].n + Mt - 1) / Mt;
                    }
                }
                n_supers++;
                continue;
            }
            if (!fuse_always) {
                // No glazing in a fused workgroup: a window's no-mass loop re-evaluates its gas cavity every pass
                // (surface.rs:814) — a long serial chain the whole workgroup would wait for at every sub-timestep's
                // barrier (rooms with double glazing: 8x slower fused than streamed). Otherwise: tiles against bytes.
                int n_cav_small = 0;
                double bytes = 0.0;
                for (int64_t q = coff[r]; q < coff[r + 1]; q++) {
                    n_cav_small += cat[csurf[q]].kind == kSmallCav;
                    bytes += 32.0 * placed[csurf[q]].n + 152.0;
                }
                const int tiles = tiles_needed_packed(cnt) + small_tiles(n_small);
                // A small batch is bound by launches and latency, not by throughput: there the resident march wins
                // with any blocking factor (one launch per march call instead of two or more per sub-timestep).
                const bool small_batch = S <= 8192;
                if (n_cav_small > 0 || tiles == 0) continue;                                        // streamed
                if (!small_batch && cluster_ns(M, tiles) > 0.85 * (bytes / kStreamBytesPerNs + kZoneNs * nz))
                    continue;                                                                       // streamed
            }
            Category cc{0, mixed ? 1 : nm, (mixed ? (M < 16) : any_cav) ? 1 : 0, 1, 7};
            const int cls = fast_class(M, cc);
            Open &o = open[{csite, 2 * cls + (mixed ? 1 : 0)}];
            int merged[kWave + 1];
            for (int k = 0; k <= kWave; k++) merged[k] = o.cnt[k] + cnt[k];
            // Workgroups of four tiles are the target (two of them share a compute unit, so one's zone balance —
            // a short serial section — overlaps the other's stencil work): clusters are merged only up to four
            // tiles; a cluster that needs five to eight gets a workgroup of its own.
            if (o.blk < 0 || tiles_needed_packed(merged) + small_tiles(o.nsmall + n_small) > 4 || o.nz + nz > kFusedMaxZones ||
                o.ne + ne > kFusedMaxEntries) {
                o = Open();
                o.blk = new_block(cls, mixed);
                for (int k = 0; k <= kWave; k++) merged[k] = cnt[k];
            }
            for (int k = 0; k <= kWave; k++) o.cnt[k] = merged[k];
            o.nsmall += n_small;
            o.nz += nz;
            o.ne += ne;
            for (int32_t z : czones[r]) blocks[o.blk].zones.push_back(z);
            for (int64_t q = coff[r]; q < coff[r + 1]; q++) {
                Placed &pl = placed[csurf[q]];
                pl.blk = o.blk;
                if (is_small(csurf[q])) {
                    pl.cls = kSmallCav;  // (one kind of small tile inside workgroups: the cavity variant covers both)
                } else {
                    pl.cls = cls;
                    pl.k = (pl.n + M - 1) / M;
                }
            }
        }
        // surfaces that face no zone: any grouping will do; workgroups of up to 4 tiles of equal k
        std::vector<int64_t> lone;
        std::vector<uint8_t> lone_ok(S, 1);
        for (int64_t s = 0; s < S; s++)
            if (sroot[s] < 0 && fusable(s) && !is_small(s)) lone.push_back(s);
        for (int64_t s : lone) {
            Placed &pl = placed[s];
            int M = opt.nodes_per_lane;
            const bool cav = cat[s].ncav > 0;
            if (M == 0) {
                M = 4;
                for (int m : {8, 16})
                    if (!(m == 16 && (cav || cat[s].chunky)) && (cat[s].m_ok & m_bit(m)) && (pl.n + m - 1) / m >= ((m == 8 && !cav) ? 1 : 2) &&
                        fused_cost(pl.n, m) <= fused_cost(pl.n, M)) M = m;
            }
            int k = (pl.n + M - 1) / M;
            const bool gains = tile_ns(M) * k / kWave < 0.85 * (32.0 * pl.n + 152.0) / kStreamBytesPerNs;
            if (k > kWave || k < ((M == 8 && !cav) ? 1 : 2) || (M == 16 && (cav || cat[s].chunky)) || (cav && cat[s].chunky) || !(cat[s].m_ok & m_bit(M)) ||
                (!fuse_always && S > 8192 && !gains)) { lone_ok[s] = 0; continue; }
            pl.cls = fast_class(M, Category{0, cat[s].nm, cav ? 1 : 0, 1, 7});
            pl.k = k;
        }
        std::stable_sort(lone.begin(), lone.end(), [&](int64_t x, int64_t y) {
            if (placed[x].cls != placed[y].cls) return placed[x].cls < placed[y].cls;
            if (placed[x].site != placed[y].site) return placed[x].site < placed[y].site;
            return placed[x].k < placed[y].k;
        });
        {
            int cur_cls = -1, cur_k = -1, cur_blk = -1, in_blk = 0, cur_site = -1;
            for (int64_t s : lone) {
                Placed &pl = placed[s];
                if (!lone_ok[s] || pl.cls >= kNumFast) continue;
                const int cap = 4 * (kWave / pl.k);
                if (pl.cls != cur_cls || pl.k != cur_k || pl.site != cur_site || in_blk >= cap) {
                    cur_cls = pl.cls; cur_k = pl.k; cur_site = pl.site; in_blk = 0;
                    cur_blk = new_block(pl.cls, false);
                }
                pl.blk = cur_blk;
                in_blk++;
            }
        }
    }
    if (fuse && !fuse_always && !blocks.empty()) {
        // A SMALL batch (bound by launches, not by throughput) is fused only as a whole: a streamed remainder would
        // still pay its launches every sub-timestep (2 000 clustered walls with 733 of them fused: 89 us per
        // sub-timestep against 64 all streamed). A large batch fuses the clusters that gain and streams the rest
        // AFTER them in the same march call, on the same stream (heat_batch_march_resident): the two kinds of kernels
        // never share the chip — side by side they did badly (1 M clustered walls with 205 000 fused: 260 against 222
        // all streamed) —, so every fused cluster keeps its gain; below a tenth of the batch's nodes the fused
        // launch's own ramp and tail are not worth it.
        double fused_nodes = 0.0, all_nodes = 0.0;
        bool remainder = false;
        for (int64_t s = 0; s < S; s++) {
            all_nodes += placed[s].n;
            if (placed[s].blk >= 0) fused_nodes += placed[s].n;
            else remainder = true;
        }
        static const double min_share = getenv("HEAT_AMD_FUSE_MIN_SHARE") ? atof(getenv("HEAT_AMD_FUSE_MIN_SHARE")) : 0.1;
        if (S <= 8192 ? remainder : fused_nodes < min_share * all_nodes) {
            placed = placed_streamed;
            blocks.clear();
        } else if (remainder) {
            // the streamed remainder keeps the blocking factors of the all-streamed plan
            for (int64_t s = 0; s < S; s++)
                if (placed[s].blk < 0) placed[s] = placed_streamed[s];
        }
    }
    for (int64_t s = 0; s < S; s++) {
        const int cls = placed[s].cls;
        p.class_counts[cls < kNumFast ? cls / 6 : (cls < kGeneral ? 3 : 4)]++;
        if (cls < kNumFast && kFastPAL[cls]) p.n_palette++;
        if (placed[s].blk >= 0) p.n_fused_surfaces++;
    }

    // ---- order: class, then streamed surfaces before the fused workgroups, then weather site, then lanes per surface ----
    // Small surfaces with a gas cavity are grouped by the branch of the Nusselt correlation their tilt selects
    // (gas.rs:197-315: five ranges of the cavity angle): the lanes of a wavefront then take the same branch instead of
    // the wavefront running all of them one after the other.
    std::vector<uint8_t> tilt_key(S, 0);
    if (d->seg_cavity && d->n_cavities > 0)
        for (int64_t s = 0; s < S; s++) {
            if (placed[s].cls != kSmallCav && !(placed[s].cls < kNumFast && kFastCAV[placed[s].cls])) continue;
            const int64_t o = d->node_offset[s];
            for (int i = 0; i < placed[s].n; i++)
                if (d->seg_cavity[o + i] >= 0) {
                    double g = std::fmod(d->cavities[d->seg_cavity[o + i]].angle, 3.14159265358979323846);
                    if (g > 1.5707963267948966) g = 3.14159265358979323846 - g;  // the kernel flips the angle by the sign of dT
                    const double deg = g * (180.0 / 3.14159265358979323846);
                    tilt_key[s] = deg < 59.5 ? 0 : (deg < 60.5 ? 1 : (deg < 89.5 ? 2 : 3));
                    break;
                }
        }
    std::vector<int64_t> order(S);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        const Placed &a = placed[x], &c = placed[y];
        if (a.cls != c.cls) return a.cls < c.cls;
        if (a.blk != c.blk) return a.blk < c.blk;
        if (a.site != c.site) return a.site < c.site;  // (a workgroup's surfaces share one already)
        if (a.cls < kNumFast && a.k != c.k) return a.k < c.k;
        if (tilt_key[x] != tilt_key[y]) return tilt_key[x] < tilt_key[y];
        if (a.cls < kNumFast) return false;
        return a.n < c.n;
    });

    // ---- tiles ----
    std::vector<FastTile> fast_tiles[kNumFast];
    std::vector<GeneralTile> gen_tiles;
    std::vector<int64_t> dev_of(S);            // original -> device surface
    std::vector<int64_t> node0_index(S), nodeN_index(S);  // index of first / last node in the T buffer
    std::vector<int64_t> orig_of(S);
    int64_t node_cursor = 0, scratch_cursor = 0;
    int64_t dcur = 0;
    size_t pos = 0;
    struct NodeMap { int64_t base; int Lk; int k; int M; int g; int tile; int lane0; };  // per device surface
    std::vector<int> blk_first_tile(blocks.size(), -1), blk_n_tiles(blocks.size(), 0);
    std::vector<int> blk_first_small(blocks.size(), -1), blk_n_small(blocks.size(), 0);
    std::vector<NodeMap> nmap(S);
    int prev_cls = -1;
    while (pos < (size_t)S) {
        const Placed &p0 = placed[order[pos]];
        if (p0.cls != prev_cls) node_cursor = (node_cursor + 15) / 16 * 16;  // class bytes are loaded 4/8/16 at a time
        prev_cls = p0.cls;
        if (p0.cls < kNumFast) {
            const int M = kFastM[p0.cls], k = p0.k;
            // A workgroup of the cluster-resident march whose surfaces differ in their lane counts packs them into
            // its wavefronts one after the other (mixed tiles, lane table behind the tile's class bytes); everything
            // else keeps tiles of one lane count, floor(64 / k) surfaces each.
            bool mixed_block = false;
            if (p0.blk >= 0) {
                for (size_t q = pos; q < (size_t)S && placed[order[q]].cls == p0.cls && placed[order[q]].blk == p0.blk &&
                                     placed[order[q]].site == p0.site; q++)
                    mixed_block = mixed_block || placed[order[q]].k != k;
            }
            const int Gmax = kWave / k;
            size_t end = pos;
            int lanes = 0;
            if (mixed_block) {
                while (end < (size_t)S && placed[order[end]].cls == p0.cls && placed[order[end]].blk == p0.blk &&
                       placed[order[end]].site == p0.site && lanes + placed[order[end]].k <= kWave) {
                    lanes += placed[order[end]].k;
                    end++;
                }
            } else {
                while (end < (size_t)S && placed[order[end]].cls == p0.cls && placed[order[end]].k == k &&
                       placed[order[end]].blk == p0.blk && placed[order[end]].site == p0.site && (int)(end - pos) < Gmax)
                    end++;
            }
            const int Lk = mixed_block ? lanes : Gmax * k;
            bool all_full = true;
            for (size_t q = pos; q < end; q++) all_full = all_full && (placed[order[q]].n == placed[order[q]].k * M);
            FastTile t;
            t.node_base = node_cursor;
            t.surf_base = (int32_t)dcur;
            bool any_chunky = false;
            for (size_t q = pos; q < end; q++) any_chunky = any_chunky || cat[order[q]].chunky;
            t.k = (int16_t)((mixed_block ? (Lk | kTileMixedBit) : k) | (all_full ? 0x100 : 0) | (any_chunky ? kTileChunkyBit : 0));
            t.G = (int16_t)(end - pos);
            const int tile_index = (int)fast_tiles[p0.cls].size();
            fast_tiles[p0.cls].push_back(t);
            if (p0.blk >= 0) {
                if (blk_first_tile[p0.blk] < 0) blk_first_tile[p0.blk] = tile_index;
                blk_n_tiles[p0.blk]++;
            } else {
                p.n_stream_tiles[p0.cls] = tile_index + 1;  // streamed tiles come first in every class
            }
            int lane0 = 0;
            for (size_t q = pos; q < end; q++) {
                const int64_t s = order[q];
                const int ks = placed[s].k;
                dev_of[s] = dcur;
                orig_of[dcur] = s;
                nmap[dcur] = NodeMap{node_cursor, Lk, ks, M, (int)(q - pos), tile_index, lane0};
                lane0 += ks;
                dcur++;
            }
            node_cursor += (int64_t)M * Lk + (mixed_block ? kLaneTableSlots : 0);
            pos = end;
        } else {
            if (gen_tiles.empty()) p.gen_base = node_cursor;
            size_t end = pos;
            while (end < (size_t)S && end < pos + (size_t)kWave && placed[order[end]].cls == p0.cls &&
                   placed[order[end]].blk == p0.blk && placed[order[end]].site == p0.site)
                end++;
            if (p0.cls < kGeneral) p.n_small_tiles++;
            if (p0.cls == kSmall) p.n_small_plain_tiles++;
            if (p0.cls == kSmallCav && p0.blk < 0) p.n_smallcav_stream_tiles++;
            if (p0.blk >= 0) {
                if (blk_first_small[p0.blk] < 0) blk_first_small[p0.blk] = (int)gen_tiles.size();
                blk_n_small[p0.blk]++;
            }
            int n_max = 0;
            for (size_t q = pos; q < end; q++) n_max = std::max(n_max, placed[order[q]].n);
            GeneralTile t;
            t.node_base = node_cursor;
            t.surf_base = (int32_t)dcur;
            t.G = (int32_t)(end - pos);
            t.n_max = n_max;
            t.pad = 0;
            t.scratch_base = scratch_cursor;
            gen_tiles.push_back(t);
            for (size_t q = pos; q < end; q++) {
                const int64_t s = order[q];
                dev_of[s] = dcur;
                orig_of[dcur] = s;
                nmap[dcur] = NodeMap{node_cursor, kWave, 1, 0, (int)(q - pos), (int)gen_tiles.size() - 1, (int)(q - pos)};
                dcur++;
            }
            node_cursor += (int64_t)n_max * kWave;
            scratch_cursor += (int64_t)kScratchArrays * n_max * kWave;
            pos = end;
        }
    }
    if (gen_tiles.empty()) p.gen_base = node_cursor;
    p.node_slots = node_cursor;
    if (node_cursor >= (int64_t)1 << 32) return failp(err, HEAT_E_SIZE, "batch too large: %lld node slots", (long long)node_cursor);

    auto node_index = [&](int64_t dsurf, int i) -> int64_t {
        const NodeMap &m = nmap[dsurf];
        if (m.M == 0) return m.base + (int64_t)i * kWave + m.g;
        const int lane = m.lane0 + i / m.M, j = i % m.M;
        return m.base + ((int64_t)(j >> 1) * m.Lk + lane) * 2 + (j & 1);
    };

    // ---- per-node constants ----
    std::vector<double> hV(node_cursor, 0.0), hU(node_cursor, 0.0);
    std::vector<uint8_t> hCls(p.n_palette ? node_cursor : 0, 0);
    // the palette width of the batch (layout.hpp): narrow unless a palette-form wall needs more entries
    static const bool tiny_off = getenv("HEAT_AMD_NO_TINY_PAL") != nullptr;  // measurement
    p.pal_stride = tiny_off ? kPalNarrow : kPalTiny;
    for (int64_t s = 0; s < S; s++)
        if (placed[s].cls < kNumFast && kFastPAL[placed[s].cls]) {
            if (cat[s].wide) p.pal_stride = kPal;
            else if (!cat[s].tiny) p.pal_stride = std::max(p.pal_stride, kPalNarrow);
        }
    p.pal_ubase = (p.pal_stride == kPal) ? kPalV : (p.pal_stride == kPalNarrow ? kPalVNarrow : kPalVTiny);
    const int pstride = p.pal_stride, ubase = p.pal_ubase;
    std::vector<double> hPal(p.n_palette ? (size_t)S * pstride : 0, 0.0);
    const int64_t gen_slots = node_cursor - p.gen_base;
    std::vector<double> hAf(gen_slots, 0.0), hAb(gen_slots, 0.0), hMass(gen_slots, 0.0);
    std::vector<int32_t> hCav(gen_slots, -1);
    for (int64_t dd = 0; dd < S; dd++) {
        const int64_t s = orig_of[dd];
        const int64_t o = d->node_offset[s];
        const int n = placed[s].n;
        const bool gen = placed[s].cls >= kNumFast;
        const bool pal = !gen && kFastPAL[placed[s].cls];
        int nv = 1, nu = 1;
        double *pp = pal ? &hPal[(size_t)dd * pstride] : nullptr;
        for (int i = 0; i < n; i++) {
            const int64_t idx = node_index(dd, i);
            const double mass = d->mass[o + i];
            hV[idx] = (mass >= kMassThreshold) ? d->dt / mass : 0.0;  // dt / C, surface.rs:172
            const bool cav = d->seg_cavity && d->n_cavities > 0 && d->seg_cavity[o + i] >= 0;
            hU[idx] = cav ? 0.0 : d->uvalue[o + i];
            if (pal) {
                int vc = -1, uc = -1;
                for (int q = 0; q < nv; q++) if (pp[q] == hV[idx]) vc = q;
                if (vc < 0) { vc = nv; pp[nv++] = hV[idx]; }
                for (int q = 0; q < nu; q++) if (pp[ubase + q] == hU[idx]) uc = q;
                if (uc < 0) { uc = nu; pp[ubase + nu++] = hU[idx]; }
                const NodeMap &m = nmap[dd];
                const int lane = m.lane0 + i / m.M, j = i % m.M;
                hCls[m.base + (int64_t)lane * m.M + j] = (uint8_t)(vc | (uc << kPalUShift));
            }
            if (gen) {
                const int64_t gi = idx - p.gen_base;
                hAf[gi] = d->front_alpha[o + i];
                hAb[gi] = d->back_alpha[o + i];
                hMass[gi] = mass;
                hCav[gi] = cav ? d->seg_cavity[o + i] : -1;
            }
        }
        node0_index[s] = node_index(dd, 0);
        nodeN_index[s] = node_index(dd, n - 1);
    }
    p.node_tile_base.resize(S);
    p.node_geom.resize(S);
    for (int64_t dd = 0; dd < S; dd++) {  // (node_slot_index, plan.hpp, is node_index for the rest of the library)
        const NodeMap &m = nmap[dd];
        p.node_tile_base[orig_of[dd]] = m.base;
        p.node_geom[orig_of[dd]] = (int32_t)(m.Lk | (m.M << 8) | ((m.M == 0 ? m.g : m.lane0) << 16));
    }

    // ---- no-mass chunk marks: V index 14 / 15 in the class byte of a chunk's first node = one / two nodes (kernels.hip) ----
    if (!hCls.empty())
        for (int64_t dd = 0; dd < S; dd++) {
            const int64_t s = orig_of[dd];
            if (!(placed[s].cls < kNumFast && kFastPAL[placed[s].cls] && cat[s].nm)) continue;
            const int64_t o = d->node_offset[s];
            const NodeMap &m = nmap[dd];
            for (int i = 0; i < placed[s].n;) {
                if (d->mass[o + i] >= kMassThreshold) { i++; continue; }
                int e = i;
                while (e < placed[s].n && d->mass[o + e] < kMassThreshold) e++;
                hCls[m.base + (int64_t)(m.lane0 + i / m.M) * m.M + i % m.M] |= (uint8_t)(kPalVMark1 - 1 + (e - i));  // (its V index is 0)
                i = e;
            }
        }

    // ---- lane tables of the mixed tiles: behind the tile's class bytes, one 16-bit entry per lane ----
    for (int c = 0; c < kNumFast; c++)
        for (const FastTile &ft : fast_tiles[c]) {
            if (!(ft.k & kTileMixedBit)) continue;
            const int M = kFastM[c], Lk = ft.k & 0xff;
            uint8_t *tab = &hCls[ft.node_base + (int64_t)M * Lk];
            int lane = 0;
            for (int g = 0; g < ft.G; g++) {
                const int ks = nmap[ft.surf_base + g].k;
                for (int seg = 0; seg < ks; seg++, lane++) {
                    const uint16_t e = (uint16_t)(g | (seg << 6) | (seg == ks - 1 ? kLaneLastBit : 0));
                    tab[2 * lane] = (uint8_t)(e & 0xff);
                    tab[2 * lane + 1] = (uint8_t)(e >> 8);
                }
            }
        }

    // ---- cavity references of the CAV fast classes ----
    std::vector<int32_t> hCavRef;
    {
        bool any = false;
        for (int64_t s = 0; s < S; s++) any = any || (placed[s].cls < kNumFast && kFastCAV[placed[s].cls]);
        if (any) {
            hCavRef.assign((size_t)4 * S, -1);
            for (int64_t dd = 0; dd < S; dd++) {
                const int64_t s = orig_of[dd];
                if (!(placed[s].cls < kNumFast && kFastCAV[placed[s].cls])) continue;
                const int64_t o = d->node_offset[s];
                int r = 0;
                for (int i = 0; i < placed[s].n && r < 2 && d->seg_cavity && d->n_cavities > 0; i++)
                    if (d->seg_cavity[o + i] >= 0) {
                        hCavRef[4 * dd + 2 * r] = i;
                        hCavRef[4 * dd + 2 * r + 1] = d->seg_cavity[o + i];
                        r++;
                    }
            }
        }
    }

    // ---- per-side records (device order) ----
    std::vector<int32_t> hMeta(S);
    std::vector<SideConst> hSide(2 * S);
    std::vector<double> hAlpha(2 * S, 1.0);
    std::vector<double> hFix;
    std::vector<int64_t> hFirst(S), hSlots(8 * S);
    const bool has_fix = d->front_hs_fix != nullptr;
    if (has_fix) hFix.resize(2 * S);
    for (int64_t dd = 0; dd < S; dd++) {
        const int64_t s = orig_of[dd];
        const int64_t o = d->node_offset[s];
        const int n = placed[s].n;
        hMeta[dd] = n;
        const double cos_tilt = d->cos_tilt[s];
        // is_windward: only tilted surfaces test the wind direction (surface.rs:38)
        const int always_windward = (std::fabs(cos_tilt) < 0.98) ? 0 : 4;
        // forced convection: 2.537 * Wf * Rf * sqrt(P * V_z / A), Rf = COEFFICIENTS[1] = 1.67, V_z = wind * modifier
        // (convection.rs:151-168; surface.rs:646,691). Wf and sqrt(wind) are applied per sub-timestep.
        const double forced = 2.537 * 1.67 * std::sqrt(d->perimeter[s] * d->wind_modifier[s] / d->area[s]);
        for (int side = 0; side < 2; side++) {
            SideConst c;
            const int kind = side ? d->back_kind[s] : d->front_kind[s];
            const int peer = side ? d->front_kind[s] : d->back_kind[s];  // the surface's other side (layout.hpp)
            c.kind_n = kind | always_windward | ((peer & 3) << 4) | (n << 16);
            c.zone = kind == HEAT_BOUNDARY_SPACE ? (side ? d->back_zone[s] : d->front_zone[s]) : 0;
            c.ambient = side ? d->back_ambient[s] : d->front_ambient[s];
            c.emis = side ? d->back_emissivity[s] : d->front_emissivity[s];
            c.alpha = side ? d->back_alpha[o + n - 1] : d->front_alpha[o];
            // front Outdoor flips the sign (surface.rs:652); back Outdoor does not (surface.rs:689-696)
            c.cos_eff = (side == 0 && kind == HEAT_BOUNDARY_OUTDOOR) ? -cos_tilt : cos_tilt;
            hAlpha[(int64_t)side * S + dd] = 1.0;
            if (placed[s].cls < kNumFast) {
                // fast classes: the absorptance goes into SideDyn::solar at upload; the two slots carry the TARP
                // natural-convection coefficients of convection.rs:87-110 with the tilt-dependent division done here
                hAlpha[(int64_t)side * S + dd] = c.alpha;
                const double ce = c.cos_eff, act = std::fabs(ce);
                const double up = 9.482 / (7.238 - act), down = 1.81 / (1.382 + act);
                double pos, neg;  // air warmer / colder than the surface
                if (ce != ce) { pos = neg = ce; }
                else if (act < 1e-3) { pos = neg = 1.31; }
                else if (ce > 0.) { pos = up; neg = down; }
                else { pos = down; neg = up; }
                c.cos_eff = pos;
                c.alpha = neg;
            }
            // (a Space-facing side carries the surface's area here: what its contribution to the zone is weighted with)
            c.forced = kind == HEAT_BOUNDARY_OUTDOOR ? forced : (kind == HEAT_BOUNDARY_SPACE ? d->area[s] : 0.0);
            if (side == 1 && kind == HEAT_BOUNDARY_AMBIENT) {
                // A back side facing an ambient temperature takes t_front for its radiant temperature
                // (surface.rs:672-686): the FRONT side's boundary source travels in this record's unused slots, so that
                // the kernels need no second record (a dependent load in front of every tile that holds such a wall)
                if (peer == HEAT_BOUNDARY_SPACE) c.zone = d->front_zone[s];
                if (peer == HEAT_BOUNDARY_AMBIENT) c.forced = d->front_ambient[s];
            }
            c.nx = d->normal_x[s];
            c.ny = d->normal_y[s];
            hSide[(int64_t)side * S + dd] = c;
            if (has_fix) hFix[(int64_t)side * S + dd] = side ? d->back_hs_fix[s] : d->front_hs_fix[s];
        }
        hFirst[dd] = d->first_node_slot[s];
        const int64_t *src[8] = {d->hs_front_slot, d->hs_back_slot, d->flow_front_slot, d->flow_back_slot,
                                 d->solar_front_slot, d->solar_back_slot, d->ir_front_slot, d->ir_back_slot};
        for (int a = 0; a < 8; a++) hSlots[(int64_t)a * S + dd] = src[a][s];
    }

    // ---- zone contribution lists, in the reference's order (model.rs:562-585) ----
    std::vector<int64_t> zoff(Z + 1, 0);
    for (int64_t s = 0; s < S; s++) {
        if (d->front_kind[s] == HEAT_BOUNDARY_SPACE) zoff[d->front_zone[s] + 1]++;
        if (d->back_kind[s] == HEAT_BOUNDARY_SPACE) zoff[d->back_zone[s] + 1]++;
    }
    for (int64_t z = 0; z < Z; z++) zoff[z + 1] += zoff[z];
    std::vector<ZoneEntry> zent(Z > 0 ? zoff[Z] : 0);
    {
        std::vector<int64_t> cur(zoff.begin(), zoff.end() - (Z >= 0 ? 1 : 0));
        // a Space-facing side keeps its position in the zone's list where an ambient side keeps its temperature
        auto put_pos = [&](int64_t rec, int64_t pos) {
            static_assert(sizeof(int64_t) == sizeof(double), "entry position is stored in the ambient slot");
            memcpy(&hSide[rec].ambient, &pos, sizeof pos);
        };
        for (int64_t s = 0; s < S; s++) {
            if (d->front_kind[s] == HEAT_BOUNDARY_SPACE) {
                ZoneEntry e{(uint32_t)node0_index[s], (uint32_t)dev_of[s], d->area[s]};
                put_pos(dev_of[s], cur[d->front_zone[s]]);
                zent[cur[d->front_zone[s]]++] = e;
            }
            if (d->back_kind[s] == HEAT_BOUNDARY_SPACE) {
                ZoneEntry e{(uint32_t)nodeN_index[s], (uint32_t)(S + dev_of[s]), d->area[s]};
                put_pos(S + dev_of[s], cur[d->back_zone[s]]);
                zent[cur[d->back_zone[s]]++] = e;
            }
        }
    }

    // ---- cluster-resident march: workgroup tables ----
    std::vector<int32_t> fz, fz_eoff(1, 0);
    std::vector<uint16_t> fent;
    std::vector<double> side_area(2 * S, 0.0);
    std::vector<int16_t> side_lz(2 * S, -1);
    p.zone_block.assign(Z, -1);
    p.any_fused = false;
    std::vector<uint32_t> fteam;
    if (!blocks.empty()) {
        std::vector<int> blk_fw(blocks.size(), 4);
        std::vector<int32_t> blk_first_zone(blocks.size(), 0);
        for (size_t bi = 0; bi < blocks.size(); bi++) {
            if (blk_n_tiles[bi] + blk_n_small[bi] <= 0) continue;  // (an empty plan: cannot happen, kept harmless)
            blk_fw[bi] = blk_n_tiles[bi] + blk_n_small[bi] <= 4 ? 4 : 8;
            blk_first_zone[bi] = (int32_t)fz.size();
            for (size_t j = 0; j < blocks[bi].zones.size(); j++) {
                const int32_t z = blocks[bi].zones[j];
                p.zone_block[z] = (int32_t)bi;
                fz.push_back(z);
                fteam.push_back(blocks[bi].super >= 0 ? blocks[bi].zinfo[j] : 0u);
            }
        }
        // (a zone belongs to ONE workgroup's list, except in a team, where every member that faces it lists it: the
        // place of zone z in workgroup bi's list is looked up there — the lists are short)
        auto local_zone = [&](int bi, int32_t z) -> int32_t {
            const std::vector<int32_t> &zl = blocks[bi].zones;
            return (int32_t)(std::find(zl.begin(), zl.end(), z) - zl.begin());
        };
        // contributions in the reference's order inside each zone (model.rs:562-585): counting sort by fused zone
        std::vector<int32_t> cnt(fz.size() + 1, 0);
        auto side_zone = [&](int64_t s, int side) -> int32_t {
            const int kind = side ? d->back_kind[s] : d->front_kind[s];
            const int32_t z = kind == HEAT_BOUNDARY_SPACE ? (side ? d->back_zone[s] : d->front_zone[s]) : -1;
            return (z >= 0 && placed[s].blk >= 0) ? z : -1;
        };
        for (int64_t s = 0; s < S; s++)
            for (int side = 0; side < 2; side++) {
                const int32_t z = side_zone(s, side);
                if (z >= 0) cnt[blk_first_zone[placed[s].blk] + local_zone(placed[s].blk, z) + 1]++;
            }
        for (size_t i = 0; i < fz.size(); i++) cnt[i + 1] += cnt[i];
        fz_eoff.assign(cnt.begin(), cnt.end());
        fent.resize(cnt[fz.size()]);
        std::vector<int32_t> cur(cnt.begin(), cnt.end() - 1);
        for (int64_t s = 0; s < S; s++)
            for (int side = 0; side < 2; side++) {
                const int32_t z = side_zone(s, side);
                if (z < 0) continue;
                const int bi = placed[s].blk;
                const NodeMap &m = nmap[dev_of[s]];
                // fast-path surfaces: the first / last lane of the surface owns the side; small surfaces: their lane
                const int lane = (m.M == 0) ? m.g : (side ? (m.lane0 + m.k - 1) : m.lane0);
                const int wave_in_block = (m.M == 0) ? blk_n_tiles[bi] + (m.tile - blk_first_small[bi])
                                                     : (m.tile - blk_first_tile[bi]);
                const uint32_t slot = (uint32_t)(side * kWave * blk_fw[bi] + wave_in_block * kWave + lane);
                const int32_t lz = local_zone(bi, z);
                fent[cur[blk_first_zone[bi] + lz]++] = (uint16_t)slot;
                side_lz[(int64_t)side * S + dev_of[s]] = (int16_t)lz;
            }
        int cur_super = -1;
        for (size_t bi = 0; bi < blocks.size(); bi++) {
            if (blk_n_tiles[bi] + blk_n_small[bi] <= 0) continue;
            FusedBlock fb{std::max(blk_first_tile[bi], 0), blk_n_tiles[bi], blk_first_zone[bi],
                          (int32_t)blocks[bi].zones.size(), std::max(blk_first_small[bi], 0), blk_n_small[bi]};
            if (blocks[bi].super >= 0) {
                // a team's members follow each other (they were planned in a row): one FusedSuper per team
                std::vector<FusedBlock> &tb = p.team_blocks[blocks[bi].cls];
                if (blocks[bi].super != cur_super) {
                    cur_super = blocks[bi].super;
                    p.team_supers[blocks[bi].cls].push_back(FusedSuper{(int32_t)tb.size(), 0});
                }
                p.team_supers[blocks[bi].cls].back().n_members++;
                tb.push_back(fb);
            } else {
                p.fblocks[blocks[bi].cls][(blk_fw[bi] == 4 ? 0 : 1) + (blocks[bi].mixed ? 2 : 0)].push_back(fb);
            }
            p.any_fused = true;
        }
    }
    p.team_zinfo = std::move(fteam);
    // zones this batch's surfaces touch (for sharded batches)
    p.touched.assign(Z, 0);
    for (int64_t z = 0; z < Z; z++) p.touched[z] = zoff[z + 1] > zoff[z] ? 1 : 0;

    // ---- what the plan hands over ----
    for (int c = 0; c < kNumFast; c++) p.fast_tiles[c] = std::move(fast_tiles[c]);
    p.gen_tiles = std::move(gen_tiles);
    p.scratch_slots = scratch_cursor;
    p.fzones = std::move(fz);
    p.fzone_eoff = std::move(fz_eoff);
    p.fslots = std::move(fent);
    for (int64_t dd = 0; dd < S; dd++) side_area[dd] = side_area[S + dd] = d->area[orig_of[dd]];
    p.side_area = std::move(side_area);
    p.side_lzone = std::move(side_lz);
    p.V = std::move(hV);
    p.U = std::move(hU);
    p.cls = std::move(hCls);
    p.pal = std::move(hPal);
    p.alpha_f = std::move(hAf);
    p.alpha_b = std::move(hAb);
    p.mass = std::move(hMass);
    p.cav_idx = std::move(hCav);
    p.cavref = std::move(hCavRef);
    p.cavs.resize(d->n_cavities);
    for (int64_t c = 0; c < d->n_cavities; c++) {
        const heat_cavity &x = d->cavities[c];
        if (x.gas < 0 || x.gas > 3) return failp(err, HEAT_E_INVALID_ARG, "cavity %lld: unknown gas", (long long)c);
        p.cavs[c] = CavityDev{x.thickness, x.height, x.angle, x.eout, x.ein, x.gas, 0};
    }
    p.meta = std::move(hMeta);
    p.side = std::move(hSide);
    p.side_alpha = std::move(hAlpha);
    p.hs_fix = std::move(hFix);
    p.first_slot = std::move(hFirst);
    p.slots = std::move(hSlots);
    if (site_of_surface) {
        p.dev_site.resize(S);
        for (int64_t dd = 0; dd < S; dd++) p.dev_site[dd] = placed[orig_of[dd]].site;
    }
    p.dev_of = std::move(dev_of);
    p.orig_of = std::move(orig_of);
    p.zone_off = std::move(zoff);
    p.zone_entries = std::move(zent);
    p.zone_slot.assign(Z, 0);
    p.zone_vol.assign(Z, 0.0);
    for (int64_t z = 0; z < Z; z++) { p.zone_slot[z] = d->zone_slot[z]; p.zone_vol[z] = d->zone_volume[z]; }
    p.h_first_slot.assign(d->first_node_slot, d->first_node_slot + S);
    p.h_node_count.resize(S);
    for (int64_t s = 0; s < S; s++) p.h_node_count[s] = placed[s].n;
    p.h_out_slots[0].assign(d->hs_front_slot, d->hs_front_slot + S);
    p.h_out_slots[1].assign(d->hs_back_slot, d->hs_back_slot + S);
    p.h_out_slots[2].assign(d->flow_front_slot, d->flow_front_slot + S);
    p.h_out_slots[3].assign(d->flow_back_slot, d->flow_back_slot + S);
    {   // no-mass pass counters: one slot per tile of the NM fast classes, one per lane of the general-layout tiles
        size_t n = 0;
        for (int c = 0; c < kNumFast; c++) {
            p.nm_count_base[c] = n;
            if (kFastNM[c]) n += p.fast_tiles[c].size();
        }
        p.nm_count_base[kNumFast] = n;
        n += p.gen_tiles.size() * (size_t)kWave;
        p.n_nm_counters = std::max<size_t>(n, 1);
    }
    return HEAT_OK;
}

// ---------------------------------------------------------------------------
// Zone-connected clusters: zones joined by a Space/Space wall belong together (model.rs:556-590).
void find_clusters(const heat_batch_desc *d, std::vector<int32_t> &cluster_of_surface,
                   std::vector<int32_t> &cluster_of_zone, int32_t &n_clusters) {
    const int64_t S = d->n_surfaces, Z = d->n_zones;
    std::vector<int32_t> uf(Z);
    std::iota(uf.begin(), uf.end(), 0);
    auto find = [&](int32_t x) {
        while (uf[x] != x) { uf[x] = uf[uf[x]]; x = uf[x]; }
        return x;
    };
    auto zone_of_side = [&](int64_t s, int side) -> int32_t {
        const int kind = side ? d->back_kind[s] : d->front_kind[s];
        return kind == HEAT_BOUNDARY_SPACE ? (side ? d->back_zone[s] : d->front_zone[s]) : -1;
    };
    for (int64_t s = 0; s < S; s++) {
        const int32_t zf = zone_of_side(s, 0), zb = zone_of_side(s, 1);
        if (zf >= 0 && zb >= 0) {
            const int32_t a = find(zf), c = find(zb);
            if (a != c) uf[std::max(a, c)] = std::min(a, c);
        }
    }
    cluster_of_zone.assign(Z, -1);
    n_clusters = 0;
    for (int64_t z = 0; z < Z; z++) {  // roots are the smallest zone of their cluster: ids follow zone order
        const int32_t r = find((int32_t)z);
        if (cluster_of_zone[r] < 0) cluster_of_zone[r] = n_clusters++;
        cluster_of_zone[z] = cluster_of_zone[r];
    }
    cluster_of_surface.assign(S, -1);
    for (int64_t s = 0; s < S; s++) {
        const int32_t zf = zone_of_side(s, 0), zb = zone_of_side(s, 1);
        const int32_t z = zf >= 0 ? zf : zb;
        if (z >= 0) cluster_of_surface[s] = cluster_of_zone[z];
    }
}

// ---------------------------------------------------------------------------
// the cluster-resident march runs surfaces of one lane in the 8-node classes without cavities only (kernels.hip)
static bool single_lane_class(int c) { return kFastM[c] == 8 && !kFastCAV[c]; }

int check_plan(const Plan &p, const heat_batch_desc *d, std::string &err, const int32_t *site_of_surface) {
#define PLAN_REQUIRE(cond, ...) \
    do { if (!(cond)) return failp(err, HEAT_E_SIZE, "plan check failed: " __VA_ARGS__); } while (0)
    const int64_t S = p.n_surf, Z = p.n_zones;
    PLAN_REQUIRE(S == d->n_surfaces && Z == d->n_zones, "counts");
    PLAN_REQUIRE((int64_t)p.dev_of.size() == S && (int64_t)p.orig_of.size() == S, "permutation size");
    for (int64_t s = 0; s < S; s++) {
        PLAN_REQUIRE(p.dev_of[s] >= 0 && p.dev_of[s] < S, "dev_of[%lld] = %lld", (long long)s, (long long)p.dev_of[s]);
        PLAN_REQUIRE(p.orig_of[p.dev_of[s]] == s, "orig_of is not the inverse of dev_of at %lld", (long long)s);
    }
    PLAN_REQUIRE((int64_t)p.side.size() == 2 * S && (int64_t)p.meta.size() == S, "side / meta size");
    PLAN_REQUIRE((int64_t)p.V.size() == p.node_slots && (int64_t)p.U.size() == p.node_slots, "V / U size");
    PLAN_REQUIRE(p.cls.empty() || (int64_t)p.cls.size() == p.node_slots, "class bytes size");
    PLAN_REQUIRE((p.pal_stride == kPalTiny && p.pal_ubase == kPalVTiny) || (p.pal_stride == kPalNarrow && p.pal_ubase == kPalVNarrow) ||
                     (p.pal_stride == kPal && p.pal_ubase == kPalV),
                 "palette stride %d, U entries from %d", p.pal_stride, p.pal_ubase);
    PLAN_REQUIRE(p.pal.empty() || (int64_t)p.pal.size() == S * p.pal_stride, "palette size");
    // tiles: every device surface in exactly one tile; node ranges inside the buffers and disjoint
    std::vector<uint8_t> covered(S, 0);
    std::vector<std::pair<int64_t, int64_t>> ranges;
    for (int c = 0; c < kNumFast; c++) {
        const int M = kFastM[c];
        PLAN_REQUIRE(p.n_stream_tiles[c] >= 0 && p.n_stream_tiles[c] <= (int)p.fast_tiles[c].size(), "class %d: streamed tiles", c);
        for (size_t t = 0; t < p.fast_tiles[c].size(); t++) {
            const FastTile &ft = p.fast_tiles[c][t];
            const bool mixed = (ft.k & kTileMixedBit) != 0;
            const int k = ft.k & 0xff;  // lanes per surface; mixed: lanes of the tile
            PLAN_REQUIRE(k >= 1 && k <= kWave && ft.G >= 1 && (mixed ? ft.G <= k : ft.G * k <= kWave), "class %d tile %zu: k %d G %d", c, t, k, (int)ft.G);
            const int Lk = mixed ? k : (kWave / k) * k;
            const int64_t extent = (int64_t)M * Lk + (mixed ? kLaneTableSlots : 0);
            PLAN_REQUIRE(ft.node_base >= 0 && ft.node_base + extent <= p.node_slots && ft.node_base % 2 == 0,
                         "class %d tile %zu: node range", c, t);
            PLAN_REQUIRE(ft.node_base + extent <= p.gen_base, "class %d tile %zu reaches into the general group", c, t);
            ranges.push_back({ft.node_base, ft.node_base + extent});
            PLAN_REQUIRE(ft.surf_base >= 0 && ft.surf_base + ft.G <= S, "class %d tile %zu: surfaces", c, t);
            PLAN_REQUIRE(!mixed || (kFastPAL[c] && !p.cls.empty()), "mixed tile outside the palette classes");
            int lane0 = 0;
            for (int g = 0; g < ft.G; g++) {
                const int64_t dd = ft.surf_base + g;
                PLAN_REQUIRE(!covered[dd], "device surface %lld in two tiles", (long long)dd);
                covered[dd] = 1;
                const int n = p.meta[dd];
                const int ks = (n + M - 1) / M;
                PLAN_REQUIRE(n >= 1 && (mixed ? lane0 + ks <= Lk : ks == k), "class %d tile %zu: surface of %d nodes, %d lanes of %d", c, t, n, k, M);
                if (!mixed) lane0 = g * k;
                if (ft.k & 0x100) PLAN_REQUIRE(n == ks * M, "class %d tile %zu marked full", c, t);
                if (mixed) {
                    const uint8_t *tab = &p.cls[ft.node_base + (int64_t)M * Lk];
                    for (int seg = 0; seg < ks; seg++) {
                        const int e = tab[2 * (lane0 + seg)] | (tab[2 * (lane0 + seg) + 1] << 8);
                        PLAN_REQUIRE((e & 63) == g && ((e >> 6) & 63) == seg && ((e & kLaneLastBit) != 0) == (seg == ks - 1),
                                     "class %d tile %zu: lane table entry of lane %d", c, t, lane0 + seg);
                    }
                }
                if (kFastPAL[c]) {
                    PLAN_REQUIRE(!p.cls.empty(), "palette class without class bytes");
                    for (int i = 0; i < n; i++) {
                        const int lane = lane0 + i / M, j = i % M;
                        const uint8_t cb = p.cls[ft.node_base + (int64_t)lane * M + j];
                        const int vi = cb & (kPalV - 1), ui = (cb >> kPalUShift) & (kPalU - 1);
                        PLAN_REQUIRE((vi < p.pal_ubase || vi >= kPalVMark1) && ui < p.pal_stride - p.pal_ubase && cb < 128 &&
                                     (vi != kPalVMark1 + 1 || j + 1 < M), "class byte %d", (int)cb);
                    }
                }
                if (mixed) lane0 += ks;
            }
            PLAN_REQUIRE(!mixed || lane0 == Lk, "class %d tile %zu: %d lanes used, %d declared", c, t, lane0, Lk);
        }
    }
    PLAN_REQUIRE(p.n_small_plain_tiles <= p.n_small_tiles && p.n_small_tiles <= (int)p.gen_tiles.size(), "small tile counts");
    for (size_t t = 0; t < p.gen_tiles.size(); t++) {
        const GeneralTile &gt = p.gen_tiles[t];
        PLAN_REQUIRE(gt.G >= 1 && gt.G <= kWave && gt.n_max >= 1, "general tile %zu: G %d n_max %d", t, gt.G, gt.n_max);
        PLAN_REQUIRE(gt.node_base >= p.gen_base && gt.node_base + (int64_t)gt.n_max * kWave <= p.node_slots, "general tile %zu: node range", t);
        PLAN_REQUIRE(gt.scratch_base >= 0 && gt.scratch_base + (int64_t)kScratchArrays * gt.n_max * kWave <= p.scratch_slots,
                     "general tile %zu: scratch range", t);
        ranges.push_back({gt.node_base, gt.node_base + (int64_t)gt.n_max * kWave});
        PLAN_REQUIRE(gt.surf_base >= 0 && gt.surf_base + gt.G <= S, "general tile %zu: surfaces", t);
        for (int g = 0; g < gt.G; g++) {
            const int64_t dd = gt.surf_base + g;
            PLAN_REQUIRE(!covered[dd], "device surface %lld in two tiles", (long long)dd);
            covered[dd] = 1;
            PLAN_REQUIRE(p.meta[dd] <= gt.n_max, "general tile %zu: surface longer than n_max", t);
            if ((int)t < p.n_small_tiles) PLAN_REQUIRE(p.meta[dd] <= 4, "small tile %zu holds a surface of %d nodes", t, p.meta[dd]);
        }
    }
    for (int64_t dd = 0; dd < S; dd++) PLAN_REQUIRE(covered[dd], "device surface %lld in no tile", (long long)dd);
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); i++)
        PLAN_REQUIRE(ranges[i].first >= ranges[i - 1].second, "node ranges of two tiles overlap at slot %lld", (long long)ranges[i].first);
    for (int64_t dd = 0; dd < S; dd++) {
        const int64_t s = p.orig_of[dd];
        const int n = (int)(d->node_offset[s + 1] - d->node_offset[s]);
        PLAN_REQUIRE(p.meta[dd] == n && (p.side[dd].kind_n >> 16) == n && (p.side[S + dd].kind_n >> 16) == n, "node count of device surface %lld", (long long)dd);
        PLAN_REQUIRE((p.side[dd].kind_n & 3) == d->front_kind[s] && (p.side[S + dd].kind_n & 3) == d->back_kind[s], "boundary kinds of device surface %lld", (long long)dd);
        PLAN_REQUIRE(((p.side[dd].kind_n >> 4) & 3) == d->back_kind[s] && ((p.side[S + dd].kind_n >> 4) & 3) == d->front_kind[s], "peer kinds of device surface %lld", (long long)dd);
        PLAN_REQUIRE(p.side[dd].zone >= 0 && p.side[S + dd].zone >= 0 && (p.n_zones == 0 || (p.side[dd].zone < p.n_zones && p.side[S + dd].zone < p.n_zones)), "zone fields of device surface %lld (read unconditionally)", (long long)dd);
    }
    // zone contribution lists: one entry per Space-facing side, each side knows its place
    PLAN_REQUIRE((int64_t)p.zone_off.size() == Z + 1 && p.zone_off[0] == 0, "zone offsets");
    for (int64_t z = 0; z < Z; z++) PLAN_REQUIRE(p.zone_off[z + 1] >= p.zone_off[z], "zone offsets not monotone at %lld", (long long)z);
    PLAN_REQUIRE((int64_t)p.zone_entries.size() == (Z > 0 ? p.zone_off[Z] : 0), "zone entries size");
    int64_t n_space_sides = 0;
    for (int64_t rec = 0; rec < 2 * S; rec++) {
        const SideConst &c = p.side[rec];
        if ((c.kind_n & 3) != KIND_SPACE) continue;
        n_space_sides++;
        int64_t pos;
        memcpy(&pos, &c.ambient, sizeof pos);
        PLAN_REQUIRE(c.zone >= 0 && c.zone < Z, "side record %lld: zone", (long long)rec);
        PLAN_REQUIRE(pos >= p.zone_off[c.zone] && pos < p.zone_off[c.zone + 1], "side record %lld: entry position %lld outside its zone's list", (long long)rec, (long long)pos);
        PLAN_REQUIRE((int64_t)p.zone_entries[pos].hs_index == rec, "side record %lld: entry %lld belongs to record %u", (long long)rec, (long long)pos, p.zone_entries[pos].hs_index);
        PLAN_REQUIRE((int64_t)p.zone_entries[pos].t_index < p.node_slots, "entry %lld: face node index", (long long)pos);
    }
    // where the series march finds a surface's nodes (probes, own-face term): inside the T buffer, no two nodes in one
    // place
    PLAN_REQUIRE((int64_t)p.node_tile_base.size() == S && (int64_t)p.node_geom.size() == S, "node placement tables");
    for (const ZoneEntry &e : p.zone_entries) {  // (the zone lists name the same face nodes)
        const int64_t s = p.orig_of[e.hs_index % S];
        const int n = (int)(d->node_offset[s + 1] - d->node_offset[s]);
        PLAN_REQUIRE((int64_t)e.t_index == node_slot_index(p.node_tile_base[s], p.node_geom[s], (int64_t)e.hs_index >= S ? n - 1 : 0),
                     "surface %lld: face node of its zone entry is not where its nodes are placed", (long long)s);
    }
    {
        std::vector<uint8_t> taken((size_t)p.node_slots, 0);
        for (int64_t s = 0; s < S; s++) {
            const int n = (int)(d->node_offset[s + 1] - d->node_offset[s]);
            for (int i = 0; i < n; i++) {
                const int64_t idx = node_slot_index(p.node_tile_base[s], p.node_geom[s], i);
                PLAN_REQUIRE(idx >= 0 && idx < p.node_slots, "surface %lld node %d: placed outside the T buffer", (long long)s, i);
                PLAN_REQUIRE(!taken[idx], "surface %lld node %d: shares its place with another node", (long long)s, i);
                taken[idx] = 1;
            }
        }
    }
    PLAN_REQUIRE(n_space_sides == (int64_t)p.zone_entries.size(), "%lld Space-facing sides, %zu entries", (long long)n_space_sides, p.zone_entries.size());
    // cluster-resident march: workgroups inside the kernel's limits
    PLAN_REQUIRE((int64_t)p.zone_block.size() == Z, "zone_block size");
    PLAN_REQUIRE(p.fzone_eoff.size() == p.fzones.size() + 1, "fused zone offsets");
    int64_t fused_surfaces = 0;
    std::vector<uint8_t> zone_seen(Z, 0);
    for (int c = 0; c < kNumFast; c++)
        for (int g2 = 0; g2 < 4; g2++)
            for (const FusedBlock &fb : p.fblocks[c][g2]) {
                const int fw = (g2 & 1) ? 8 : 4;
                PLAN_REQUIRE(fb.n_tiles >= 0 && fb.n_small >= 0 && fb.n_tiles + fb.n_small >= 1 && fb.n_tiles + fb.n_small <= fw,
                             "class %d list %d: workgroup of %d + %d wavefronts", c, g2, fb.n_tiles, fb.n_small);
                PLAN_REQUIRE((g2 >> 1) || fb.n_small == 0, "plain workgroup with small-surface tiles");
                PLAN_REQUIRE(fb.first_tile >= p.n_stream_tiles[c] && fb.first_tile + fb.n_tiles <= (int)p.fast_tiles[c].size(), "class %d list %d: tile range", c, g2);
                PLAN_REQUIRE(fb.n_small == 0 || (fb.first_small >= p.n_small_plain_tiles + p.n_smallcav_stream_tiles &&
                                                 fb.first_small + fb.n_small <= p.n_small_tiles), "class %d list %d: small tile range", c, g2);
                PLAN_REQUIRE(fb.n_zones >= 0 && fb.n_zones <= kFusedMaxZones && fb.first_zone >= 0 &&
                             fb.first_zone + fb.n_zones <= (int)p.fzones.size(), "class %d list %d: zone range", c, g2);
                const int e0 = p.fzone_eoff[fb.first_zone], e1 = p.fzone_eoff[fb.first_zone + fb.n_zones];
                PLAN_REQUIRE(e1 - e0 <= kFusedMaxEntries && e1 <= (int)p.fslots.size(), "class %d list %d: %d zone-facing sides", c, g2, e1 - e0);
                for (int e = e0; e < e1; e++) PLAN_REQUIRE(p.fslots[e] < 2 * kWave * fw, "slot %d outside the workgroup", (int)p.fslots[e]);
                for (int j = 0; j < fb.n_zones; j++) {
                    const int32_t z = p.fzones[fb.first_zone + j];
                    PLAN_REQUIRE(z >= 0 && z < Z && !zone_seen[z] && p.zone_block[z] >= 0, "fused zone %d", z);
                    zone_seen[z] = 1;
                    // a fused zone's contributions all come from inside the workgroup
                    PLAN_REQUIRE(p.fzone_eoff[fb.first_zone + j + 1] - p.fzone_eoff[fb.first_zone + j] == p.zone_off[z + 1] - p.zone_off[z],
                                 "zone %d: %d sides in the workgroup, %lld in the model", z,
                                 p.fzone_eoff[fb.first_zone + j + 1] - p.fzone_eoff[fb.first_zone + j], (long long)(p.zone_off[z + 1] - p.zone_off[z]));
                }
                for (int q = 0; q < fb.n_tiles; q++) {
                    const FastTile &ft = p.fast_tiles[c][fb.first_tile + q];
                    if (!single_lane_class(c) || (g2 >> 1))
                        for (int g = 0; g < ft.G; g++)
                            PLAN_REQUIRE(p.meta[ft.surf_base + g] > kFastM[c], "fused tile with a single-lane surface (class %d)", c);
                    fused_surfaces += ft.G;
                    for (int g = 0; g < ft.G; g++)
                        for (int side = 0; side < 2; side++) {
                            const int64_t rec = (int64_t)side * S + ft.surf_base + g;
                            const int lz = p.side_lzone[rec];
                            PLAN_REQUIRE(((p.side[rec].kind_n & 3) == KIND_SPACE) == (lz >= 0) && lz < fb.n_zones, "side %lld: local zone %d", (long long)rec, lz);
                            if (lz >= 0) PLAN_REQUIRE(p.fzones[fb.first_zone + lz] == p.side[rec].zone, "side %lld: local zone maps to another zone", (long long)rec);
                        }
                }
                for (int q = 0; q < fb.n_small; q++) fused_surfaces += p.gen_tiles[fb.first_small + q].G;
            }
    // teams (layout.hpp, FusedSuper): members of four wavefronts, a zone's sides spread over the members that list it
    PLAN_REQUIRE(p.team_zinfo.size() == p.fzones.size(), "team zone table size");
    {
        std::vector<int64_t> team_sides(Z, 0);
        for (int c = 0; c < kNumFast; c++) {
            PLAN_REQUIRE(p.team_supers[c].empty() || (kFastPAL[c] && !kFastCAV[c]), "class %d cannot march in teams", c);
            size_t covered = 0;
            for (const FusedSuper &su : p.team_supers[c]) {
                PLAN_REQUIRE(su.n_members >= 2 && su.n_members <= kTeamMax && su.first_block == (int32_t)covered &&
                             su.first_block + su.n_members <= (int32_t)p.team_blocks[c].size(), "class %d: team of %d members at %d", c, su.n_members, su.first_block);
                covered += (size_t)su.n_members;
                std::vector<uint32_t> mask_seen(kTeamZones, 0), mask_told(kTeamZones, 0);
                std::vector<int32_t> slot_zone(kTeamZones, -1);
                for (int m = 0; m < su.n_members; m++) {
                    const FusedBlock &fb = p.team_blocks[c][su.first_block + m];
                    PLAN_REQUIRE(fb.n_tiles >= 1 && fb.n_tiles <= 4 && fb.n_small == 0, "team member of %d + %d wavefronts", fb.n_tiles, fb.n_small);
                    PLAN_REQUIRE(fb.first_tile >= p.n_stream_tiles[c] && fb.first_tile + fb.n_tiles <= (int)p.fast_tiles[c].size(), "team member: tile range");
                    PLAN_REQUIRE(fb.n_zones >= 0 && fb.n_zones <= kFusedMaxZones && fb.first_zone >= 0 &&
                                 fb.first_zone + fb.n_zones <= (int)p.fzones.size(), "team member: zone range");
                    const int e0 = p.fzone_eoff[fb.first_zone], e1 = p.fzone_eoff[fb.first_zone + fb.n_zones];
                    PLAN_REQUIRE(e1 - e0 <= kFusedMaxEntries && e1 <= (int)p.fslots.size(), "team member: %d zone-facing sides", e1 - e0);
                    for (int e = e0; e < e1; e++) PLAN_REQUIRE(p.fslots[e] < 2 * kWave * 4, "slot %d outside the workgroup", (int)p.fslots[e]);
                    for (int j = 0; j < fb.n_zones; j++) {
                        const int32_t z = p.fzones[fb.first_zone + j];
                        const uint32_t info = p.team_zinfo[fb.first_zone + j], slot = info & 0xffffu;
                        PLAN_REQUIRE(z >= 0 && z < Z && p.zone_block[z] >= 0 && slot < (uint32_t)kTeamZones, "team zone %d", z);
                        PLAN_REQUIRE(slot_zone[slot] < 0 || slot_zone[slot] == z, "exchange slot %u names two zones", slot);
                        PLAN_REQUIRE(((info >> 16) >> m) & 1u, "zone %d: member %d lists it but is not among its members", z, m);
                        slot_zone[slot] = z;
                        mask_seen[slot] |= 1u << m;
                        mask_told[slot] = info >> 16;
                        zone_seen[z] = 1;
                        team_sides[z] += p.fzone_eoff[fb.first_zone + j + 1] - p.fzone_eoff[fb.first_zone + j];
                    }
                    for (int q = 0; q < fb.n_tiles; q++) {
                        const FastTile &ft = p.fast_tiles[c][fb.first_tile + q];
                        fused_surfaces += ft.G;
                        for (int g = 0; g < ft.G; g++)
                            for (int side = 0; side < 2; side++) {
                                const int64_t rec = (int64_t)side * S + ft.surf_base + g;
                                const int lz = p.side_lzone[rec];
                                PLAN_REQUIRE(((p.side[rec].kind_n & 3) == KIND_SPACE) == (lz >= 0) && lz < fb.n_zones, "side %lld: local zone %d", (long long)rec, lz);
                                if (lz >= 0) PLAN_REQUIRE(p.fzones[fb.first_zone + lz] == p.side[rec].zone, "side %lld: local zone maps to another zone", (long long)rec);
                            }
                    }
                }
                // every member awaited for a zone really publishes for it, and nobody else does
                for (int q = 0; q < kTeamZones; q++) PLAN_REQUIRE(mask_seen[q] == mask_told[q], "exchange slot %d: members %x listed, %x awaited", q, mask_seen[q], mask_told[q]);
            }
            PLAN_REQUIRE(covered == p.team_blocks[c].size(), "class %d: team members outside any team", c);
        }
        // a zone marched by a team has all its sides inside the team
        for (int64_t z = 0; z < Z; z++)
            if (team_sides[z] > 0) PLAN_REQUIRE(team_sides[z] == p.zone_off[z + 1] - p.zone_off[z], "zone %lld: %lld sides in its team, %lld in the model", (long long)z, (long long)team_sides[z], (long long)(p.zone_off[z + 1] - p.zone_off[z]));
    }
    for (int64_t z = 0; z < Z; z++) PLAN_REQUIRE((p.zone_block[z] >= 0) == (zone_seen[z] != 0), "zone %lld: block table and workgroup lists disagree", (long long)z);
    if (site_of_surface && p.n_sites > 1) {
        // weather sites: the kernels read the record of the site of a tile's first surface for the whole wavefront, and a
        // workgroup or team holds one site — so every tile, workgroup and team must be of one site
        PLAN_REQUIRE((int64_t)p.dev_site.size() == S, "site table size");
        for (int64_t dd = 0; dd < S; dd++)
            PLAN_REQUIRE(p.dev_site[dd] == site_of_surface[p.orig_of[dd]], "device surface %lld: site %d, surface %lld has %d",
                         (long long)dd, p.dev_site[dd], (long long)p.orig_of[dd], site_of_surface[p.orig_of[dd]]);
        auto run_site = [&](int64_t base, int G) -> int32_t {  // the site of surfaces [base, base + G), -1 when they differ
            for (int g = 1; g < G; g++) if (p.dev_site[base + g] != p.dev_site[base]) return -1;
            return G > 0 ? p.dev_site[base] : -2;
        };
        for (int c = 0; c < kNumFast; c++)
            for (size_t t = 0; t < p.fast_tiles[c].size(); t++)
                PLAN_REQUIRE(run_site(p.fast_tiles[c][t].surf_base, p.fast_tiles[c][t].G) >= 0, "class %d tile %zu holds more than one site", c, t);
        for (size_t t = 0; t < p.gen_tiles.size(); t++)
            PLAN_REQUIRE(run_site(p.gen_tiles[t].surf_base, p.gen_tiles[t].G) >= 0, "general tile %zu holds more than one site", t);
        auto block_site = [&](int c, const FusedBlock &fb, int32_t &site) -> bool {
            for (int q = 0; q < fb.n_tiles + fb.n_small; q++) {
                const int32_t ts = q < fb.n_tiles ? p.dev_site[p.fast_tiles[c][fb.first_tile + q].surf_base]
                                                  : p.dev_site[p.gen_tiles[fb.first_small + q - fb.n_tiles].surf_base];
                if (site >= 0 && ts != site) return false;
                site = ts;
            }
            return true;
        };
        for (int c = 0; c < kNumFast; c++) {
            for (int g2 = 0; g2 < 4; g2++)
                for (size_t bi = 0; bi < p.fblocks[c][g2].size(); bi++) {
                    int32_t site = -1;
                    PLAN_REQUIRE(block_site(c, p.fblocks[c][g2][bi], site), "class %d list %d: workgroup %zu holds more than one site", c, g2, bi);
                }
            for (size_t si = 0; si < p.team_supers[c].size(); si++) {
                int32_t site = -1;
                const FusedSuper &su = p.team_supers[c][si];
                for (int m = 0; m < su.n_members; m++)
                    PLAN_REQUIRE(block_site(c, p.team_blocks[c][su.first_block + m], site), "class %d: team %zu holds more than one site", c, si);
            }
        }
    } else {
        PLAN_REQUIRE(p.dev_site.empty() && p.n_sites == 1, "site table of a single-site plan");
    }
    PLAN_REQUIRE(fused_surfaces == p.n_fused_surfaces, "%lld surfaces in workgroups, %lld counted", (long long)fused_surfaces, (long long)p.n_fused_surfaces);
    if (!p.cavref.empty()) {
        PLAN_REQUIRE((int64_t)p.cavref.size() == 4 * S, "cavref size");
        for (int64_t dd = 0; dd < S; dd++)
            for (int r = 0; r < 2; r++) {
                const int node = p.cavref[4 * dd + 2 * r], cav = p.cavref[4 * dd + 2 * r + 1];
                PLAN_REQUIRE((node < 0) == (cav < 0) && node < p.meta[dd] - 1 + (node < 0) && cav < p.n_cav, "cavity reference of device surface %lld", (long long)dd);
            }
    }
    for (int32_t cidx : p.cav_idx) PLAN_REQUIRE(cidx >= -1 && cidx < p.n_cav, "cavity index %d", cidx);
#undef PLAN_REQUIRE
    return HEAT_OK;
}

// ---------------------------------------------------------------------------
// Partition of a model over ranks along its clusters (include/heat_amd.h, heat_partition).
int partition_surfaces(const heat_batch_desc *d, int32_t n_ranks, int32_t *rank_of_surface, int64_t *n_shared_zones,
                       std::string &err) {
    if (!d || !rank_of_surface) return failp(err, HEAT_E_INVALID_ARG, "NULL argument");
    if (n_ranks < 1) return failp(err, HEAT_E_INVALID_ARG, "n_ranks < 1");
    int rc = check_desc(d, err);
    if (rc) return rc;
    const int64_t S = d->n_surfaces, Z = d->n_zones;
    std::vector<int32_t> cs, cz;
    int32_t nc = 0;
    find_clusters(d, cs, cz, nc);
    auto weight = [&](int64_t s) { return 32.0 * (double)(d->node_offset[s + 1] - d->node_offset[s]) + 152.0; };
    std::vector<double> cw(nc, 0.0);
    double total = 0.0;
    for (int64_t s = 0; s < S; s++) {
        const double w = weight(s);
        total += w;
        if (cs[s] >= 0) cw[cs[s]] += w;
    }
    const double target = total / n_ranks;
    // Items in model order: a whole cluster at the place of its first surface (its later surfaces follow it to its
    // rank), or — a cluster heavier than a quarter of a shard, and surfaces that face no zone — single surfaces.
    std::vector<int32_t> crank(nc, -1);
    double cum = 0.0;
    int32_t r = 0;
    auto advance = [&](double w) {
        // the item goes to the rank its midpoint falls into
        const double mid = cum + 0.5 * w;
        while (r + 1 < n_ranks && mid >= (r + 1) * target) r++;
        cum += w;
        return r;
    };
    for (int64_t s = 0; s < S; s++) {
        const int32_t c = cs[s];
        if (c >= 0 && cw[c] <= 0.25 * target) {
            if (crank[c] < 0) crank[c] = advance(cw[c]);
            rank_of_surface[s] = crank[c];
        } else {
            rank_of_surface[s] = advance(weight(s));
        }
    }
    if (n_shared_zones) {
        std::vector<int32_t> first(Z, -1);
        std::vector<uint8_t> shared(Z, 0);
        auto touch = [&](int32_t z, int32_t rk) {
            if (first[z] < 0) first[z] = rk;
            else if (first[z] != rk) shared[z] = 1;
        };
        for (int64_t s = 0; s < S; s++) {
            if (d->front_kind[s] == HEAT_BOUNDARY_SPACE) touch(d->front_zone[s], rank_of_surface[s]);
            if (d->back_kind[s] == HEAT_BOUNDARY_SPACE) touch(d->back_zone[s], rank_of_surface[s]);
        }
        int64_t n = 0;
        for (int64_t z = 0; z < Z; z++) n += shared[z];
        *n_shared_zones = n;
    }
    return HEAT_OK;
}

// The descriptor of one rank's surfaces (zones, cavities and state slots stay global).
void ShardDesc::build(const heat_batch_desc *d, const int32_t *rank_of_surface, int32_t rank) {
    const int64_t S = d->n_surfaces;
    std::vector<int64_t> idx;
    for (int64_t s = 0; s < S; s++)
        if (rank_of_surface[s] == rank) idx.push_back(s);
    const int64_t n = (int64_t)idx.size();
    node_offset.assign(n + 1, 0);
    for (int64_t q = 0; q < n; q++) node_offset[q + 1] = node_offset[q] + (d->node_offset[idx[q] + 1] - d->node_offset[idx[q]]);
    const int64_t N = node_offset[n];
    auto take_nodes = [&](const double *src, std::vector<double> &dst) {
        dst.resize(N);
        for (int64_t q = 0; q < n; q++)
            std::copy(src + d->node_offset[idx[q]], src + d->node_offset[idx[q] + 1], dst.begin() + node_offset[q]);
    };
    take_nodes(d->mass, mass);
    take_nodes(d->uvalue, uvalue);
    take_nodes(d->front_alpha, front_alpha);
    take_nodes(d->back_alpha, back_alpha);
    if (d->seg_cavity) {
        seg_cavity.resize(N);
        for (int64_t q = 0; q < n; q++)
            std::copy(d->seg_cavity + d->node_offset[idx[q]], d->seg_cavity + d->node_offset[idx[q] + 1], seg_cavity.begin() + node_offset[q]);
    }
    const double *fsrc[] = {d->front_ambient, d->back_ambient, d->front_emissivity, d->back_emissivity, d->area, d->perimeter,
                            d->cos_tilt, d->normal_x, d->normal_y, d->wind_modifier, d->front_hs_fix, d->back_hs_fix};
    for (int a = 0; a < 12; a++) {
        f64[a].clear();
        if (!fsrc[a]) continue;
        f64[a].resize(n);
        for (int64_t q = 0; q < n; q++) f64[a][q] = fsrc[a][idx[q]];
    }
    const int32_t *isrc[] = {d->front_kind, d->back_kind, d->front_zone, d->back_zone};
    for (int a = 0; a < 4; a++) {
        i32[a].resize(n);
        for (int64_t q = 0; q < n; q++) i32[a][q] = isrc[a][idx[q]];
    }
    const int64_t *ssrc[] = {d->first_node_slot, d->hs_front_slot, d->hs_back_slot, d->flow_front_slot, d->flow_back_slot,
                             d->solar_front_slot, d->solar_back_slot, d->ir_front_slot, d->ir_back_slot};
    for (int a = 0; a < 9; a++) {
        i64[a].resize(n);
        for (int64_t q = 0; q < n; q++) i64[a][q] = ssrc[a][idx[q]];
    }
    desc = *d;
    desc.n_surfaces = n;
    desc.node_offset = node_offset.data();
    desc.mass = mass.data();
    desc.uvalue = uvalue.data();
    desc.front_alpha = front_alpha.data();
    desc.back_alpha = back_alpha.data();
    desc.seg_cavity = d->seg_cavity ? seg_cavity.data() : nullptr;
    const double **fdst[] = {&desc.front_ambient, &desc.back_ambient, &desc.front_emissivity, &desc.back_emissivity, &desc.area,
                             &desc.perimeter, &desc.cos_tilt, &desc.normal_x, &desc.normal_y, &desc.wind_modifier,
                             &desc.front_hs_fix, &desc.back_hs_fix};
    for (int a = 0; a < 12; a++) *fdst[a] = fsrc[a] ? f64[a].data() : nullptr;
    const int32_t **idst[] = {&desc.front_kind, &desc.back_kind, &desc.front_zone, &desc.back_zone};
    for (int a = 0; a < 4; a++) *idst[a] = i32[a].data();
    const int64_t **sdst[] = {&desc.first_node_slot, &desc.hs_front_slot, &desc.hs_back_slot, &desc.flow_front_slot,
                              &desc.flow_back_slot, &desc.solar_front_slot, &desc.solar_back_slot, &desc.ir_front_slot,
                              &desc.ir_back_slot};
    for (int a = 0; a < 9; a++) *sdst[a] = i64[a].data();
    original_index = std::move(idx);
}

// ---- series march: the host-only half (include/heat_amd.h, heat_series) ----
bool SlotResolver::resolve(int64_t slot, int &kind, int64_t &index, int &node) {
    auto find = [&](const std::vector<std::pair<int64_t, int64_t>> &v, int64_t &what) {
        auto it = std::lower_bound(v.begin(), v.end(), std::make_pair(slot, (int64_t)INT64_MIN));
        if (it == v.end() || it->first != slot) return false;
        what = it->second;
        return true;
    };
    node = 0;
    if (!zones_built_) {
        zones_.reserve((size_t)m_.n_zones);
        for (int64_t z = 0; z < m_.n_zones; z++) zones_.push_back({m_.zone_slot[z], z});
        std::sort(zones_.begin(), zones_.end());
        zones_built_ = true;
    }
    if (find(zones_, index)) {
        kind = PROBE_ZONE;
        return true;
    }
    if (!nodes_built_) {
        nodes_.reserve((size_t)m_.n_surfaces);
        for (int64_t s = 0; s < m_.n_surfaces; s++) nodes_.push_back({m_.first_node_slot[s], s});
        std::sort(nodes_.begin(), nodes_.end());
        nodes_built_ = true;
    }
    {   // the surface whose node slots start at or before `slot` (node slots of a surface are contiguous)
        auto it = std::upper_bound(nodes_.begin(), nodes_.end(), std::make_pair(slot, (int64_t)INT64_MAX));
        if (it != nodes_.begin()) {
            --it;
            if (slot - it->first < m_.node_count[it->second]) {
                kind = PROBE_NODE;
                index = it->second;
                node = (int)(slot - it->first);
                return true;
            }
        }
    }
    if (!scalars_built_) {
        scalars_.reserve(4 * (size_t)m_.n_surfaces);
        for (int a = 0; a < 4; a++)
            for (int64_t s = 0; s < m_.n_surfaces; s++) scalars_.push_back({m_.out_slot[a][s], 4 * s + a});
        std::sort(scalars_.begin(), scalars_.end());
        scalars_built_ = true;
    }
    int64_t code = 0;
    if (!find(scalars_, code)) return false;
    kind = PROBE_HS_FRONT + (int)(code & 3);
    index = code >> 2;
    return true;
}

int check_series(const SeriesModel &m, SlotResolver &res, int32_t n_sites, const heat_series *s, std::string &err) {
    if (!s) return failp(err, HEAT_E_INVALID_ARG, "series is NULL");
    if (s->n_steps < 0 || s->n_sub < 0 || s->n_channels < 0 || s->n_probes < 0 || s->n_zone_term_steps < 0)
        return failp(err, HEAT_E_INVALID_ARG, "negative count in series (n_steps %d, n_sub %d, n_channels %d, n_probes %lld, n_zone_term_steps %d)",
                     s->n_steps, s->n_sub, s->n_channels, (long long)s->n_probes, s->n_zone_term_steps);
    if (n_sites < 1 || n_sites > kMaxSites) return failp(err, HEAT_E_INVALID_ARG, "n_sites = %d outside [1, %d]", n_sites, kMaxSites);
    if (s->n_zone_term_steps != 0 && s->n_zone_term_steps != 1 && s->n_zone_term_steps != s->n_steps)
        return failp(err, HEAT_E_INVALID_ARG, "n_zone_term_steps = %d: must be 0, 1 or n_steps (%d)", s->n_zone_term_steps, s->n_steps);
    // (the limit of heat_batch_set_weather, per step)
    constexpr int64_t kMaxWeatherRecords = (int64_t)1 << 24;
    if (n_sites > 1 && (int64_t)s->n_sub * n_sites > kMaxWeatherRecords)
        return failp(err, HEAT_E_INVALID_ARG, "n_sub %d x %d sites = %lld weather records, more than %lld per step", s->n_sub, n_sites,
                     (long long)s->n_sub * n_sites, (long long)kMaxWeatherRecords);
    if (!s->weather && (int64_t)s->n_steps * s->n_sub > 0) return failp(err, HEAT_E_INVALID_ARG, "series weather is NULL");
    if (!s->channel && (int64_t)s->n_steps * s->n_channels > 0) return failp(err, HEAT_E_INVALID_ARG, "series channel table is NULL");
    if (!s->probe_slot && s->n_probes > 0) return failp(err, HEAT_E_INVALID_ARG, "probe_slot is NULL");
    const int32_t *chan[4] = {s->solar_front_chan, s->solar_back_chan, s->ir_front_chan, s->ir_back_chan};
    static const char *const input_name[4] = {"solar front", "solar back", "long-wave front", "long-wave back"};
    for (int a = 0; a < 4; a++) {
        if (!chan[a]) continue;
        for (int64_t q = 0; q < m.n_surfaces; q++)
            if (chan[a][q] < -1 || chan[a][q] >= s->n_channels)
                return failp(err, HEAT_E_SIZE, "surface %lld: %s channel %d outside [-1, %d)", (long long)q, input_name[a], chan[a][q], s->n_channels);
    }
    if (s->ir_own_face)
        for (int64_t q = 0; q < m.n_surfaces; q++)
            for (int side = 0; side < 2; side++)
                if ((s->ir_own_face[q] >> side & 1) && (!chan[2 + side] || chan[2 + side][q] < 0))
                    return failp(err, HEAT_E_SIZE, "surface %lld: own-face term on its %s side, whose long-wave input is not driven (channel -1)",
                                 (long long)q, side ? "back" : "front");
    for (int64_t q = 0; q < s->n_probes; q++) {
        int kind, node;
        int64_t index;
        if (!res.resolve(s->probe_slot[q], kind, index, node))
            return failp(err, HEAT_E_SIZE, "probe %lld: slot %lld is not a node-temperature, hs, flow or zone slot of the descriptor", (long long)q,
                         (long long)s->probe_slot[q]);
    }
    return HEAT_OK;
}

// ---- zone loads of a series (include/heat_amd.h, heat_zone_loads) ----
int check_zone_loads(int64_t n_zones, int32_t n_channels, const heat_zone_loads *l, std::string &err) {
    if (!l) return HEAT_OK;
    if (l->n_gains < 0 || l->n_flows < 0 || l->n_thermostats < 0)
        return failp(err, HEAT_E_INVALID_ARG, "negative count in zone loads (n_gains %lld, n_flows %lld, n_thermostats %lld)",
                     (long long)l->n_gains, (long long)l->n_flows, (long long)l->n_thermostats);
    // (the tables number their terms with 32 bits)
    if (l->n_gains > INT32_MAX || l->n_flows > INT32_MAX || l->n_thermostats > INT32_MAX)
        return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 terms in zone loads (n_gains %lld, n_flows %lld, n_thermostats %lld)",
                     (long long)l->n_gains, (long long)l->n_flows, (long long)l->n_thermostats);
    if (l->n_gains > 0 && (!l->gain_zone || !l->gain_chan)) return failp(err, HEAT_E_INVALID_ARG, "gain_zone or gain_chan is NULL");
    if (l->n_flows > 0 && (!l->flow_zone || !l->flow_volume_chan || !l->flow_temp_chan))
        return failp(err, HEAT_E_INVALID_ARG, "flow_zone, flow_volume_chan or flow_temp_chan is NULL");
    if (l->n_thermostats > 0 && (!l->th_sensor_zone || !l->th_target_zone || !l->th_heat_chan || !l->th_cool_chan ||
                                 !l->th_heat_power || !l->th_cool_power || !l->th_band))
        return failp(err, HEAT_E_INVALID_ARG, "a thermostat array is NULL (only th_mode may be)");
    auto zone_ok = [&](int32_t z) { return z >= 0 && z < n_zones; };
    auto chan_ok = [&](int32_t c) { return c >= 0 && c < n_channels; };
    for (int64_t i = 0; i < l->n_gains; i++) {
        if (!zone_ok(l->gain_zone[i]))
            return failp(err, HEAT_E_SIZE, "gain %lld: zone %d outside [0, %lld)", (long long)i, l->gain_zone[i], (long long)n_zones);
        if (!chan_ok(l->gain_chan[i]))
            return failp(err, HEAT_E_SIZE, "gain %lld: channel %d outside [0, %d)", (long long)i, l->gain_chan[i], n_channels);
    }
    for (int64_t i = 0; i < l->n_flows; i++) {
        if (!zone_ok(l->flow_zone[i]))
            return failp(err, HEAT_E_SIZE, "flow %lld: zone %d outside [0, %lld)", (long long)i, l->flow_zone[i], (long long)n_zones);
        if (!chan_ok(l->flow_volume_chan[i]))
            return failp(err, HEAT_E_SIZE, "flow %lld: volume channel %d outside [0, %d)", (long long)i, l->flow_volume_chan[i], n_channels);
        if (!chan_ok(l->flow_temp_chan[i]))
            return failp(err, HEAT_E_SIZE, "flow %lld: temperature channel %d outside [0, %d)", (long long)i, l->flow_temp_chan[i], n_channels);
    }
    for (int64_t i = 0; i < l->n_thermostats; i++) {
        if (!zone_ok(l->th_sensor_zone[i]))
            return failp(err, HEAT_E_SIZE, "thermostat %lld: sensor zone %d outside [0, %lld)", (long long)i, l->th_sensor_zone[i], (long long)n_zones);
        if (!zone_ok(l->th_target_zone[i]))
            return failp(err, HEAT_E_SIZE, "thermostat %lld: target zone %d outside [0, %lld)", (long long)i, l->th_target_zone[i], (long long)n_zones);
        const int32_t hc = l->th_heat_chan[i], cc = l->th_cool_chan[i];
        if (hc != -1 && !chan_ok(hc))
            return failp(err, HEAT_E_SIZE, "thermostat %lld: heating setpoint channel %d outside [-1, %d)", (long long)i, hc, n_channels);
        if (cc != -1 && !chan_ok(cc))
            return failp(err, HEAT_E_SIZE, "thermostat %lld: cooling setpoint channel %d outside [-1, %d)", (long long)i, cc, n_channels);
        if (hc == -1 && cc == -1)
            return failp(err, HEAT_E_SIZE, "thermostat %lld: neither a heating nor a cooling setpoint channel", (long long)i);
        const double v[3] = {l->th_heat_power[i], l->th_cool_power[i], l->th_band[i]};
        static const char *const name[3] = {"heating power", "cooling power", "band"};
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(v[a]) || v[a] < 0.0)
                return failp(err, HEAT_E_INVALID_ARG, "thermostat %lld: %s %g is negative or not finite", (long long)i, name[a], v[a]);
        if (l->th_mode && l->th_mode[i] > 2)
            return failp(err, HEAT_E_INVALID_ARG, "thermostat %lld: mode %d is none of 0 (off), 1 (heating), 2 (cooling)", (long long)i,
                         (int)l->th_mode[i]);
    }
    return HEAT_OK;
}

void build_zone_load_tables(int64_t n_zones, const heat_zone_loads *l, ZoneLoadTables &t) {
    const size_t Z = (size_t)n_zones;
    t = ZoneLoadTables();
    t.off.assign(3 * (Z + 1), 0);
    if (!l) return;
    // a counting sort by zone: stable, so the caller's order survives inside a zone. place[i] = where term i goes.
    auto csr = [&](int64_t n, const int32_t *zone, int32_t *off, std::vector<int32_t> &place) {
        place.resize((size_t)n);
        for (int64_t i = 0; i < n; i++) off[zone[i] + 1]++;
        for (size_t z = 0; z < Z; z++) off[z + 1] += off[z];
        std::vector<int32_t> next(off, off + Z);
        for (int64_t i = 0; i < n; i++) place[(size_t)i] = next[(size_t)zone[i]]++;
    };
    std::vector<int32_t> place;
    csr(l->n_gains, l->gain_zone, t.off.data(), place);
    t.gain_chan.resize(place.size());
    t.gain_factor.resize(place.size());
    for (size_t i = 0; i < place.size(); i++) {
        t.gain_chan[(size_t)place[i]] = l->gain_chan[i];
        t.gain_factor[(size_t)place[i]] = l->gain_factor ? l->gain_factor[i] : 1.0;
    }
    csr(l->n_flows, l->flow_zone, t.off.data() + (Z + 1), place);
    t.flow_volume_chan.resize(place.size());
    t.flow_temp_chan.resize(place.size());
    t.flow_volume_gain.resize(place.size());
    for (size_t i = 0; i < place.size(); i++) {
        t.flow_volume_chan[(size_t)place[i]] = l->flow_volume_chan[i];
        t.flow_temp_chan[(size_t)place[i]] = l->flow_temp_chan[i];
        t.flow_volume_gain[(size_t)place[i]] = l->flow_volume_gain ? l->flow_volume_gain[i] : 1.0;
    }
    csr(l->n_thermostats, l->th_target_zone, t.off.data() + 2 * (Z + 1), place);
    const size_t n = place.size();
    t.th_sensor.resize(n);
    t.th_heat_chan.resize(n);
    t.th_cool_chan.resize(n);
    t.th_orig.resize(n);
    t.th_heat_power.resize(n);
    t.th_cool_power.resize(n);
    t.th_half_band.resize(n);
    for (size_t i = 0; i < n; i++) {
        const size_t p = (size_t)place[i];
        t.th_sensor[p] = l->th_sensor_zone[i];
        t.th_heat_chan[p] = l->th_heat_chan[i];
        t.th_cool_chan[p] = l->th_cool_chan[i];
        t.th_orig[p] = (int32_t)i;
        t.th_heat_power[p] = l->th_heat_power[i];
        t.th_cool_power[p] = l->th_cool_power[i];
        t.th_half_band[p] = l->th_band[i] / 2.0;
    }
}

// ---- air paths of a series (include/heat_amd.h, heat_air_paths) ----
int check_air_paths(int64_t n_zones, int32_t n_channels, const heat_air_paths *air, std::string &err) {
    if (!air) return HEAT_OK;
    const int64_t n = air->n_paths;
    if (n < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count of air paths (air path count n_paths %lld)", (long long)n);
    // (the tables number the paths with 32 bits)
    if (n > INT32_MAX) return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 air paths (air path count n_paths %lld)", (long long)n);
    if (n == 0) return HEAT_OK;
    if (!air->target) return failp(err, HEAT_E_INVALID_ARG, "air path 0: target is NULL");
    if (!air->source) return failp(err, HEAT_E_INVALID_ARG, "air path 0: source is NULL");
    if (!air->volume_chan) return failp(err, HEAT_E_INVALID_ARG, "air path 0: volume_chan is NULL");
    for (int64_t i = 0; i < n; i++) {
        const int32_t zt = air->target[i], zs = air->source[i], vc = air->volume_chan[i];
        const int32_t tc = air->temp_chan ? air->temp_chan[i] : -1, oc = air->open_chan ? air->open_chan[i] : -1;
        if (zt < 0 || zt >= n_zones)
            return failp(err, HEAT_E_SIZE, "air path %lld: target zone %d outside [0, %lld)", (long long)i, zt, (long long)n_zones);
        if (zs < -1 || zs >= n_zones)
            return failp(err, HEAT_E_SIZE, "air path %lld: source zone %d outside [-1, %lld)", (long long)i, zs, (long long)n_zones);
        if (zs == zt) return failp(err, HEAT_E_INVALID_ARG, "air path %lld: source and target are the same zone %d", (long long)i, zt);
        if (vc < 0 || vc >= n_channels)
            return failp(err, HEAT_E_SIZE, "air path %lld: volume channel %d outside [0, %d)", (long long)i, vc, n_channels);
        if (zs == -1 && (tc < 0 || tc >= n_channels))
            return failp(err, HEAT_E_SIZE, "air path %lld: source -1 (supply air) needs a temperature channel in [0, %d), not %d%s", (long long)i,
                         n_channels, tc, air->temp_chan ? "" : " (temp_chan is NULL)");
        if (zs >= 0 && tc != -1)
            return failp(err, HEAT_E_SIZE, "air path %lld: its air comes from zone %d and from temperature channel %d: an input has one source",
                         (long long)i, zs, tc);
        if (oc < -1 || oc >= n_channels)
            return failp(err, HEAT_E_SIZE, "air path %lld: open channel %d outside [-1, %d)", (long long)i, oc, n_channels);
        if (air->volume_gain && !std::isfinite(air->volume_gain[i]))
            return failp(err, HEAT_E_INVALID_ARG, "air path %lld: volume_gain %g is not finite", (long long)i, air->volume_gain[i]);
        if (air->state && air->state[i] > 1)
            return failp(err, HEAT_E_INVALID_ARG, "air path %lld: state %d is neither 0 (closed) nor 1 (open)", (long long)i, (int)air->state[i]);
        if (oc < 0) continue;  // (uncontrolled: sense, band and min_delta are not read)
        if (!air->sense || !air->band || !air->min_delta)
            return failp(err, HEAT_E_INVALID_ARG, "air path %lld: controlled (open channel %d), but %s is NULL", (long long)i, oc,
                         !air->sense ? "sense" : (!air->band ? "band" : "min_delta"));
        if (air->sense[i] != 1 && air->sense[i] != -1)
            return failp(err, HEAT_E_INVALID_ARG, "air path %lld: sense %d is neither +1 (cooling) nor -1 (heating)", (long long)i, (int)air->sense[i]);
        const double v[2] = {air->band[i], air->min_delta[i]};
        static const char *const name[2] = {"band", "min_delta"};
        for (int a = 0; a < 2; a++)
            if (!std::isfinite(v[a]) || v[a] < 0.0)
                return failp(err, HEAT_E_INVALID_ARG, "air path %lld: %s %g is negative or not finite", (long long)i, name[a], v[a]);
    }
    return HEAT_OK;
}

void build_air_path_tables(int64_t n_zones, const heat_air_paths *air, AirPathTables &t) {
    const size_t Z = (size_t)n_zones, n = air ? (size_t)air->n_paths : 0;
    t = AirPathTables();
    t.n_zones = n_zones;
    t.n_paths = (int64_t)n;
    t.i32.assign(Z + 1 + 5 * n, 0);
    t.f64.assign(4 * n, 0.0);
    if (n == 0) return;
    // a counting sort by target zone: stable, so the caller's order survives inside a zone
    int32_t *off = t.i32.data();
    for (size_t i = 0; i < n; i++) off[air->target[i] + 1]++;
    for (size_t z = 0; z < Z; z++) off[z + 1] += off[z];
    std::vector<int32_t> next(off, off + Z);
    int32_t *list = t.i32.data() + Z + 1;
    double *real = t.f64.data();
    for (size_t i = 0; i < n; i++) {
        const size_t p = (size_t)next[(size_t)air->target[i]]++;
        const int32_t oc = air->open_chan ? air->open_chan[i] : -1;
        list[p] = air->source[i];
        list[n + p] = air->temp_chan ? air->temp_chan[i] : -1;
        list[2 * n + p] = air->volume_chan[i];
        list[3 * n + p] = oc;
        list[4 * n + p] = (int32_t)i;
        real[p] = air->volume_gain ? air->volume_gain[i] : 1.0;
        real[n + p] = oc >= 0 ? (double)air->sense[i] : 0.0;
        real[2 * n + p] = oc >= 0 ? air->band[i] / 2.0 : 0.0;
        real[3 * n + p] = oc >= 0 ? air->min_delta[i] : 0.0;
    }
}

int check_air_path_tables(int64_t n_zones, const heat_air_paths *air, const AirPathTables &t, std::string &err) {
    const size_t Z = (size_t)n_zones, n = air ? (size_t)air->n_paths : 0;
    if (t.n_zones != n_zones || t.n_paths != (int64_t)n || t.i32.size() != Z + 1 + 5 * n || t.f64.size() != 4 * n)
        return failp(err, HEAT_E_SIZE, "air path tables: %zu integers and %zu reals for %zu paths into %zu zones", t.i32.size(), t.f64.size(), n, Z);
    const int32_t *off = t.off();
    if (off[0] != 0 || off[Z] != (int32_t)n)
        return failp(err, HEAT_E_SIZE, "air path tables: the offsets run from %d to %d for %zu paths", off[0], off[Z], n);
    for (size_t z = 0; z < Z; z++)
        if (off[z + 1] < off[z] || off[z + 1] > (int32_t)n)
            return failp(err, HEAT_E_SIZE, "air path tables: zone %zu runs from %d to %d", z, off[z], off[z + 1]);
    // every path of the caller's, in the caller's order, is the next element of its target's range ...
    std::vector<int32_t> cursor(off, off + Z);
    for (size_t i = 0; i < n; i++) {
        const size_t z = (size_t)air->target[i];
        const int32_t p = cursor[z]++;
        if (p >= off[z + 1]) return failp(err, HEAT_E_SIZE, "air path tables: air path %zu: zone %zu has no room for it", i, z);
        const int32_t oc = air->open_chan ? air->open_chan[i] : -1;
        const double gain = air->volume_gain ? air->volume_gain[i] : 1.0;
        if (t.list(4)[p] != (int32_t)i || t.list(0)[p] != air->source[i] || t.list(1)[p] != (air->temp_chan ? air->temp_chan[i] : -1) ||
            t.list(2)[p] != air->volume_chan[i] || t.list(3)[p] != oc || std::memcmp(&t.real(0)[p], &gain, sizeof(double)) != 0)
            return failp(err, HEAT_E_SIZE, "air path tables: air path %zu is not element %d of zone %zu", i, p - off[z], z);
        if (oc >= 0 && (t.real(1)[p] != (double)air->sense[i] || t.real(2)[p] != air->band[i] / 2.0 || t.real(3)[p] != air->min_delta[i]))
            return failp(err, HEAT_E_SIZE, "air path tables: air path %zu: its controller is not the caller's", i);
    }
    // ... and every range is full: with n elements in all, each path is present exactly once
    for (size_t z = 0; z < Z; z++)
        if (cursor[z] != off[z + 1]) return failp(err, HEAT_E_SIZE, "air path tables: zone %zu holds %d paths of %d", z, cursor[z] - off[z], off[z + 1] - off[z]);
    return HEAT_OK;
}

// ---- air handlers of a series (include/heat_amd.h, heat_air_handlers) ----
int check_air_handlers(int64_t n_zones, int32_t n_channels, const heat_air_handlers *h, std::string &err) {
    if (!h) return HEAT_OK;
    const int64_t U = h->n_units, B = h->n_branches;
    const int NC = n_channels;
    if (U < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count of air handlers (n_units %lld): no air handler u", (long long)U);
    if (B < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count of air handler branches (n_branches %lld): no air handler branch j", (long long)B);
    // (the tables number units and branches with 32 bits)
    if (U > INT32_MAX || B > INT32_MAX)
        return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 air handlers u or air handler branches j (n_units %lld, n_branches %lld)",
                     (long long)U, (long long)B);
    if (U == 0 && B > 0)
        return failp(err, HEAT_E_INVALID_ARG, "air handler branch 0: %lld branches, but no air handler u (n_units 0)", (long long)B);
    if (U == 0) return HEAT_OK;
    if (!h->outdoor_chan) return failp(err, HEAT_E_INVALID_ARG, "air handler 0: outdoor_chan is NULL (n_units %lld)", (long long)U);
    for (int64_t u = 0; u < U; u++) {
        const int32_t oc = h->outdoor_chan[u];
        if (oc < 0 || oc >= NC) return failp(err, HEAT_E_SIZE, "air handler %lld: outdoor channel %d outside [0, %d)", (long long)u, oc, NC);
        const int32_t *const opt[4] = {h->eff_chan, h->bypass_chan, h->heat_chan, h->cool_chan};
        static const char *const opt_name[4] = {"effectiveness", "bypass", "heating", "cooling"};
        for (int a = 0; a < 4; a++) {
            const int32_t ch = opt[a] ? opt[a][u] : -1;
            if (ch < -1 || ch >= NC)
                return failp(err, HEAT_E_SIZE, "air handler %lld: %s channel %d outside [-1, %d)", (long long)u, opt_name[a], ch, NC);
        }
        if (h->eff_gain && !std::isfinite(h->eff_gain[u]))
            return failp(err, HEAT_E_INVALID_ARG, "air handler %lld: eff_gain %g is not finite", (long long)u, h->eff_gain[u]);
        const double *const cap[2] = {h->heat_cap, h->cool_cap};
        static const char *const cap_name[2] = {"heat_cap", "cool_cap"};
        for (int a = 0; a < 2; a++)
            if (cap[a] && !(cap[a][u] >= 0.0))
                return failp(err, HEAT_E_INVALID_ARG, "air handler %lld: %s %g is negative or NaN", (long long)u, cap_name[a], cap[a][u]);
        if (h->bypass && h->bypass[u] > 1)
            return failp(err, HEAT_E_INVALID_ARG, "air handler %lld: bypass %d is neither 0 (recovering) nor 1 (bypassed)", (long long)u, (int)h->bypass[u]);
        if (!h->bypass_chan || h->bypass_chan[u] < 0) continue;  // (no bypass: band and min_delta are not read)
        if (!h->bypass_band || !h->bypass_min_delta)
            return failp(err, HEAT_E_INVALID_ARG, "air handler %lld: it bypasses (bypass channel %d), but %s is NULL", (long long)u, h->bypass_chan[u],
                         !h->bypass_band ? "bypass_band" : "bypass_min_delta");
        const double v[2] = {h->bypass_band[u], h->bypass_min_delta[u]};
        static const char *const name[2] = {"bypass_band", "bypass_min_delta"};
        for (int a = 0; a < 2; a++)
            if (!std::isfinite(v[a]) || v[a] < 0.0)
                return failp(err, HEAT_E_INVALID_ARG, "air handler %lld: %s %g is negative or not finite", (long long)u, name[a], v[a]);
    }
    if (B == 0) return HEAT_OK;
    if (!h->br_unit || !h->br_zone || !h->br_volume_chan)
        return failp(err, HEAT_E_INVALID_ARG, "air handler branch 0: %s is NULL (n_branches %lld)",
                     !h->br_unit ? "br_unit" : (!h->br_zone ? "br_zone" : "br_volume_chan"), (long long)B);
    for (int64_t j = 0; j < B; j++) {
        const int32_t u = h->br_unit[j], z = h->br_zone[j], vc = h->br_volume_chan[j];
        if (u < 0 || u >= U) return failp(err, HEAT_E_SIZE, "air handler branch %lld: unit %d outside [0, %lld)", (long long)j, u, (long long)U);
        if (z < 0 || z >= n_zones) return failp(err, HEAT_E_SIZE, "air handler branch %lld: zone %d outside [0, %lld)", (long long)j, z, (long long)n_zones);
        if (vc < 0 || vc >= NC) return failp(err, HEAT_E_SIZE, "air handler branch %lld: volume channel %d outside [0, %d)", (long long)j, vc, NC);
        if (h->br_volume_gain && !std::isfinite(h->br_volume_gain[j]))
            return failp(err, HEAT_E_INVALID_ARG, "air handler branch %lld: br_volume_gain %g is not finite", (long long)j, h->br_volume_gain[j]);
        if (h->br_kind && (h->br_kind[j] < 1 || h->br_kind[j] > 3))
            return failp(err, HEAT_E_INVALID_ARG, "air handler branch %lld: br_kind %d is none of 1 (supplies), 2 (extracts), 3 (both)", (long long)j,
                         (int)h->br_kind[j]);
    }
    return HEAT_OK;
}

void build_air_handler_tables(int64_t n_zones, const heat_air_handlers *h, HandlerTables &t) {
    t = HandlerTables();
    const size_t U = h ? (size_t)h->n_units : 0, B = h ? (size_t)h->n_branches : 0, Z = (size_t)n_zones;
    if (U == 0) return;
    const double inf = std::numeric_limits<double>::infinity();
    t.i32.assign(kHandlerI32Rows * U, -1);
    t.f64.assign(kHandlerF64Rows * U, 0.0);
    for (size_t u = 0; u < U; u++) {
        const int32_t bc = h->bypass_chan ? h->bypass_chan[u] : -1;
        t.i32[AH_OUTDOOR_CHAN * U + u] = h->outdoor_chan[u];
        t.i32[AH_EFF_CHAN * U + u] = h->eff_chan ? h->eff_chan[u] : -1;
        t.i32[AH_BYPASS_CHAN * U + u] = bc;
        t.i32[AH_HEAT_CHAN * U + u] = h->heat_chan ? h->heat_chan[u] : -1;
        t.i32[AH_COOL_CHAN * U + u] = h->cool_chan ? h->cool_chan[u] : -1;
        t.f64[AH_EFF_GAIN * U + u] = h->eff_gain ? h->eff_gain[u] : 1.0;
        t.f64[AH_HALF_BAND * U + u] = bc >= 0 ? h->bypass_band[u] / 2.0 : 0.0;
        t.f64[AH_MIN_DELTA * U + u] = bc >= 0 ? h->bypass_min_delta[u] : 0.0;
        t.f64[AH_HEAT_CAP * U + u] = h->heat_cap ? h->heat_cap[u] : inf;
        t.f64[AH_COOL_CAP * U + u] = h->cool_cap ? h->cool_cap[u] : inf;
    }
    // two counting sorts, stable: the caller's order survives inside a unit and inside a zone
    t.unit_off.assign(U + 1, 0);
    t.zone_off.assign(Z + 1, 0);
    size_t n_supply = 0;
    for (size_t j = 0; j < B; j++) {
        const unsigned kind = h->br_kind ? h->br_kind[j] : 3u;
        t.unit_off[(size_t)h->br_unit[j] + 1]++;
        if (kind & 1u) t.zone_off[(size_t)h->br_zone[j] + 1]++, n_supply++;
    }
    for (size_t u = 0; u < U; u++) t.unit_off[u + 1] += t.unit_off[u];
    for (size_t z = 0; z < Z; z++) t.zone_off[z + 1] += t.zone_off[z];
    t.u_zone.resize(B), t.u_chan.resize(B), t.u_orig.resize(B), t.u_kind.resize(B), t.u_gain.resize(B);
    t.z_unit.resize(n_supply), t.z_orig.resize(n_supply);
    std::vector<int32_t> next_u(t.unit_off.begin(), t.unit_off.end() - 1), next_z(t.zone_off.begin(), t.zone_off.end() - 1);
    for (size_t j = 0; j < B; j++) {
        const unsigned kind = h->br_kind ? h->br_kind[j] : 3u;
        const size_t p = (size_t)next_u[(size_t)h->br_unit[j]]++;
        t.u_zone[p] = h->br_zone[j];
        t.u_chan[p] = h->br_volume_chan[j];
        t.u_orig[p] = (int32_t)j;
        t.u_kind[p] = (uint8_t)kind;
        t.u_gain[p] = h->br_volume_gain ? h->br_volume_gain[j] : 1.0;
        if (!(kind & 1u)) continue;
        const size_t q = (size_t)next_z[(size_t)h->br_zone[j]]++;
        t.z_unit[q] = h->br_unit[j];
        t.z_orig[q] = (int32_t)j;
    }
}

int check_air_handler_tables(int64_t n_zones, const heat_air_handlers *h, const HandlerTables &t, std::string &err) {
    const size_t U = h ? (size_t)h->n_units : 0, B = h ? (size_t)h->n_branches : 0, Z = (size_t)n_zones;
    if (U == 0) return HEAT_OK;
    const size_t NS = t.z_unit.size();
    if (t.unit_off.size() != U + 1 || t.zone_off.size() != Z + 1 || t.u_zone.size() != B || t.u_chan.size() != B || t.u_orig.size() != B ||
        t.u_kind.size() != B || t.u_gain.size() != B || t.z_orig.size() != NS || NS > B || t.i32.size() != kHandlerI32Rows * U ||
        t.f64.size() != kHandlerF64Rows * U)
        return failp(err, HEAT_E_SIZE, "air handler tables: %zu unit offsets, %zu zone offsets, %zu and %zu elements for air handler u < %zu, air handler branch j < %zu",
                     t.unit_off.size(), t.zone_off.size(), t.u_zone.size(), NS, U, B);
    if (t.unit_off[0] != 0 || t.unit_off[U] != (int32_t)B || t.zone_off[0] != 0 || t.zone_off[Z] != (int32_t)NS)
        return failp(err, HEAT_E_SIZE, "air handler tables: the offsets run from %d to %d for %zu branches and from %d to %d for %zu supply branches",
                     t.unit_off[0], t.unit_off[U], B, t.zone_off[0], t.zone_off[Z], NS);
    for (size_t u = 0; u < U; u++)
        if (t.unit_off[u + 1] < t.unit_off[u] || t.unit_off[u + 1] > (int32_t)B)
            return failp(err, HEAT_E_SIZE, "air handler tables: air handler %zu runs from %d to %d", u, t.unit_off[u], t.unit_off[u + 1]);
    for (size_t z = 0; z < Z; z++)
        if (t.zone_off[z + 1] < t.zone_off[z] || t.zone_off[z + 1] > (int32_t)NS)
            return failp(err, HEAT_E_SIZE, "air handler tables: zone %zu runs from %d to %d", z, t.zone_off[z], t.zone_off[z + 1]);
    // every branch of the caller's, in the caller's order, is the next element of its unit's range and, where it supplies, of
    // its zone's ...
    std::vector<int32_t> cu(t.unit_off.begin(), t.unit_off.end() - 1), cz(t.zone_off.begin(), t.zone_off.end() - 1);
    for (size_t j = 0; j < B; j++) {
        const size_t u = (size_t)h->br_unit[j], z = (size_t)h->br_zone[j];
        const unsigned kind = h->br_kind ? h->br_kind[j] : 3u;
        const double gain = h->br_volume_gain ? h->br_volume_gain[j] : 1.0;
        const int32_t p = cu[u]++;
        if (p >= t.unit_off[u + 1]) return failp(err, HEAT_E_SIZE, "air handler tables: air handler branch %zu: air handler %zu has no room for it", j, u);
        if (t.u_orig[p] != (int32_t)j || t.u_zone[p] != h->br_zone[j] || t.u_chan[p] != h->br_volume_chan[j] || (unsigned)t.u_kind[p] != kind ||
            std::memcmp(&t.u_gain[p], &gain, sizeof(double)) != 0)
            return failp(err, HEAT_E_SIZE, "air handler tables: air handler branch %zu is not element %d of air handler %zu", j, p - t.unit_off[u], u);
        if (!(kind & 1u)) continue;
        const int32_t q = cz[z]++;
        if (q >= t.zone_off[z + 1]) return failp(err, HEAT_E_SIZE, "air handler tables: air handler branch %zu: zone %zu has no room for it", j, z);
        if (t.z_orig[q] != (int32_t)j || t.z_unit[q] != h->br_unit[j])
            return failp(err, HEAT_E_SIZE, "air handler tables: air handler branch %zu is not element %d of zone %zu", j, q - t.zone_off[z], z);
    }
    // ... and every range is full: each branch is present exactly once
    for (size_t u = 0; u < U; u++)
        if (cu[u] != t.unit_off[u + 1])
            return failp(err, HEAT_E_SIZE, "air handler tables: air handler %zu holds %d branches of %d", u, cu[u] - t.unit_off[u], t.unit_off[u + 1] - t.unit_off[u]);
    for (size_t z = 0; z < Z; z++)
        if (cz[z] != t.zone_off[z + 1])
            return failp(err, HEAT_E_SIZE, "air handler tables: zone %zu holds %d supply branches of %d", z, cz[z] - t.zone_off[z], t.zone_off[z + 1] - t.zone_off[z]);
    // the units' rows
    const double inf = std::numeric_limits<double>::infinity();
    for (size_t u = 0; u < U; u++) {
        const int32_t bc = h->bypass_chan ? h->bypass_chan[u] : -1;
        const int32_t i32[kHandlerI32Rows] = {h->outdoor_chan[u], h->eff_chan ? h->eff_chan[u] : -1, bc, h->heat_chan ? h->heat_chan[u] : -1,
                                              h->cool_chan ? h->cool_chan[u] : -1};
        const double f64[kHandlerF64Rows] = {h->eff_gain ? h->eff_gain[u] : 1.0, bc >= 0 ? h->bypass_band[u] / 2.0 : 0.0,
                                             bc >= 0 ? h->bypass_min_delta[u] : 0.0, h->heat_cap ? h->heat_cap[u] : inf,
                                             h->cool_cap ? h->cool_cap[u] : inf};
        for (int a = 0; a < kHandlerI32Rows; a++)
            if (t.i32[a * U + u] != i32[a]) return failp(err, HEAT_E_SIZE, "air handler tables: air handler %zu: row %d is not the caller's", u, a);
        for (int a = 0; a < kHandlerF64Rows; a++)
            if (std::memcmp(&t.f64[a * U + u], &f64[a], sizeof(double)) != 0)
                return failp(err, HEAT_E_SIZE, "air handler tables: air handler %zu: real row %d is not the caller's", u, a);
    }
    return HEAT_OK;
}

// ---- ideal loads in the cluster-resident march: eligibility of a batch (plan.hpp) ----
int ideal_resident_reason(const size_t (&n_blocks)[kNumFast][4], const size_t (&n_supers)[kNumFast], const bool (&has_chunks)[kNumFast]) {
    bool any = false, teams = false, cavity = false, chunks = false;
    for (int c = 0; c < kNumFast; c++) {
        if (n_supers[c] > 0) any = teams = true;
        for (int g2 = 0; g2 < 4; g2++) {
            if (n_blocks[c][g2] == 0) continue;
            any = true;
            // (a list of workgroups with small surfaces marches the universal variant of its blocking factor whatever
            // its class — cavities allowed —, and that variant has its ideal instantiation: kernels.hip)
            if (kFastCAV[c] && !(g2 >> 1)) cavity = true;
            // (the launch's choice of the chunk-loop variant, NM = 2: batch.hip, enqueue_fused)
            if (kFastNM[c] && has_chunks[c] && !(g2 >> 1) && !kFastCAV[c] && kFastM[c] <= 8) chunks = true;
        }
    }
    if (!any) return HEAT_IDEAL_RESIDENT_NONE_PLANNED;
    if (teams) return HEAT_IDEAL_RESIDENT_TEAMS;
    if (cavity) return HEAT_IDEAL_RESIDENT_CAVITY_CLASS;
    if (chunks) return HEAT_IDEAL_RESIDENT_CHUNK_LOOP_CLASS;
    return HEAT_IDEAL_RESIDENT_OK;
}

const char *ideal_resident_reason_text(int reason) {
    switch (reason) {
    case HEAT_IDEAL_RESIDENT_OK: return "eligible";
    case HEAT_IDEAL_RESIDENT_NONE_PLANNED: return "nothing of the batch is planned resident";
    case HEAT_IDEAL_RESIDENT_TEAMS: return "clusters marched by teams of workgroups";
    case HEAT_IDEAL_RESIDENT_CAVITY_CLASS: return "resident workgroups of walls only in a class with gas cavities";
    case HEAT_IDEAL_RESIDENT_CHUNK_LOOP_CLASS: return "resident workgroups of a class with no-mass chunks other than facings";
    default: return "unknown";
    }
}

// ---- air species of a series (include/heat_amd.h, heat_air_species) ----
int check_air_species(int64_t n_zones, int32_t n_channels, const heat_air_species *sp, std::string &err) {
    if (!sp) return HEAT_OK;
    const int64_t NS = sp->n_species, NQ = sp->n_sources, NV = sp->n_vents, Z = n_zones;
    const int NC = n_channels;
    if (NS < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count of air species (n_species %lld): no air species s", (long long)NS);
    if (NQ < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count of species sources (n_sources %lld): no species source i", (long long)NQ);
    if (NV < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count of demand vents (n_vents %lld): no demand vent j", (long long)NV);
    // (the tables number lanes, sources and vents with 32 bits)
    if (NS > INT32_MAX || NQ > INT32_MAX || NV > INT32_MAX || (Z > 0 && NS > INT32_MAX / Z))
        return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 lanes of air species s, species sources i or demand vents j (n_species %lld x %lld zones, n_sources %lld, n_vents %lld)",
                     (long long)NS, (long long)Z, (long long)NQ, (long long)NV);
    if (NS == 0 && NQ > 0) return failp(err, HEAT_E_INVALID_ARG, "species source 0: %lld sources, but no air species s (n_species 0)", (long long)NQ);
    if (NS == 0 && NV > 0) return failp(err, HEAT_E_INVALID_ARG, "demand vent 0: %lld vents, but no air species s (n_species 0)", (long long)NV);
    if (NS == 0) return HEAT_OK;
    if (Z > 0 && !sp->outdoor_chan) return failp(err, HEAT_E_INVALID_ARG, "air species 0: outdoor_chan is NULL (n_species %lld)", (long long)NS);
    if (Z > 0 && !sp->conc) return failp(err, HEAT_E_INVALID_ARG, "air species 0: conc is NULL (n_species %lld)", (long long)NS);
    for (int64_t s = 0; s < NS; s++) {
        for (int64_t z = 0; z < Z; z++) {
            const int32_t oc = sp->outdoor_chan[s * Z + z];
            if (oc < -1 || oc >= NC)
                return failp(err, HEAT_E_SIZE, "air species %lld: outdoor channel %d of zone %lld outside [-1, %d)", (long long)s, oc, (long long)z, NC);
        }
        const int32_t lc = sp->limit_chan ? sp->limit_chan[s] : -1;
        if (lc < -1 || lc >= NC) return failp(err, HEAT_E_SIZE, "air species %lld: limit channel %d outside [-1, %d)", (long long)s, lc, NC);
    }
    for (int64_t z = 0; sp->occ_chan && z < Z; z++)
        if (sp->occ_chan[z] < -1 || sp->occ_chan[z] >= NC)
            return failp(err, HEAT_E_SIZE, "air species 0: occupancy channel %d of zone %lld outside [-1, %d)", sp->occ_chan[z], (long long)z, NC);
    if (NQ > 0 && (!sp->src_zone || !sp->src_species || !sp->src_chan))
        return failp(err, HEAT_E_INVALID_ARG, "species source 0: %s is NULL (n_sources %lld)",
                     !sp->src_zone ? "src_zone" : (!sp->src_species ? "src_species" : "src_chan"), (long long)NQ);
    for (int64_t i = 0; i < NQ; i++) {
        const int32_t z = sp->src_zone[i], s = sp->src_species[i], ch = sp->src_chan[i];
        if (z < 0 || z >= Z) return failp(err, HEAT_E_SIZE, "species source %lld: zone %d outside [0, %lld)", (long long)i, z, (long long)Z);
        if (s < 0 || s >= NS) return failp(err, HEAT_E_SIZE, "species source %lld: species %d outside [0, %lld)", (long long)i, s, (long long)NS);
        if (ch < 0 || ch >= NC) return failp(err, HEAT_E_SIZE, "species source %lld: channel %d outside [0, %d)", (long long)i, ch, NC);
        if (sp->src_factor && !std::isfinite(sp->src_factor[i]))
            return failp(err, HEAT_E_INVALID_ARG, "species source %lld: src_factor %g is not finite", (long long)i, sp->src_factor[i]);
    }
    if (NV == 0) return HEAT_OK;
    const void *const need[7] = {sp->vent_zone, sp->vent_species, sp->vent_temp_chan, sp->vent_v_min, sp->vent_v_max, sp->vent_c_lo, sp->vent_c_hi};
    static const char *const need_name[7] = {"vent_zone", "vent_species", "vent_temp_chan", "vent_v_min", "vent_v_max", "vent_c_lo", "vent_c_hi"};
    for (int a = 0; a < 7; a++)
        if (!need[a]) return failp(err, HEAT_E_INVALID_ARG, "demand vent 0: %s is NULL (n_vents %lld)", need_name[a], (long long)NV);
    for (int64_t j = 0; j < NV; j++) {
        const int32_t z = sp->vent_zone[j], s = sp->vent_species[j], tc = sp->vent_temp_chan[j];
        const int32_t ec = sp->vent_enable_chan ? sp->vent_enable_chan[j] : -1;
        if (z < 0 || z >= Z) return failp(err, HEAT_E_SIZE, "demand vent %lld: zone %d outside [0, %lld)", (long long)j, z, (long long)Z);
        if (s < 0 || s >= NS) return failp(err, HEAT_E_SIZE, "demand vent %lld: species %d outside [0, %lld)", (long long)j, s, (long long)NS);
        if (tc < 0 || tc >= NC) return failp(err, HEAT_E_SIZE, "demand vent %lld: temperature channel %d outside [0, %d)", (long long)j, tc, NC);
        if (ec < -1 || ec >= NC) return failp(err, HEAT_E_SIZE, "demand vent %lld: enable channel %d outside [-1, %d)", (long long)j, ec, NC);
        const double v[4] = {sp->vent_v_min[j], sp->vent_v_max[j], sp->vent_c_lo[j], sp->vent_c_hi[j]};
        for (int a = 0; a < 4; a++)
            if (!std::isfinite(v[a])) return failp(err, HEAT_E_INVALID_ARG, "demand vent %lld: %s %g is not finite", (long long)j, need_name[3 + a], v[a]);
        if (v[0] < 0.0) return failp(err, HEAT_E_INVALID_ARG, "demand vent %lld: vent_v_min %g is negative", (long long)j, v[0]);
        if (v[1] < v[0]) return failp(err, HEAT_E_INVALID_ARG, "demand vent %lld: vent_v_max %g is below vent_v_min %g", (long long)j, v[1], v[0]);
        if (v[3] <= v[2]) return failp(err, HEAT_E_INVALID_ARG, "demand vent %lld: vent_c_hi %g is not above vent_c_lo %g", (long long)j, v[3], v[2]);
    }
    return HEAT_OK;
}

void build_air_species_tables(int64_t n_zones, const heat_air_handlers *h, const heat_air_species *sp, SpeciesTables &t) {
    t = SpeciesTables();
    const size_t NS = sp ? (size_t)sp->n_species : 0, Z = (size_t)n_zones;
    if (NS == 0) return;
    const size_t NQ = (size_t)sp->n_sources, NV = (size_t)sp->n_vents, L = NS * Z;
    t.outdoor_chan.assign(sp->outdoor_chan, sp->outdoor_chan + L);
    t.limit_chan.assign(NS, -1);
    t.occ_chan.assign(Z, -1);
    if (sp->limit_chan) std::copy(sp->limit_chan, sp->limit_chan + NS, t.limit_chan.begin());
    if (sp->occ_chan) std::copy(sp->occ_chan, sp->occ_chan + Z, t.occ_chan.begin());
    // two counting sorts, stable: the caller's order survives inside a lane and inside a zone
    t.src_off.assign(L + 1, 0);
    t.vent_off.assign(Z + 1, 0);
    for (size_t i = 0; i < NQ; i++) t.src_off[(size_t)sp->src_species[i] * Z + (size_t)sp->src_zone[i] + 1]++;
    for (size_t j = 0; j < NV; j++) t.vent_off[(size_t)sp->vent_zone[j] + 1]++;
    for (size_t l = 0; l < L; l++) t.src_off[l + 1] += t.src_off[l];
    for (size_t z = 0; z < Z; z++) t.vent_off[z + 1] += t.vent_off[z];
    t.src_chan.resize(NQ), t.src_factor.resize(NQ);
    t.v_species.resize(NV), t.v_temp_chan.resize(NV), t.v_enable_chan.resize(NV), t.v_orig.resize(NV);
    t.v_min.resize(NV), t.v_max.resize(NV), t.c_lo.resize(NV), t.c_hi.resize(NV);
    std::vector<int32_t> next_s(t.src_off.begin(), t.src_off.end() - 1), next_v(t.vent_off.begin(), t.vent_off.end() - 1);
    for (size_t i = 0; i < NQ; i++) {
        const size_t p = (size_t)next_s[(size_t)sp->src_species[i] * Z + (size_t)sp->src_zone[i]]++;
        t.src_chan[p] = sp->src_chan[i];
        t.src_factor[p] = sp->src_factor ? sp->src_factor[i] : 1.0;
    }
    for (size_t j = 0; j < NV; j++) {
        const size_t p = (size_t)next_v[(size_t)sp->vent_zone[j]]++;
        t.v_species[p] = sp->vent_species[j];
        t.v_temp_chan[p] = sp->vent_temp_chan[j];
        t.v_enable_chan[p] = sp->vent_enable_chan ? sp->vent_enable_chan[j] : -1;
        t.v_orig[p] = (int32_t)j;
        t.v_min[p] = sp->vent_v_min[j], t.v_max[p] = sp->vent_v_max[j], t.c_lo[p] = sp->vent_c_lo[j], t.c_hi[p] = sp->vent_c_hi[j];
    }
    const size_t B = h && h->n_units > 0 ? (size_t)h->n_branches : 0;
    t.br_chan.resize(B), t.br_gain.resize(B);
    for (size_t j = 0; j < B; j++) {
        t.br_chan[j] = h->br_volume_chan[j];
        t.br_gain[j] = h->br_volume_gain ? h->br_volume_gain[j] : 1.0;
    }
}

int check_air_species_tables(int64_t n_zones, const heat_air_handlers *h, const heat_air_species *sp, const SpeciesTables &t,
                             std::string &err) {
    const size_t NS = sp ? (size_t)sp->n_species : 0, Z = (size_t)n_zones;
    if (NS == 0) return HEAT_OK;
    const size_t NQ = (size_t)sp->n_sources, NV = (size_t)sp->n_vents, L = NS * Z;
    const size_t B = h && h->n_units > 0 ? (size_t)h->n_branches : 0;
    if (t.outdoor_chan.size() != L || t.src_off.size() != L + 1 || t.src_chan.size() != NQ || t.src_factor.size() != NQ ||
        t.vent_off.size() != Z + 1 || t.v_species.size() != NV || t.v_temp_chan.size() != NV || t.v_enable_chan.size() != NV ||
        t.v_orig.size() != NV || t.v_min.size() != NV || t.v_max.size() != NV || t.c_lo.size() != NV || t.c_hi.size() != NV ||
        t.limit_chan.size() != NS || t.occ_chan.size() != Z || t.br_chan.size() != B || t.br_gain.size() != B)
        return failp(err, HEAT_E_SIZE, "air species tables: %zu source offsets, %zu vent offsets, %zu and %zu elements for air species s < %zu, species source i < %zu, demand vent j < %zu",
                     t.src_off.size(), t.vent_off.size(), t.src_chan.size(), t.v_orig.size(), NS, NQ, NV);
    if (t.src_off[0] != 0 || t.src_off[L] != (int32_t)NQ || t.vent_off[0] != 0 || t.vent_off[Z] != (int32_t)NV)
        return failp(err, HEAT_E_SIZE, "air species tables: the offsets run from %d to %d for %zu sources and from %d to %d for %zu vents",
                     t.src_off[0], t.src_off[L], NQ, t.vent_off[0], t.vent_off[Z], NV);
    for (size_t l = 0; l < L; l++)
        if (t.src_off[l + 1] < t.src_off[l] || t.src_off[l + 1] > (int32_t)NQ)
            return failp(err, HEAT_E_SIZE, "air species tables: air species %zu, zone %zu runs from %d to %d", l / Z, l % Z, t.src_off[l], t.src_off[l + 1]);
    for (size_t z = 0; z < Z; z++)
        if (t.vent_off[z + 1] < t.vent_off[z] || t.vent_off[z + 1] > (int32_t)NV)
            return failp(err, HEAT_E_SIZE, "air species tables: zone %zu runs from %d to %d", z, t.vent_off[z], t.vent_off[z + 1]);
    // every source and vent of the caller's, in the caller's order, is the next element of its range ...
    std::vector<int32_t> cs(t.src_off.begin(), t.src_off.end() - 1), cv(t.vent_off.begin(), t.vent_off.end() - 1);
    for (size_t i = 0; i < NQ; i++) {
        const size_t l = (size_t)sp->src_species[i] * Z + (size_t)sp->src_zone[i];
        const double factor = sp->src_factor ? sp->src_factor[i] : 1.0;
        const int32_t p = cs[l]++;
        if (p >= t.src_off[l + 1]) return failp(err, HEAT_E_SIZE, "air species tables: species source %zu: its lane has no room for it", i);
        if (t.src_chan[p] != sp->src_chan[i] || std::memcmp(&t.src_factor[p], &factor, sizeof(double)) != 0)
            return failp(err, HEAT_E_SIZE, "air species tables: species source %zu is not element %d of its lane", i, p - t.src_off[l]);
    }
    for (size_t j = 0; j < NV; j++) {
        const size_t z = (size_t)sp->vent_zone[j];
        const int32_t p = cv[z]++;
        if (p >= t.vent_off[z + 1]) return failp(err, HEAT_E_SIZE, "air species tables: demand vent %zu: zone %zu has no room for it", j, z);
        const double want[4] = {sp->vent_v_min[j], sp->vent_v_max[j], sp->vent_c_lo[j], sp->vent_c_hi[j]};
        const double have[4] = {t.v_min[p], t.v_max[p], t.c_lo[p], t.c_hi[p]};
        if (t.v_orig[p] != (int32_t)j || t.v_species[p] != sp->vent_species[j] || t.v_temp_chan[p] != sp->vent_temp_chan[j] ||
            t.v_enable_chan[p] != (sp->vent_enable_chan ? sp->vent_enable_chan[j] : -1) || std::memcmp(want, have, sizeof want) != 0)
            return failp(err, HEAT_E_SIZE, "air species tables: demand vent %zu is not element %d of zone %zu", j, p - t.vent_off[z], z);
    }
    // ... and every range is full: each is present exactly once
    for (size_t l = 0; l < L; l++)
        if (cs[l] != t.src_off[l + 1])
            return failp(err, HEAT_E_SIZE, "air species tables: air species %zu, zone %zu holds %d sources of %d", l / Z, l % Z, cs[l] - t.src_off[l], t.src_off[l + 1] - t.src_off[l]);
    for (size_t z = 0; z < Z; z++)
        if (cv[z] != t.vent_off[z + 1])
            return failp(err, HEAT_E_SIZE, "air species tables: zone %zu holds %d demand vents of %d", z, cv[z] - t.vent_off[z], t.vent_off[z + 1] - t.vent_off[z]);
    // the rows
    for (size_t l = 0; l < L; l++)
        if (t.outdoor_chan[l] != sp->outdoor_chan[l])
            return failp(err, HEAT_E_SIZE, "air species tables: air species %zu: the outdoor channel of zone %zu is not the caller's", l / Z, l % Z);
    for (size_t s = 0; s < NS; s++)
        if (t.limit_chan[s] != (sp->limit_chan ? sp->limit_chan[s] : -1))
            return failp(err, HEAT_E_SIZE, "air species tables: air species %zu: the limit channel is not the caller's", s);
    for (size_t z = 0; z < Z; z++)
        if (t.occ_chan[z] != (sp->occ_chan ? sp->occ_chan[z] : -1))
            return failp(err, HEAT_E_SIZE, "air species tables: air species 0: the occupancy channel of zone %zu is not the caller's", z);
    for (size_t j = 0; j < B; j++) {
        const double gain = h->br_volume_gain ? h->br_volume_gain[j] : 1.0;
        if (t.br_chan[j] != h->br_volume_chan[j] || std::memcmp(&t.br_gain[j], &gain, sizeof(double)) != 0)
            return failp(err, HEAT_E_SIZE, "air species tables: air species 0: branch %zu of the handlers is not the caller's", j);
    }
    return HEAT_OK;
}

// ---- openings of a series (include/heat_amd.h, heat_openings) ----
int check_openings(int64_t n_zones, int32_t n_channels, const heat_openings *op, std::string &err) {
    if (!op) return HEAT_OK;
    const int64_t n = op->n_openings;
    if (n < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count of openings (opening count n_openings %lld)", (long long)n);
    // (the tables number the openings with 32 bits)
    if (n > INT32_MAX) return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 openings (opening count n_openings %lld)", (long long)n);
    if (n == 0) return HEAT_OK;
    if (!op->zone_a) return failp(err, HEAT_E_INVALID_ARG, "opening 0: zone_a is NULL");
    if (!op->zone_b) return failp(err, HEAT_E_INVALID_ARG, "opening 0: zone_b is NULL");
    if (!op->out_chan) return failp(err, HEAT_E_INVALID_ARG, "opening 0: out_chan is NULL");
    if (!op->area) return failp(err, HEAT_E_INVALID_ARG, "opening 0: area is NULL");
    for (int64_t i = 0; i < n; i++) {
        const int32_t za = op->zone_a[i], zb = op->zone_b[i], oc = op->out_chan[i];
        const int32_t tc = op->temp_chan ? op->temp_chan[i] : -1, wc = op->wind_chan ? op->wind_chan[i] : -1;
        const int32_t fc = op->frac_chan ? op->frac_chan[i] : -1;
        if (za < 0 || za >= n_zones)
            return failp(err, HEAT_E_SIZE, "opening %lld: zone_a %d outside [0, %lld)", (long long)i, za, (long long)n_zones);
        if (zb < -1 || zb >= n_zones)
            return failp(err, HEAT_E_SIZE, "opening %lld: zone_b %d outside [-1, %lld)", (long long)i, zb, (long long)n_zones);
        if (za == zb) return failp(err, HEAT_E_INVALID_ARG, "opening %lld: zone_a and zone_b are the same zone %d", (long long)i, za);
        if (oc < 0 || oc >= n_channels)
            return failp(err, HEAT_E_SIZE, "opening %lld: derived channel out_chan %d outside [0, %d)", (long long)i, oc, n_channels);
        if (zb == -1 && (tc < 0 || tc >= n_channels))
            return failp(err, HEAT_E_SIZE, "opening %lld: zone_b -1 (outside air) needs a temperature channel in [0, %d), not %d%s", (long long)i,
                         n_channels, tc, op->temp_chan ? "" : " (temp_chan is NULL)");
        if (zb >= 0 && tc != -1)
            return failp(err, HEAT_E_SIZE, "opening %lld: it joins zone %d to zone %d and names temperature channel %d: a side has one temperature",
                         (long long)i, za, zb, tc);
        if (wc < -1 || wc >= n_channels)
            return failp(err, HEAT_E_SIZE, "opening %lld: wind channel %d outside [-1, %d)", (long long)i, wc, n_channels);
        if (fc < -1 || fc >= n_channels)
            return failp(err, HEAT_E_SIZE, "opening %lld: open-fraction channel %d outside [-1, %d)", (long long)i, fc, n_channels);
        const double *const coef[5] = {op->area, op->cw, op->cs, op->ca, op->c0};
        static const char *const name[5] = {"area", "cw", "cs", "ca", "c0"};
        for (int a = 0; a < 5; a++)
            if (coef[a] && (!std::isfinite(coef[a][i]) || coef[a][i] < 0.0))
                return failp(err, HEAT_E_INVALID_ARG, "opening %lld: %s %g is negative or not finite", (long long)i, name[a], coef[a][i]);
    }
    // a derived channel has one writer, and feeds consumers: never another opening (nor its own)
    std::vector<int32_t> writer((size_t)n_channels, -1);
    for (int64_t i = 0; i < n; i++) {
        int32_t &w = writer[(size_t)op->out_chan[i]];
        if (w >= 0)
            return failp(err, HEAT_E_SIZE, "opening %lld: its derived channel out_chan %d is also opening %d's: a derived channel has one writer",
                         (long long)i, op->out_chan[i], w);
        w = (int32_t)i;
    }
    for (int64_t i = 0; i < n; i++) {
        const int32_t *const read[3] = {op->temp_chan, op->wind_chan, op->frac_chan};
        static const char *const name[3] = {"temp_chan", "wind_chan", "frac_chan"};
        for (int a = 0; a < 3; a++) {
            const int32_t ch = read[a] ? read[a][i] : -1;
            if (ch >= 0 && writer[(size_t)ch] >= 0)
                return failp(err, HEAT_E_SIZE, "opening %lld: its %s %d is the derived channel of opening %d: a derived channel feeds consumers, never an opening",
                             (long long)i, name[a], ch, writer[(size_t)ch]);
        }
    }
    return HEAT_OK;
}

void build_opening_tables(const heat_openings *op, OpeningTables &t) {
    const size_t n = op ? (size_t)op->n_openings : 0;
    t = OpeningTables();
    t.n_openings = (int64_t)n;
    t.i32.assign((size_t)kOpeningI32Rows * n, -1);
    t.f64.assign((size_t)kOpeningF64Rows * n, 0.0);
    if (n == 0) return;
    const int32_t *const src_i32[kOpeningI32Rows] = {op->zone_a, op->zone_b, op->temp_chan, op->wind_chan, op->frac_chan, op->out_chan};
    const double *const src_f64[kOpeningF64Rows] = {op->area, op->cw, op->cs, op->ca, op->c0};
    for (int a = 0; a < kOpeningI32Rows; a++)
        if (src_i32[a]) std::copy(src_i32[a], src_i32[a] + n, t.i32.begin() + (size_t)a * n);
    for (int a = 0; a < kOpeningF64Rows; a++)
        if (src_f64[a]) std::copy(src_f64[a], src_f64[a] + n, t.f64.begin() + (size_t)a * n);
}

int check_opening_tables(int64_t n_zones, int32_t n_channels, const heat_openings *op, const OpeningTables &t, std::string &err) {
    const size_t n = op ? (size_t)op->n_openings : 0;
    if (t.n_openings != (int64_t)n || t.i32.size() != (size_t)kOpeningI32Rows * n || t.f64.size() != (size_t)kOpeningF64Rows * n)
        return failp(err, HEAT_E_SIZE, "opening tables: %zu integers and %zu reals for %zu openings", t.i32.size(), t.f64.size(), n);
    if (n == 0) return HEAT_OK;
    const int32_t *const src_i32[kOpeningI32Rows] = {op->zone_a, op->zone_b, op->temp_chan, op->wind_chan, op->frac_chan, op->out_chan};
    const double *const src_f64[kOpeningF64Rows] = {op->area, op->cw, op->cs, op->ca, op->c0};
    std::vector<uint8_t> written((size_t)n_channels, 0);
    for (size_t i = 0; i < n; i++) {
        // every row the caller's ...
        for (int a = 0; a < kOpeningI32Rows; a++)
            if (t.list(a)[i] != (src_i32[a] ? src_i32[a][i] : -1))
                return failp(err, HEAT_E_SIZE, "opening tables: opening %zu: integer row %d is not the caller's", i, a);
        for (int a = 0; a < kOpeningF64Rows; a++) {
            const double want = src_f64[a] ? src_f64[a][i] : 0.0;
            if (std::memcmp(&t.real(a)[i], &want, sizeof(double)) != 0)
                return failp(err, HEAT_E_SIZE, "opening tables: opening %zu: real row %d is not the caller's", i, a);
        }
        // ... and everything the lane indexes with inside its array
        const int32_t za = t.list(OP_ZONE_A)[i], zb = t.list(OP_ZONE_B)[i], tc = t.list(OP_TEMP_CHAN)[i], oc = t.list(OP_OUT_CHAN)[i];
        if (za < 0 || za >= n_zones || zb >= n_zones || (zb < 0 && (tc < 0 || tc >= n_channels)) || oc < 0 || oc >= n_channels ||
            t.list(OP_WIND_CHAN)[i] >= n_channels || t.list(OP_FRAC_CHAN)[i] >= n_channels)
            return failp(err, HEAT_E_SIZE, "opening tables: opening %zu: a zone or channel lies outside its array", i);
        if (written[(size_t)oc]++) return failp(err, HEAT_E_SIZE, "opening tables: opening %zu: derived channel %d has two writers", i, oc);
    }
    for (size_t i = 0; i < n; i++)
        for (int a : {OP_TEMP_CHAN, OP_WIND_CHAN, OP_FRAC_CHAN})
            if (t.list(a)[i] >= 0 && written[(size_t)t.list(a)[i]])
                return failp(err, HEAT_E_SIZE, "opening tables: opening %zu: it reads derived channel %d", i, t.list(a)[i]);
    return HEAT_OK;
}

// ---- controllers of a series (include/heat_amd.h, heat_controllers) ----
namespace {
// what a NULL list of a controller stands for
inline int32_t ct_i32(const int32_t *list, int64_t i, int32_t neutral) { return list ? list[i] : neutral; }
inline double ct_f64(const double *list, int64_t i) { return list ? list[i] : 0.0; }
}  // namespace

int check_controllers(const SeriesModel &m, int32_t n_channels, const heat_openings *op, const heat_controllers *ct, std::string &err) {
    if (!ct) return HEAT_OK;
    const int64_t n = ct->n_controllers;
    if (n < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count of controllers (controller count n_controllers %lld)", (long long)n);
    // (the tables number the controllers with 32 bits)
    if (n > INT32_MAX) return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 controllers (controller count n_controllers %lld)", (long long)n);
    if (n == 0) return HEAT_OK;
    if (!ct->sense_index) return failp(err, HEAT_E_INVALID_ARG, "controller 0: sense_index is NULL");
    if (!ct->set_chan) return failp(err, HEAT_E_INVALID_ARG, "controller 0: set_chan is NULL");
    if (!ct->out_chan) return failp(err, HEAT_E_INVALID_ARG, "controller 0: out_chan is NULL");
    if (!ct->kp) return failp(err, HEAT_E_INVALID_ARG, "controller 0: kp is NULL");
    if (!ct->out_hi) return failp(err, HEAT_E_INVALID_ARG, "controller 0: out_hi is NULL");
    // where a controller senses or limits: the kind in its range, then the zone, surface and node, or channel in theirs
    auto place = [&](int64_t i, const char *what, int32_t kind, int32_t index, int32_t node) {
        if (kind == 0 && (index < 0 || index >= m.n_zones))
            return failp(err, HEAT_E_SIZE, "controller %lld: %s zone %d outside [0, %lld)", (long long)i, what, index, (long long)m.n_zones);
        if (kind == 1) {
            if (index < 0 || index >= m.n_surfaces)
                return failp(err, HEAT_E_SIZE, "controller %lld: %s surface %d outside [0, %lld)", (long long)i, what, index, (long long)m.n_surfaces);
            if (node < -1 || node >= m.node_count[index])
                return failp(err, HEAT_E_SIZE, "controller %lld: %s node %d outside [-1, %lld), the nodes of surface %d", (long long)i, what, node,
                             (long long)m.node_count[index], index);
        }
        if (kind == 2 && (index < 0 || index >= n_channels))
            return failp(err, HEAT_E_SIZE, "controller %lld: %s channel %d outside [0, %d)", (long long)i, what, index, n_channels);
        return (int)HEAT_OK;
    };
    for (int64_t i = 0; i < n; i++) {
        const int32_t sk = ct_i32(ct->sense_kind, i, 0), lk = ct_i32(ct->lim_kind, i, -1);
        const int32_t sc = ct->set_chan[i], ec = ct_i32(ct->en_chan, i, -1), oc = ct->out_chan[i];
        if (sk < 0 || sk > 2)
            return failp(err, HEAT_E_INVALID_ARG, "controller %lld: sense_kind %d is none of 0 (zone), 1 (node), 2 (channel)", (long long)i, sk);
        if (lk < -1 || lk > 2)
            return failp(err, HEAT_E_INVALID_ARG, "controller %lld: lim_kind %d is none of -1 (no limit), 0 (zone), 1 (node), 2 (channel)", (long long)i, lk);
        if (lk >= 0 && (!ct->lim_index || !ct->lim_hi || !ct->lim_lo))
            return failp(err, HEAT_E_INVALID_ARG, "controller %lld: a limit of kind %d needs lim_index, lim_hi and lim_lo, and one is NULL", (long long)i, lk);
        if (const int rc = place(i, "sense", sk, ct->sense_index[i], ct_i32(ct->sense_node, i, -1))) return rc;
        if (lk >= 0)
            if (const int rc = place(i, "limit", lk, ct->lim_index[i], ct_i32(ct->lim_node, i, -1))) return rc;
        if (sc == -1) return failp(err, HEAT_E_SIZE, "controller %lld: no setpoint channel (set_chan -1)", (long long)i);
        if (sc < 0 || sc >= n_channels)
            return failp(err, HEAT_E_SIZE, "controller %lld: setpoint channel %d outside [0, %d)", (long long)i, sc, n_channels);
        if (ec < -1 || ec >= n_channels)
            return failp(err, HEAT_E_SIZE, "controller %lld: enable channel %d outside [-1, %d)", (long long)i, ec, n_channels);
        if (oc < 0 || oc >= n_channels)
            return failp(err, HEAT_E_SIZE, "controller %lld: derived channel out_chan %d outside [0, %d)", (long long)i, oc, n_channels);
        const double *const real[7] = {ct->kp, ct->ki, ct->bias, ct->out_lo, ct->out_hi, lk >= 0 ? ct->lim_hi : nullptr, lk >= 0 ? ct->lim_lo : nullptr};
        static const char *const name[7] = {"kp", "ki", "bias", "out_lo", "out_hi", "lim_hi", "lim_lo"};
        for (int a = 0; a < 7; a++) {
            if (real[a] && !std::isfinite(real[a][i]))
                return failp(err, HEAT_E_INVALID_ARG, "controller %lld: %s %g is not finite", (long long)i, name[a], real[a][i]);
            if (a < 2 && real[a] && real[a][i] < 0.0)
                return failp(err, HEAT_E_INVALID_ARG, "controller %lld: %s %g is negative", (long long)i, name[a], real[a][i]);
        }
        if (lk >= 0 && ct->lim_lo[i] > ct->lim_hi[i])
            return failp(err, HEAT_E_INVALID_ARG, "controller %lld: lim_lo %g above lim_hi %g", (long long)i, ct->lim_lo[i], ct->lim_hi[i]);
        if (ct->resume && ct->tripped && ct->tripped[i] > 1)
            return failp(err, HEAT_E_INVALID_ARG, "controller %lld: tripped byte %d is neither 0 nor 1", (long long)i, (int)ct->tripped[i]);
        // (a NaN integral is data: a series that met one resumes with it)
        if (ct->resume && ct->integral && (ct->integral[i] < 0.0 || ct->integral[i] > 1.0))
            return failp(err, HEAT_E_INVALID_ARG, "controller %lld: integral %g outside [0, 1]", (long long)i, ct->integral[i]);
    }
    // a derived channel has one writer among the controllers and the openings ...
    std::vector<int32_t> writer((size_t)n_channels, -1), opening((size_t)n_channels, -1);
    const int64_t n_op = op ? op->n_openings : 0;
    for (int64_t j = 0; j < n_op; j++) opening[(size_t)op->out_chan[j]] = (int32_t)j;
    for (int64_t i = 0; i < n; i++) {
        const int32_t oc = ct->out_chan[i];
        if (writer[(size_t)oc] >= 0)
            return failp(err, HEAT_E_SIZE, "controller %lld: its derived channel out_chan %d is also controller %d's: a derived channel has one writer",
                         (long long)i, oc, writer[(size_t)oc]);
        if (opening[(size_t)oc] >= 0)
            return failp(err, HEAT_E_SIZE, "controller %lld: its derived channel out_chan %d is also opening %d's: a derived channel has one writer",
                         (long long)i, oc, opening[(size_t)oc]);
        writer[(size_t)oc] = (int32_t)i;
    }
    // ... and no controller reads one: not a controller's (no cascades), not an opening's (the openings run behind)
    for (int64_t i = 0; i < n; i++) {
        const int32_t sk = ct_i32(ct->sense_kind, i, 0), lk = ct_i32(ct->lim_kind, i, -1);
        const int32_t read[4] = {sk == 2 ? ct->sense_index[i] : -1, ct->set_chan[i], ct_i32(ct->en_chan, i, -1), lk == 2 ? ct->lim_index[i] : -1};
        static const char *const name[4] = {"sense channel", "set_chan", "en_chan", "limit channel"};
        for (int a = 0; a < 4; a++) {
            if (read[a] < 0) continue;
            if (writer[(size_t)read[a]] >= 0)
                return failp(err, HEAT_E_SIZE, "controller %lld: its %s %d is the derived channel of controller %d: a controller never reads a controller",
                             (long long)i, name[a], read[a], writer[(size_t)read[a]]);
            if (opening[(size_t)read[a]] >= 0)
                return failp(err, HEAT_E_SIZE, "controller %lld: its %s %d is the derived channel of opening %d: the openings run behind the controllers",
                             (long long)i, name[a], read[a], opening[(size_t)read[a]]);
        }
    }
    return HEAT_OK;
}

void build_controller_tables(const SeriesModel &m, const heat_controllers *ct, const std::function<uint32_t(int64_t, int)> &node_at,
                             ControllerTables &t) {
    const size_t n = ct ? (size_t)ct->n_controllers : 0;
    t = ControllerTables();
    t.n_controllers = (int64_t)n;
    t.i32.assign((size_t)kControllerI32Rows * n, -1);
    t.f64.assign((size_t)kControllerF64Rows * n, 0.0);
    if (n == 0) return;
    auto at = [&](int32_t kind, int32_t index, int32_t node) {
        if (kind != 1) return index;
        return (int32_t)node_at(index, node < 0 ? (int)m.node_count[index] - 1 : node);
    };
    int32_t *const I = t.i32.data();
    for (size_t i = 0; i < n; i++) {
        const int32_t sk = ct_i32(ct->sense_kind, (int64_t)i, 0), lk = ct_i32(ct->lim_kind, (int64_t)i, -1);
        I[CT_SENSE_KIND * n + i] = sk;
        I[CT_SENSE_AT * n + i] = at(sk, ct->sense_index[i], ct_i32(ct->sense_node, (int64_t)i, -1));
        I[CT_SET_CHAN * n + i] = ct->set_chan[i];
        I[CT_ACTION * n + i] = ct_i32(ct->action, (int64_t)i, 1);
        I[CT_EN_CHAN * n + i] = ct_i32(ct->en_chan, (int64_t)i, -1);
        I[CT_LIM_KIND * n + i] = lk;
        I[CT_LIM_AT * n + i] = lk >= 0 ? at(lk, ct->lim_index[i], ct_i32(ct->lim_node, (int64_t)i, -1)) : -1;
        I[CT_OUT_CHAN * n + i] = ct->out_chan[i];
        const double *const src[kControllerF64Rows] = {ct->kp, ct->ki, ct->bias, ct->out_lo, ct->out_hi, lk >= 0 ? ct->lim_hi : nullptr,
                                                       lk >= 0 ? ct->lim_lo : nullptr};
        for (int a = 0; a < kControllerF64Rows; a++) t.f64[(size_t)a * n + i] = ct_f64(src[a], (int64_t)i);
    }
}

int check_controller_tables(const SeriesModel &m, int32_t n_channels, int64_t n_nodes, const heat_controllers *ct, const ControllerTables &t,
                            std::string &err) {
    const size_t n = ct ? (size_t)ct->n_controllers : 0;
    if (t.n_controllers != (int64_t)n || t.i32.size() != (size_t)kControllerI32Rows * n || t.f64.size() != (size_t)kControllerF64Rows * n)
        return failp(err, HEAT_E_SIZE, "controller tables: %zu integers and %zu reals for %zu controllers", t.i32.size(), t.f64.size(), n);
    if (n == 0) return HEAT_OK;
    std::vector<uint8_t> written((size_t)n_channels, 0);
    auto inside = [&](int32_t kind, int32_t at) {
        const int64_t bound = kind == 0 ? m.n_zones : kind == 1 ? n_nodes : (int64_t)n_channels;
        return (int64_t)(uint32_t)at < bound;
    };
    for (size_t i = 0; i < n; i++) {
        const int32_t sk = t.list(CT_SENSE_KIND)[i], lk = t.list(CT_LIM_KIND)[i], oc = t.list(CT_OUT_CHAN)[i];
        // every row the caller's ...
        const bool same_i32 = sk == ct_i32(ct->sense_kind, (int64_t)i, 0) && lk == ct_i32(ct->lim_kind, (int64_t)i, -1) &&
                              t.list(CT_SET_CHAN)[i] == ct->set_chan[i] && t.list(CT_ACTION)[i] == ct_i32(ct->action, (int64_t)i, 1) &&
                              t.list(CT_EN_CHAN)[i] == ct_i32(ct->en_chan, (int64_t)i, -1) && oc == ct->out_chan[i];
        if (!same_i32) return failp(err, HEAT_E_SIZE, "controller tables: controller %zu: an integer row is not the caller's", i);
        const double *const src[kControllerF64Rows] = {ct->kp, ct->ki, ct->bias, ct->out_lo, ct->out_hi, lk >= 0 ? ct->lim_hi : nullptr,
                                                       lk >= 0 ? ct->lim_lo : nullptr};
        for (int a = 0; a < kControllerF64Rows; a++) {
            const double want = ct_f64(src[a], (int64_t)i);
            if (std::memcmp(&t.real(a)[i], &want, sizeof(double)) != 0)
                return failp(err, HEAT_E_SIZE, "controller tables: controller %zu: real row %d is not the caller's", i, a);
        }
        // ... and everything the lane indexes with inside its array
        if (sk < 0 || sk > 2 || lk < -1 || lk > 2 || !inside(sk, t.list(CT_SENSE_AT)[i]) || (lk >= 0 && !inside(lk, t.list(CT_LIM_AT)[i])) ||
            !inside(2, t.list(CT_SET_CHAN)[i]) || t.list(CT_EN_CHAN)[i] >= n_channels || !inside(2, oc))
            return failp(err, HEAT_E_SIZE, "controller tables: controller %zu: a zone, node or channel lies outside its array", i);
        if (written[(size_t)oc]++) return failp(err, HEAT_E_SIZE, "controller tables: controller %zu: derived channel %d has two writers", i, oc);
    }
    for (size_t i = 0; i < n; i++) {
        const int32_t read[4] = {t.list(CT_SENSE_KIND)[i] == 2 ? t.list(CT_SENSE_AT)[i] : -1, t.list(CT_SET_CHAN)[i], t.list(CT_EN_CHAN)[i],
                                 t.list(CT_LIM_KIND)[i] == 2 ? t.list(CT_LIM_AT)[i] : -1};
        for (int a = 0; a < 4; a++)
            if (read[a] >= 0 && written[(size_t)read[a]])
                return failp(err, HEAT_E_SIZE, "controller tables: controller %zu: it reads derived channel %d", i, read[a]);
    }
    return HEAT_OK;
}

// ---- air networks of a series (include/heat_amd.h, heat_air_networks) ----
namespace {
inline double nw_f64(const double *list, int64_t i, double neutral) { return list ? list[i] : neutral; }
inline int network_class(int n) { return n <= 8 ? 0 : n <= 16 ? 1 : n <= 32 ? 2 : 3; }
}  // namespace

int check_air_networks(int64_t n_zones, int32_t n_channels, const heat_openings *op, const heat_controllers *ct, const heat_air_networks *nw,
                       std::string &err) {
    if (!nw) return HEAT_OK;
    const int64_t W = nw->n_networks, N = nw->n_nodes, L = nw->n_links;
    if (W < 0 || N < 0 || L < 0)
        return failp(err, HEAT_E_INVALID_ARG, "negative count of air networks (n_networks %lld, n_nodes %lld, n_links %lld)", (long long)W,
                     (long long)N, (long long)L);
    if (W > INT32_MAX / 2 || N > INT32_MAX / 2 || L > INT32_MAX / 2)
        return failp(err, HEAT_E_INVALID_ARG, "more than 2^30 air networks, nodes or links (n_networks %lld, n_nodes %lld, n_links %lld)",
                     (long long)W, (long long)N, (long long)L);
    if (W == 0) {
        if (N != 0 || L != 0) return failp(err, HEAT_E_SIZE, "network 0: %lld nodes and %lld links without a network", (long long)N, (long long)L);
        return HEAT_OK;
    }
    if (!nw->net_offset) return failp(err, HEAT_E_INVALID_ARG, "network 0: net_offset is NULL");
    if (!nw->tol) return failp(err, HEAT_E_INVALID_ARG, "network 0: tol is NULL");
    if (!nw->max_iter) return failp(err, HEAT_E_INVALID_ARG, "network 0: max_iter is NULL");
    if (!nw->g_min) return failp(err, HEAT_E_INVALID_ARG, "network 0: g_min is NULL");
    if (N > 0 && !nw->node_zone) return failp(err, HEAT_E_INVALID_ARG, "node 0: node_zone is NULL");
    if (L > 0) {
        if (!nw->zone_a) return failp(err, HEAT_E_INVALID_ARG, "link 0: zone_a is NULL");
        if (!nw->zone_b) return failp(err, HEAT_E_INVALID_ARG, "link 0: zone_b is NULL");
        if (!nw->temp_chan) return failp(err, HEAT_E_INVALID_ARG, "link 0: temp_chan is NULL");
        if (!nw->c) return failp(err, HEAT_E_INVALID_ARG, "link 0: c is NULL");
        if (!nw->p_lin) return failp(err, HEAT_E_INVALID_ARG, "link 0: p_lin is NULL");
    }
    // the networks' extents and numbers
    if (nw->net_offset[0] != 0) return failp(err, HEAT_E_SIZE, "network 0: net_offset starts at %d, not at 0", nw->net_offset[0]);
    for (int64_t w = 0; w < W; w++) {
        const int64_t n = (int64_t)nw->net_offset[w + 1] - nw->net_offset[w];
        if (n < 1 || n > kNetworkMaxNodes)
            return failp(err, HEAT_E_SIZE, "network %lld: %lld nodes, outside [1, %d]", (long long)w, (long long)n, kNetworkMaxNodes);
        if (nw->net_offset[w + 1] > N)
            return failp(err, HEAT_E_SIZE, "network %lld: its nodes end at %d, beyond the %lld nodes", (long long)w, nw->net_offset[w + 1], (long long)N);
        if (!std::isfinite(nw->tol[w]) || nw->tol[w] < 0.0)
            return failp(err, HEAT_E_INVALID_ARG, "network %lld: tol %g is not finite or is negative", (long long)w, nw->tol[w]);
        if (!std::isfinite(nw->g_min[w]) || !(nw->g_min[w] > 0.0))
            return failp(err, HEAT_E_INVALID_ARG, "network %lld: g_min %g is not positive and finite", (long long)w, nw->g_min[w]);
        if (nw->max_iter[w] < 1 || nw->max_iter[w] > kNetworkMaxNodes)
            return failp(err, HEAT_E_INVALID_ARG, "network %lld: max_iter %d outside [1, %d]", (long long)w, nw->max_iter[w], kNetworkMaxNodes);
    }
    if (nw->net_offset[W] != N)
        return failp(err, HEAT_E_SIZE, "network %lld: net_offset ends at %d, not at the %lld nodes", (long long)(W - 1), nw->net_offset[W], (long long)N);
    // the nodes: a zone is in at most one network
    std::vector<int32_t> net_of_zone((size_t)n_zones, -1);
    for (int64_t w = 0; w < W; w++)
        for (int64_t i = nw->net_offset[w]; i < nw->net_offset[w + 1]; i++) {
            const int32_t z = nw->node_zone[i], sc = ct_i32(nw->src_chan, i, -1);
            if (z < 0 || z >= n_zones) return failp(err, HEAT_E_SIZE, "node %lld: zone %d outside [0, %lld)", (long long)i, z, (long long)n_zones);
            if (net_of_zone[(size_t)z] >= 0)
                return failp(err, HEAT_E_SIZE, "node %lld: zone %d is a node of network %d already: a zone is in at most one network", (long long)i, z,
                             net_of_zone[(size_t)z]);
            net_of_zone[(size_t)z] = (int32_t)w;
            if (sc < -1 || sc >= n_channels)
                return failp(err, HEAT_E_SIZE, "node %lld: source channel %d outside [-1, %d)", (long long)i, sc, n_channels);
            if (!std::isfinite(nw_f64(nw->src_gain, i, 1.0)))
                return failp(err, HEAT_E_INVALID_ARG, "node %lld: src_gain %g is not finite", (long long)i, nw->src_gain[i]);
            if (nw->resume && nw->pressure && !std::isfinite(nw->pressure[i]))
                return failp(err, HEAT_E_INVALID_ARG, "node %lld: pressure %g is not finite", (long long)i, nw->pressure[i]);
        }
    // the links
    std::vector<uint8_t> has_outside((size_t)W, 0);
    for (int64_t l = 0; l < L; l++) {
        const int32_t za = nw->zone_a[l], zb = nw->zone_b[l], tc = nw->temp_chan[l];
        const int32_t wc = ct_i32(nw->wp_chan, l, -1), fc = ct_i32(nw->frac_chan, l, -1);
        const int32_t oab = ct_i32(nw->out_ab, l, -1), oba = ct_i32(nw->out_ba, l, -1);
        if (za < 0 || za >= n_zones) return failp(err, HEAT_E_SIZE, "link %lld: zone_a %d outside [0, %lld)", (long long)l, za, (long long)n_zones);
        if (zb < -1 || zb >= n_zones) return failp(err, HEAT_E_SIZE, "link %lld: zone_b %d outside [-1, %lld)", (long long)l, zb, (long long)n_zones);
        if (za == zb) return failp(err, HEAT_E_INVALID_ARG, "link %lld: zone_a == zone_b == %d", (long long)l, za);
        const int32_t wa = net_of_zone[(size_t)za];
        if (wa < 0) return failp(err, HEAT_E_SIZE, "link %lld: zone_a %d is in no network", (long long)l, za);
        if (zb >= 0 && net_of_zone[(size_t)zb] != wa)
            return failp(err, HEAT_E_SIZE, "link %lld: zone_a %d is in network %d and zone_b %d in %d: a link stays within one network", (long long)l, za, wa,
                         zb, net_of_zone[(size_t)zb]);
        if (zb < 0 && tc == -1) return failp(err, HEAT_E_SIZE, "link %lld: a link to outside without a temperature channel (temp_chan -1)", (long long)l);
        if (zb >= 0 && (tc != -1 || wc != -1))
            return failp(err, HEAT_E_SIZE, "link %lld: a link between zones with an outside channel (temp_chan %d, wp_chan %d)", (long long)l, tc, wc);
        const int32_t chans[5] = {tc, wc, fc, oab, oba};
        static const char *const cname[5] = {"temp_chan", "wp_chan", "frac_chan", "out_ab", "out_ba"};
        for (int a = 0; a < 5; a++)
            if (chans[a] < -1 || chans[a] >= n_channels)
                return failp(err, HEAT_E_SIZE, "link %lld: %s %d outside [-1, %d)", (long long)l, cname[a], chans[a], n_channels);
        const double real[2] = {nw->c[l], nw_f64(nw->gh, l, 0.0)};
        static const char *const rname[2] = {"c", "gh"};
        for (int a = 0; a < 2; a++)
            if (!std::isfinite(real[a]) || real[a] < 0.0)
                return failp(err, HEAT_E_INVALID_ARG, "link %lld: %s %g is not finite or is negative", (long long)l, rname[a], real[a]);
        if (!std::isfinite(nw->p_lin[l]) || !(nw->p_lin[l] > 0.0))
            return failp(err, HEAT_E_INVALID_ARG, "link %lld: p_lin %g is not positive and finite", (long long)l, nw->p_lin[l]);
        if (!std::isfinite(nw_f64(nw->wp_gain, l, 1.0)))
            return failp(err, HEAT_E_INVALID_ARG, "link %lld: wp_gain %g is not finite", (long long)l, nw->wp_gain[l]);
        if (zb < 0) has_outside[(size_t)wa] = 1;
    }
    for (int64_t w = 0; w < W; w++)
        if (!has_outside[(size_t)w])
            return failp(err, HEAT_E_SIZE, "network %lld: no link to outside: its pressures have no reference", (long long)w);
    // every derived channel has one writer among the controllers, the openings and the links ...
    std::vector<int32_t> link_of((size_t)n_channels, -1), opening((size_t)n_channels, -1), controller((size_t)n_channels, -1);
    const int64_t n_op = op ? op->n_openings : 0, n_ct = ct ? ct->n_controllers : 0;
    for (int64_t j = 0; j < n_op; j++) opening[(size_t)op->out_chan[j]] = (int32_t)j;
    for (int64_t j = 0; j < n_ct; j++) controller[(size_t)ct->out_chan[j]] = (int32_t)j;
    for (int64_t l = 0; l < L; l++) {
        const int32_t out[2] = {ct_i32(nw->out_ab, l, -1), ct_i32(nw->out_ba, l, -1)};
        for (int a = 0; a < 2; a++) {
            const int32_t oc = out[a];
            if (oc < 0) continue;
            if (link_of[(size_t)oc] >= 0)
                return failp(err, HEAT_E_SIZE, "link %lld: its derived channel %s %d is also link %d's: a derived channel has one writer", (long long)l,
                             a ? "out_ba" : "out_ab", oc, link_of[(size_t)oc]);
            if (opening[(size_t)oc] >= 0)
                return failp(err, HEAT_E_SIZE, "link %lld: its derived channel %s %d is also opening %d's: a derived channel has one writer", (long long)l,
                             a ? "out_ba" : "out_ab", oc, opening[(size_t)oc]);
            if (controller[(size_t)oc] >= 0)
                return failp(err, HEAT_E_SIZE, "link %lld: its derived channel %s %d is also controller %d's: a derived channel has one writer",
                             (long long)l, a ? "out_ba" : "out_ab", oc, controller[(size_t)oc]);
            link_of[(size_t)oc] = (int32_t)l;
        }
    }
    // ... a network reads no opening's and no network's (a controller's it may) ...
    for (int64_t l = 0; l < L; l++) {
        const int32_t read[3] = {nw->temp_chan[l], ct_i32(nw->wp_chan, l, -1), ct_i32(nw->frac_chan, l, -1)};
        static const char *const name[3] = {"temp_chan", "wp_chan", "frac_chan"};
        for (int a = 0; a < 3; a++) {
            if (read[a] < 0) continue;
            if (link_of[(size_t)read[a]] >= 0)
                return failp(err, HEAT_E_SIZE, "link %lld: its %s %d is the derived channel of link %d: a network never reads a network", (long long)l,
                             name[a], read[a], link_of[(size_t)read[a]]);
            if (opening[(size_t)read[a]] >= 0)
                return failp(err, HEAT_E_SIZE, "link %lld: its %s %d is the derived channel of opening %d: a network never reads an opening", (long long)l,
                             name[a], read[a], opening[(size_t)read[a]]);
        }
    }
    for (int64_t i = 0; i < N; i++) {
        const int32_t sc = ct_i32(nw->src_chan, i, -1);
        if (sc < 0) continue;
        if (link_of[(size_t)sc] >= 0)
            return failp(err, HEAT_E_SIZE, "node %lld: its src_chan %d is the derived channel of link %d: a network never reads a network", (long long)i, sc,
                         link_of[(size_t)sc]);
        if (opening[(size_t)sc] >= 0)
            return failp(err, HEAT_E_SIZE, "node %lld: its src_chan %d is the derived channel of opening %d: a network never reads an opening", (long long)i,
                         sc, opening[(size_t)sc]);
    }
    // ... and no opening and no controller reads a network's: the networks run behind both
    for (int64_t j = 0; j < n_op; j++) {
        const int32_t read[3] = {ct_i32(op->temp_chan, j, -1), ct_i32(op->wind_chan, j, -1), ct_i32(op->frac_chan, j, -1)};
        for (int a = 0; a < 3; a++)
            if (read[a] >= 0 && link_of[(size_t)read[a]] >= 0)
                return failp(err, HEAT_E_SIZE, "link %d: its derived channel %d is read by opening %lld: the networks run behind the openings",
                             link_of[(size_t)read[a]], read[a], (long long)j);
    }
    for (int64_t j = 0; j < n_ct; j++) {
        const int32_t sk = ct_i32(ct->sense_kind, j, 0), lk = ct_i32(ct->lim_kind, j, -1);
        const int32_t read[4] = {sk == 2 ? ct->sense_index[j] : -1, ct->set_chan[j], ct_i32(ct->en_chan, j, -1), lk == 2 ? ct->lim_index[j] : -1};
        for (int a = 0; a < 4; a++)
            if (read[a] >= 0 && link_of[(size_t)read[a]] >= 0)
                return failp(err, HEAT_E_SIZE, "link %d: its derived channel %d is read by controller %lld: the networks run behind the controllers",
                             link_of[(size_t)read[a]], read[a], (long long)j);
    }
    return HEAT_OK;
}

void build_network_tables(const heat_air_networks *nw, NetworkTables &t) {
    t = NetworkTables();
    const size_t W = nw ? (size_t)nw->n_networks : 0, N = nw ? (size_t)nw->n_nodes : 0, L = nw ? (size_t)nw->n_links : 0;
    t.n_networks = (int64_t)W, t.n_nodes = (int64_t)N, t.n_links = (int64_t)L;
    t.net_i32.assign((size_t)kNetworkNetI32Rows * W, 0);
    t.net_f64.assign((size_t)kNetworkNetF64Rows * W, 0.0);
    t.node_i32.assign((size_t)kNetworkNodeI32Rows * N, -1);
    t.node_f64.assign(N, 1.0);
    t.link_i32.assign((size_t)kNetworkLinkI32Rows * L, -1);
    t.link_f64.assign((size_t)kNetworkLinkF64Rows * L, 0.0);
    if (W == 0) return;
    // the networks by width class, the caller's order within a class; their nodes behind one another
    int32_t count[kNetworkClasses] = {0, 0, 0, 0};
    for (size_t w = 0; w < W; w++) count[network_class(nw->net_offset[w + 1] - nw->net_offset[w])]++;
    for (int c = 0; c < kNetworkClasses; c++) t.class_start[c + 1] = t.class_start[c] + count[c];
    int32_t next[kNetworkClasses];
    for (int c = 0; c < kNetworkClasses; c++) next[c] = t.class_start[c];
    std::vector<int32_t> sorted_of_net(W);
    for (size_t w = 0; w < W; w++) sorted_of_net[w] = next[network_class(nw->net_offset[w + 1] - nw->net_offset[w])]++;
    std::vector<int32_t> net_at(W);
    for (size_t w = 0; w < W; w++) net_at[(size_t)sorted_of_net[w]] = (int32_t)w;
    int32_t *const NI = t.net_i32.data();
    int32_t *const DI = t.node_i32.data();
    std::vector<int32_t> sorted_of_node(N), local_of_node(N);
    int32_t at = 0;
    for (size_t s = 0; s < W; s++) {
        const size_t w = (size_t)net_at[s];
        const int32_t n = nw->net_offset[w + 1] - nw->net_offset[w];
        NI[NW_ID * W + s] = (int32_t)w, NI[NW_N * W + s] = n, NI[NW_NODE0 * W + s] = at, NI[NW_MAX_ITER * W + s] = nw->max_iter[w];
        t.net_f64[NW_TOL * W + s] = nw->tol[w], t.net_f64[NW_G_MIN * W + s] = nw->g_min[w];
        for (int32_t i = 0; i < n; i++) {
            const size_t id = (size_t)nw->net_offset[w] + (size_t)i, p = (size_t)at + (size_t)i;
            sorted_of_node[id] = (int32_t)p, local_of_node[id] = i;
            DI[ND_ID * N + p] = (int32_t)id, DI[ND_ZONE * N + p] = nw->node_zone[id], DI[ND_SRC_CHAN * N + p] = ct_i32(nw->src_chan, (int64_t)id, -1);
            t.node_f64[p] = nw_f64(nw->src_gain, (int64_t)id, 1.0);
        }
        at += n;
    }
    // the links in the caller's order, their nodes as local numbers; every node's incident links, ascending
    std::vector<int32_t> node_of_zone;
    for (size_t id = 0; id < N; id++) {
        const size_t z = (size_t)nw->node_zone[id];
        if (z >= node_of_zone.size()) node_of_zone.resize(z + 1, -1);
        node_of_zone[z] = (int32_t)id;
    }
    int32_t *const KI = t.link_i32.data();
    double *const KF = t.link_f64.data();
    std::vector<int32_t> degree(N, 0);
    for (size_t l = 0; l < L; l++) {
        const int32_t za = nw->zone_a[l], zb = nw->zone_b[l];
        const int32_t a = node_of_zone[(size_t)za], b = zb >= 0 ? node_of_zone[(size_t)zb] : -1;
        KI[LK_ZONE_A * L + l] = za, KI[LK_ZONE_B * L + l] = zb;
        KI[LK_LA * L + l] = local_of_node[(size_t)a], KI[LK_LB * L + l] = b >= 0 ? local_of_node[(size_t)b] : -1;
        KI[LK_TEMP_CHAN * L + l] = nw->temp_chan[l], KI[LK_WP_CHAN * L + l] = ct_i32(nw->wp_chan, (int64_t)l, -1);
        KI[LK_FRAC_CHAN * L + l] = ct_i32(nw->frac_chan, (int64_t)l, -1);
        KI[LK_OUT_AB * L + l] = ct_i32(nw->out_ab, (int64_t)l, -1), KI[LK_OUT_BA * L + l] = ct_i32(nw->out_ba, (int64_t)l, -1);
        KF[LK_C * L + l] = nw->c[l], KF[LK_GH * L + l] = nw_f64(nw->gh, (int64_t)l, 0.0), KF[LK_P_LIN * L + l] = nw->p_lin[l];
        KF[LK_S_LIN * L + l] = std::sqrt(nw->p_lin[l]), KF[LK_WP_GAIN * L + l] = nw_f64(nw->wp_gain, (int64_t)l, 1.0);
        degree[(size_t)sorted_of_node[(size_t)a]]++;
        if (b >= 0) degree[(size_t)sorted_of_node[(size_t)b]]++;
    }
    int32_t first = 0;
    for (size_t p = 0; p < N; p++) {
        DI[ND_INC0 * N + p] = first, DI[ND_INC_N * N + p] = 0;
        first += degree[p];
    }
    t.inc.assign((size_t)first, -1);
    for (size_t l = 0; l < L; l++) {
        const int32_t zb = nw->zone_b[l];
        const int32_t ends[2] = {node_of_zone[(size_t)nw->zone_a[l]], zb >= 0 ? node_of_zone[(size_t)zb] : -1};
        for (int a = 0; a < 2; a++) {
            if (ends[a] < 0) continue;
            const size_t p = (size_t)sorted_of_node[(size_t)ends[a]];
            t.inc[(size_t)DI[ND_INC0 * N + p] + (size_t)DI[ND_INC_N * N + p]++] = (int32_t)l;
        }
    }
}

int check_network_tables(int64_t n_zones, int32_t n_channels, const heat_air_networks *nw, const NetworkTables &t, std::string &err) {
    const size_t W = nw ? (size_t)nw->n_networks : 0, N = nw ? (size_t)nw->n_nodes : 0, L = nw ? (size_t)nw->n_links : 0;
    if (t.n_networks != (int64_t)W || t.n_nodes != (int64_t)N || t.n_links != (int64_t)L || t.net_i32.size() != (size_t)kNetworkNetI32Rows * W ||
        t.net_f64.size() != (size_t)kNetworkNetF64Rows * W || t.node_i32.size() != (size_t)kNetworkNodeI32Rows * N || t.node_f64.size() != N ||
        t.link_i32.size() != (size_t)kNetworkLinkI32Rows * L || t.link_f64.size() != (size_t)kNetworkLinkF64Rows * L)
        return failp(err, HEAT_E_SIZE, "network tables: their sizes are not those of %zu networks, %zu nodes and %zu links", W, N, L);
    if (W == 0) return HEAT_OK;
    if (t.class_start[0] != 0 || t.class_start[kNetworkClasses] != (int32_t)W)
        return failp(err, HEAT_E_SIZE, "network tables: the classes hold [%d, %d), not the %zu networks", t.class_start[0], t.class_start[kNetworkClasses], W);
    std::vector<uint8_t> seen_net(W, 0), seen_node(N, 0);
    int64_t at = 0;
    for (int c = 0; c < kNetworkClasses; c++) {
        if (t.class_start[c + 1] < t.class_start[c]) return failp(err, HEAT_E_SIZE, "network tables: class %d ends before it starts", c);
        for (int32_t s = t.class_start[c]; s < t.class_start[c + 1]; s++) {
            const int32_t w = t.net(NW_ID)[s], n = t.net(NW_N)[s];
            if (w < 0 || (size_t)w >= W || seen_net[(size_t)w]++) return failp(err, HEAT_E_SIZE, "network tables: network %d is listed twice or is none", w);
            if (n != nw->net_offset[w + 1] - nw->net_offset[w] || n < 1 || n > (8 << c) || (c > 0 && n <= (4 << c)))
                return failp(err, HEAT_E_SIZE, "network tables: network %d: %d nodes in the class of %d lanes", w, n, 8 << c);
            if (t.net(NW_NODE0)[s] != at || at + n > (int64_t)N) return failp(err, HEAT_E_SIZE, "network tables: network %d: its nodes are not behind the last", w);
            if (t.net(NW_MAX_ITER)[s] != nw->max_iter[w] || t.net(NW_MAX_ITER)[s] < 1 || t.net(NW_MAX_ITER)[s] > kNetworkMaxNodes ||
                std::memcmp(&t.net_f64[NW_TOL * W + (size_t)s], &nw->tol[w], sizeof(double)) != 0 ||
                std::memcmp(&t.net_f64[NW_G_MIN * W + (size_t)s], &nw->g_min[w], sizeof(double)) != 0)
                return failp(err, HEAT_E_SIZE, "network tables: network %d: tol, max_iter or g_min is not the caller's", w);
            for (int32_t i = 0; i < n; i++) {
                const size_t p = (size_t)(at + i);
                const int32_t id = t.node(ND_ID)[p], sc = t.node(ND_SRC_CHAN)[p];
                if (id != nw->net_offset[w] + i || seen_node[(size_t)id]++) return failp(err, HEAT_E_SIZE, "network tables: node %d is not in its network's place", id);
                if (t.node(ND_ZONE)[p] != nw->node_zone[id] || (int64_t)(uint32_t)t.node(ND_ZONE)[p] >= n_zones || sc != ct_i32(nw->src_chan, id, -1) ||
                    sc < -1 || sc >= n_channels)
                    return failp(err, HEAT_E_SIZE, "network tables: node %d: its zone or source channel is not the caller's or lies outside its array", id);
                const int32_t i0 = t.node(ND_INC0)[p], in = t.node(ND_INC_N)[p];
                if (i0 < 0 || in < 0 || (size_t)i0 + (size_t)in > t.inc.size()) return failp(err, HEAT_E_SIZE, "network tables: node %d: its links lie outside the list", id);
                for (int32_t e = 0; e < in; e++) {
                    const int32_t l = t.inc[(size_t)(i0 + e)];
                    if (l < 0 || (size_t)l >= L || (e > 0 && l <= t.inc[(size_t)(i0 + e - 1)]))
                        return failp(err, HEAT_E_SIZE, "network tables: node %d: its links are not ascending links", id);
                    if (t.link(LK_ZONE_A)[l] != nw->node_zone[id] && t.link(LK_ZONE_B)[l] != nw->node_zone[id])
                        return failp(err, HEAT_E_SIZE, "network tables: node %d: link %d does not touch it", id, l);
                    if ((t.link(LK_ZONE_A)[l] == nw->node_zone[id] ? t.link(LK_LA)[l] : t.link(LK_LB)[l]) != i)
                        return failp(err, HEAT_E_SIZE, "network tables: node %d: link %d names it by another local number", id, l);
                }
            }
            at += n;
        }
    }
    size_t ends = 0;
    for (size_t l = 0; l < L; l++) {
        const int32_t za = t.link(LK_ZONE_A)[l], zb = t.link(LK_ZONE_B)[l], la = t.link(LK_LA)[l], lb = t.link(LK_LB)[l];
        if (za != nw->zone_a[l] || zb != nw->zone_b[l] || (int64_t)(uint32_t)za >= n_zones || zb < -1 || zb >= n_zones || la < 0 ||
            la >= kNetworkMaxNodes || lb < -1 || lb >= kNetworkMaxNodes || (lb < 0) != (zb < 0))
            return failp(err, HEAT_E_SIZE, "network tables: link %zu: a zone or a local node number is not the caller's or lies outside its array", l);
        static const int chan_row[5] = {LK_TEMP_CHAN, LK_WP_CHAN, LK_FRAC_CHAN, LK_OUT_AB, LK_OUT_BA};
        for (int a = 0; a < 5; a++)
            if (t.link(chan_row[a])[l] < -1 || t.link(chan_row[a])[l] >= n_channels || (a == 0 && zb < 0 && t.link(chan_row[a])[l] < 0))
                return failp(err, HEAT_E_SIZE, "network tables: link %zu: a channel lies outside the row", l);
        const double s_lin = std::sqrt(nw->p_lin[l]);
        if (std::memcmp(&t.link_real(LK_C)[l], &nw->c[l], sizeof(double)) != 0 || std::memcmp(&t.link_real(LK_S_LIN)[l], &s_lin, sizeof(double)) != 0)
            return failp(err, HEAT_E_SIZE, "network tables: link %zu: c or sqrt(p_lin) is not the caller's", l);
        ends += zb >= 0 ? 2 : 1;
    }
    if (ends != t.inc.size()) return failp(err, HEAT_E_SIZE, "network tables: %zu incidences for %zu link ends", t.inc.size(), ends);
    return HEAT_OK;
}

// ---- ideal loads of a series (include/heat_amd.h, heat_ideal_loads) ----
int check_ideal_loads(int64_t n_zones, int32_t n_channels, const heat_ideal_loads *il, std::string &err,
                      std::vector<int32_t> *load_of_zone) {
    if (load_of_zone) load_of_zone->assign((size_t)std::max<int64_t>(n_zones, 0), -1);
    if (!il) return HEAT_OK;
    if (il->n_loads < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count in ideal loads (n_loads %lld)", (long long)il->n_loads);
    // (the table numbers the loads with 32 bits)
    if (il->n_loads > INT32_MAX) return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 ideal loads (n_loads %lld)", (long long)il->n_loads);
    if (il->n_loads > 0 && (!il->zone || !il->heat_chan || !il->cool_chan))
        return failp(err, HEAT_E_INVALID_ARG, "ideal loads: zone, heat_chan or cool_chan is NULL");
    if ((il->step_peak_heating && !il->peak_heating) || (il->step_peak_cooling && !il->peak_cooling))
        return failp(err, HEAT_E_INVALID_ARG, "ideal loads: step_peak_heating / step_peak_cooling without peak_heating / peak_cooling");
    std::vector<int32_t> local;
    std::vector<int32_t> &of = load_of_zone ? *load_of_zone : local;
    if (!load_of_zone) of.assign((size_t)std::max<int64_t>(n_zones, 0), -1);
    for (int64_t i = 0; i < il->n_loads; i++) {
        const int32_t z = il->zone[i], hc = il->heat_chan[i], cc = il->cool_chan[i];
        if (z < 0 || z >= n_zones)
            return failp(err, HEAT_E_SIZE, "ideal load %lld: zone %d outside [0, %lld)", (long long)i, z, (long long)n_zones);
        if (hc != -1 && (hc < 0 || hc >= n_channels))
            return failp(err, HEAT_E_SIZE, "ideal load %lld: heating setpoint channel %d outside [-1, %d)", (long long)i, hc, n_channels);
        if (cc != -1 && (cc < 0 || cc >= n_channels))
            return failp(err, HEAT_E_SIZE, "ideal load %lld: cooling setpoint channel %d outside [-1, %d)", (long long)i, cc, n_channels);
        if (hc == -1 && cc == -1)
            return failp(err, HEAT_E_SIZE, "ideal load %lld: neither a heating nor a cooling setpoint channel", (long long)i);
        const double *cap[2] = {il->heat_cap, il->cool_cap};
        for (int a = 0; a < 2; a++)
            if (cap[a] && !(cap[a][i] >= 0.0))  // (+inf passes: unlimited)
                return failp(err, HEAT_E_INVALID_ARG, "ideal load %lld: %s capacity %g is negative or NaN", (long long)i,
                             a ? "cooling" : "heating", cap[a][i]);
        if (of[(size_t)z] >= 0)
            return failp(err, HEAT_E_INVALID_ARG, "ideal load %lld: zone %d already has ideal load %d", (long long)i, z, of[(size_t)z]);
        of[(size_t)z] = (int32_t)i;
    }
    return HEAT_OK;
}

// ---- sky of a series (include/heat_amd.h, heat_sky) ----
int check_sky(int64_t n_surfaces, const heat_series *s, const heat_sky *sky, std::string &err, unsigned *any_bits) {
    if (any_bits) *any_bits = 0;
    if (!sky) return HEAT_OK;
    if (!sky->mode) return failp(err, HEAT_E_INVALID_ARG, "sky: mode is NULL (one byte per surface s, 0: the surface takes nothing from the sky)");
    // (the mode bits number the inputs as the series does)
    const int32_t *chan_of_bit[4] = {s->solar_front_chan, s->solar_back_chan, s->ir_front_chan, s->ir_back_chan};
    static const char *const input_name[4] = {"solar front", "solar back", "long-wave front", "long-wave back"};
    const double *normal[3] = {sky->normal_x, sky->normal_y, sky->normal_z};
    unsigned any = 0;
    for (int64_t q = 0; q < n_surfaces; q++) {
        const unsigned m = sky->mode[q];
        if (m > 15) return failp(err, HEAT_E_INVALID_ARG, "surface %lld: sky mode %u above 15 (bits 0-3)", (long long)q, m);
        if (m == 0) continue;
        any |= m;
        for (int a = 0; a < 3; a++) {
            if (!normal[a]) return failp(err, HEAT_E_INVALID_ARG, "surface %lld: sky mode %u, but normal_%c is NULL", (long long)q, m, "xyz"[a]);
            if (!std::isfinite(normal[a][q]))
                return failp(err, HEAT_E_INVALID_ARG, "surface %lld: sky mode %u, but normal_%c = %g is not finite", (long long)q, m, "xyz"[a],
                             normal[a][q]);
        }
        if (!sky->record && s->n_steps > 0)
            return failp(err, HEAT_E_INVALID_ARG, "surface %lld: sky mode %u, but record is NULL (n_steps %d)", (long long)q, m, s->n_steps);
        for (int a = 0; a < 4; a++)
            if ((m >> a & 1) && chan_of_bit[a] && chan_of_bit[a][q] >= 0)
                return failp(err, HEAT_E_SIZE, "surface %lld: its %s input is driven by the sky (mode bit %d) and by channel %d: an input has one source",
                             (long long)q, input_name[a], a, chan_of_bit[a][q]);
    }
    if (any_bits) *any_bits = any;
    return HEAT_OK;
}

// ---- the one-struct call of a series (include/heat_amd.h, heat_series_call) ----
int check_series_call(const heat_series_call *call, std::string &err) {
    if (!call) return failp(err, HEAT_E_INVALID_ARG, "series call is NULL");
    if (call->size != sizeof(heat_series_call))
        return failp(err, HEAT_E_INVALID_ARG, "series call: size %zu is not sizeof(heat_series_call) = %zu of this library", call->size,
                     sizeof(heat_series_call));
    if (!call->s) return failp(err, HEAT_E_INVALID_ARG, "series call: s is NULL");
    return HEAT_OK;
}

// ---- anisotropic sky of a series (include/heat_amd.h, heat_sky_aniso) ----
int check_sky_aniso(int64_t n_surfaces, const heat_series *s, const heat_sky *sky, const heat_solar_gains *g, const heat_shades *sh,
                    const heat_sky_aniso *an, std::string &err) {
    if (!an) return HEAT_OK;
    if (!sky || !sky->record)
        return failp(err, HEAT_E_INVALID_ARG, "sky aniso: the coefficients stand beside the sky records, but %s is NULL", sky ? "sky->record" : "sky");
    if (!an->coef && s->n_steps > 0) return failp(err, HEAT_E_INVALID_ARG, "sky aniso: coef is NULL (n_steps %d)", s->n_steps);
    if (an->aperture_band && !g) return failp(err, HEAT_E_INVALID_ARG, "sky aniso: aperture_band without solar gains: no aperture a reads it");
    if (an->shade_band && !sh) return failp(err, HEAT_E_INVALID_ARG, "sky aniso: shade_band without shades: no shade j reads it");
    const double *side_band[2] = {an->front_band, an->back_band};
    for (int side = 0; side < 2; side++)
        for (int64_t q = 0; q < n_surfaces && side_band[side] && sky->mode; q++)
            if ((sky->mode[q] >> side & 1) && !(side_band[side][q] >= 0.0 && std::isfinite(side_band[side][q])))
                return failp(err, HEAT_E_INVALID_ARG, "surface %lld: %s_band = %g is negative or not finite", (long long)q, side ? "back" : "front",
                             side_band[side][q]);
    for (int64_t a = 0; an->aperture_band && a < g->n_apertures; a++)
        if (!(an->aperture_band[a] >= 0.0 && std::isfinite(an->aperture_band[a])))
            return failp(err, HEAT_E_INVALID_ARG, "aperture %lld: aperture_band = %g is negative or not finite", (long long)a, an->aperture_band[a]);
    for (int64_t j = 0; an->shade_band && j < sh->n_shades; j++)
        if (!(an->shade_band[j] >= 0.0 && std::isfinite(an->shade_band[j])))
            return failp(err, HEAT_E_INVALID_ARG, "shade %lld: shade_band = %g is negative or not finite", (long long)j, an->shade_band[j]);
    return HEAT_OK;
}

// ---- solar gains of a series (include/heat_amd.h, heat_solar_gains) ----
int check_solar_gains(int64_t n_surfaces, const heat_series *s, const heat_sky *sky, const heat_solar_gains *g, std::string &err) {
    if (!g) return HEAT_OK;
    const int64_t NA = g->n_apertures, NE = g->n_entries;
    if (NA < 0 || NE < 0)
        return failp(err, HEAT_E_INVALID_ARG, "negative count in solar gains (n_apertures %lld, n_entries %lld): no aperture a, no entry i",
                     (long long)NA, (long long)NE);
    if (NA > INT32_MAX || NE > INT32_MAX)
        return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 in solar gains (n_apertures %lld, n_entries %lld): aperture a and entry i are 32-bit",
                     (long long)NA, (long long)NE);
    if (NA > 0) {
        const void *need[7] = {g->ap_surface, g->ap_normal_x, g->ap_normal_y, g->ap_normal_z, g->ap_tau_coef, g->ap_tau_diffuse, g->ap_scale};
        static const char *const name[7] = {"ap_surface", "ap_normal_x", "ap_normal_y", "ap_normal_z", "ap_tau_coef", "ap_tau_diffuse", "ap_scale"};
        for (int a = 0; a < 7; a++)
            if (!need[a]) return failp(err, HEAT_E_INVALID_ARG, "aperture 0: %s is NULL (n_apertures %lld)", name[a], (long long)NA);
        if (s->n_steps > 0 && (!sky || !sky->record))
            return failp(err, HEAT_E_INVALID_ARG, "aperture 0: its site's record is read, but %s is NULL (n_steps %d)", sky ? "sky->record" : "sky",
                         s->n_steps);
    }
    if (NE > 0) {
        const void *need[5] = {g->en_surface, g->en_side, g->en_aperture, g->en_beam, g->en_diffuse};
        static const char *const name[5] = {"en_surface", "en_side", "en_aperture", "en_beam", "en_diffuse"};
        for (int a = 0; a < 5; a++)
            if (!need[a]) return failp(err, HEAT_E_INVALID_ARG, "entry 0: %s is NULL (n_entries %lld)", name[a], (long long)NE);
    }
    for (int64_t a = 0; a < NA; a++) {
        if (g->ap_surface[a] < 0 || g->ap_surface[a] >= n_surfaces)
            return failp(err, HEAT_E_SIZE, "aperture %lld: surface %lld outside [0, %lld)", (long long)a, (long long)g->ap_surface[a], (long long)n_surfaces);
        const double v[5] = {g->ap_normal_x[a], g->ap_normal_y[a], g->ap_normal_z[a], g->ap_tau_diffuse[a], g->ap_scale[a]};
        static const char *const name[5] = {"normal_x", "normal_y", "normal_z", "tau_diffuse", "scale"};
        for (int j = 0; j < 5; j++)
            if (!std::isfinite(v[j])) return failp(err, HEAT_E_INVALID_ARG, "aperture %lld: %s = %g is not finite", (long long)a, name[j], v[j]);
        for (int j = 0; j < 6; j++)
            if (!std::isfinite(g->ap_tau_coef[6 * a + j]))
                return failp(err, HEAT_E_INVALID_ARG, "aperture %lld: tau_coef[%d] = %g is not finite", (long long)a, j, g->ap_tau_coef[6 * a + j]);
    }
    const int32_t *chan[2] = {s->solar_front_chan, s->solar_back_chan};
    for (int64_t i = 0; i < NE; i++) {
        const int64_t q = g->en_surface[i];
        const unsigned side = g->en_side[i];
        if (side > 1) return failp(err, HEAT_E_INVALID_ARG, "entry %lld: side %u above 1 (0 front, 1 back)", (long long)i, side);
        if (!std::isfinite(g->en_beam[i]) || !std::isfinite(g->en_diffuse[i]))
            return failp(err, HEAT_E_INVALID_ARG, "entry %lld: shares beam = %g, diffuse = %g are not finite", (long long)i, g->en_beam[i],
                         g->en_diffuse[i]);
        if (q < 0 || q >= n_surfaces)
            return failp(err, HEAT_E_SIZE, "entry %lld: surface %lld outside [0, %lld)", (long long)i, (long long)q, (long long)n_surfaces);
        if (g->en_aperture[i] < 0 || g->en_aperture[i] >= NA)
            return failp(err, HEAT_E_SIZE, "entry %lld: aperture %d outside [0, %lld)", (long long)i, g->en_aperture[i], (long long)NA);
        if (chan[side] && chan[side][q] >= 0)
            return failp(err, HEAT_E_SIZE, "entry %lld: the solar %s input of surface %lld is driven by channel %d already: an input has one source",
                         (long long)i, side ? "back" : "front", (long long)q, chan[side][q]);
        if (sky && sky->mode && (sky->mode[q] >> side & 1))
            return failp(err, HEAT_E_SIZE, "entry %lld: the solar %s input of surface %lld is driven by the sky (mode bit %u) already: an input has one source",
                         (long long)i, side ? "back" : "front", (long long)q, side);
    }
    return HEAT_OK;
}

// ---- shades of a series (include/heat_amd.h, heat_shades) ----
namespace {
struct ShadeColumn {
    const double *v;
    const char *name;
    int rule;  // 0: finite, 1: finite and > 0, 2: finite and >= 0
};
}  // namespace

int check_shades(int64_t n_surfaces, const heat_series *s, const heat_sky *sky, const heat_solar_gains *g, const heat_shades *sh,
                 std::string &err) {
    if (!sh) return HEAT_OK;
    const int64_t NS = sh->n_shades, NH = sh->n_horizons;
    if (NS < 0 || NH < 0)
        return failp(err, HEAT_E_INVALID_ARG, "negative count in shades (n_shades %lld, n_horizons %lld): no shade j, no horizon p", (long long)NS,
                     (long long)NH);
    if (NS > INT32_MAX || NH > INT32_MAX)
        return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 in shades (n_shades %lld, n_horizons %lld): shade j and horizon p are 32-bit",
                     (long long)NS, (long long)NH);
    const ShadeColumn col[17] = {{sh->sh_normal_x, "sh_normal_x", 0}, {sh->sh_normal_y, "sh_normal_y", 0}, {sh->sh_normal_z, "sh_normal_z", 0},
                                 {sh->sh_right_x, "sh_right_x", 0},   {sh->sh_right_y, "sh_right_y", 0},   {sh->sh_right_z, "sh_right_z", 0},
                                 {sh->sh_up_x, "sh_up_x", 0},         {sh->sh_up_y, "sh_up_y", 0},         {sh->sh_up_z, "sh_up_z", 0},
                                 {sh->sh_width, "sh_width", 1},       {sh->sh_height, "sh_height", 1},
                                 {sh->overhang_depth, "overhang_depth", 2}, {sh->overhang_gap, "overhang_gap", 2},
                                 {sh->fin_pos_depth, "fin_pos_depth", 2},   {sh->fin_pos_gap, "fin_pos_gap", 2},
                                 {sh->fin_neg_depth, "fin_neg_depth", 2},   {sh->fin_neg_gap, "fin_neg_gap", 2}};
    const ShadeColumn factor[2] = {{sh->diffuse_factor, "diffuse_factor", 0}, {sh->ground_factor, "ground_factor", 0}};
    if (NS > 0) {
        if (!sh->sh_surface) return failp(err, HEAT_E_INVALID_ARG, "shade 0: sh_surface is NULL (n_shades %lld)", (long long)NS);
        for (const ShadeColumn &c : col)
            if (!c.v) return failp(err, HEAT_E_INVALID_ARG, "shade 0: %s is NULL (n_shades %lld)", c.name, (long long)NS);
        if (s->n_steps > 0 && (!sky || !sky->record))
            return failp(err, HEAT_E_INVALID_ARG, "shade 0: its site's record is read, but %s is NULL (n_steps %d)", sky ? "sky->record" : "sky",
                         s->n_steps);
    }
    if (NH > 0 && !sh->horizon_tan2) return failp(err, HEAT_E_INVALID_ARG, "horizon 0: horizon_tan2 is NULL (n_horizons %lld)", (long long)NH);
    for (int64_t p = 0; p < NH; p++)
        for (int q = 0; q < 16; q++) {
            const double t = sh->horizon_tan2[16 * p + q];
            if (!std::isfinite(t) || t < 0.0)
                return failp(err, HEAT_E_INVALID_ARG, "horizon %lld: tan2[%d] = %g is %s", (long long)p, q, t, std::isfinite(t) ? "negative" : "not finite");
        }
    for (int64_t j = 0; j < NS; j++) {
        for (const ShadeColumn &c : col) {
            const double v = c.v[j];
            if (!std::isfinite(v)) return failp(err, HEAT_E_INVALID_ARG, "shade %lld: %s = %g is not finite", (long long)j, c.name, v);
            if (c.rule == 1 && !(v > 0.0)) return failp(err, HEAT_E_INVALID_ARG, "shade %lld: %s = %g is not positive", (long long)j, c.name, v);
            if (c.rule == 2 && v < 0.0) return failp(err, HEAT_E_INVALID_ARG, "shade %lld: %s = %g is negative", (long long)j, c.name, v);
        }
        for (const ShadeColumn &c : factor)
            if (c.v && !std::isfinite(c.v[j]))
                return failp(err, HEAT_E_INVALID_ARG, "shade %lld: %s = %g is not finite", (long long)j, c.name, c.v[j]);
        if (sh->sh_surface[j] < 0 || sh->sh_surface[j] >= n_surfaces)
            return failp(err, HEAT_E_SIZE, "shade %lld: surface %lld outside [0, %lld)", (long long)j, (long long)sh->sh_surface[j],
                         (long long)n_surfaces);
        if (sh->sh_horizon && (sh->sh_horizon[j] < -1 || sh->sh_horizon[j] >= NH))
            return failp(err, HEAT_E_SIZE, "shade %lld: horizon %d outside [-1, %lld)", (long long)j, sh->sh_horizon[j], (long long)NH);
    }
    const int32_t *side_shade[2] = {sh->front_shade, sh->back_shade};
    for (int side = 0; side < 2; side++) {
        if (!side_shade[side]) continue;
        for (int64_t q = 0; q < n_surfaces; q++) {
            const int32_t j = side_shade[side][q];
            if (j == -1) continue;
            if (j < -1 || j >= NS)
                return failp(err, HEAT_E_SIZE, "surface %lld: %s shade %d outside [-1, %lld)", (long long)q, side ? "back" : "front", j, (long long)NS);
            if (!sky || !sky->mode || !(sky->mode[q] >> side & 1))
                return failp(err, HEAT_E_SIZE, "surface %lld: %s shade %d, but the solar %s input is not driven by the sky (mode bit %d is not set)",
                             (long long)q, side ? "back" : "front", j, side ? "back" : "front", side);
        }
    }
    if (sh->aperture_shade) {
        if (!g) return failp(err, HEAT_E_INVALID_ARG, "aperture 0: aperture_shade without solar gains (gains is NULL)");
        for (int64_t a = 0; a < g->n_apertures; a++) {
            const int32_t j = sh->aperture_shade[a];
            if (j < -1 || j >= NS)
                return failp(err, HEAT_E_SIZE, "aperture %lld: shade %d outside [-1, %lld)", (long long)a, j, (long long)NS);
        }
    }
    return HEAT_OK;
}

void build_shade_tables(const heat_shades *sh, ShadeTables &t) {
    t.f64.clear();
    t.horizon.clear();
    const int64_t NS = sh ? sh->n_shades : 0;
    if (NS <= 0) return;
    const double *row[kShadeRows] = {sh->sh_normal_x, sh->sh_normal_y, sh->sh_normal_z, sh->sh_right_x, sh->sh_right_y, sh->sh_right_z,
                                     sh->sh_up_x, sh->sh_up_y, sh->sh_up_z, sh->sh_width, sh->sh_height, sh->overhang_depth,
                                     sh->overhang_gap, sh->fin_pos_depth, sh->fin_pos_gap, sh->fin_neg_depth, sh->fin_neg_gap,
                                     sh->diffuse_factor, sh->ground_factor};
    t.f64.assign((size_t)kShadeRows * NS, 1.0);
    for (int a = 0; a < kShadeRows; a++)
        if (row[a]) std::copy(row[a], row[a] + NS, t.f64.begin() + (size_t)a * NS);
    t.horizon.assign((size_t)NS, -1);
    if (sh->sh_horizon) std::copy(sh->sh_horizon, sh->sh_horizon + NS, t.horizon.begin());
}

// ---- blinds of a series (include/heat_amd.h, heat_blinds) ----
int check_blinds(int64_t n_zones, const heat_series *s, const heat_shades *sh, const heat_blinds *bl, std::string &err) {
    if (!bl) return HEAT_OK;
    const int64_t N = bl->n_blinds, NS = sh ? sh->n_shades : 0;
    if (N < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count of blinds (n_blinds %lld): no blind i", (long long)N);
    if (N == 0) return HEAT_OK;
    if (NS <= 0)
        return failp(err, HEAT_E_INVALID_ARG, "blind 0: a blind rides on a shade, but there are no shades (%s, n_blinds %lld)",
                     sh ? "n_shades is 0" : "shades is NULL", (long long)N);
    if (!bl->shade) return failp(err, HEAT_E_INVALID_ARG, "blind 0: shade is NULL (n_blinds %lld)", (long long)N);
    const double *const closed[3] = {bl->beam_closed, bl->diffuse_closed, bl->ground_closed};
    static const char *const closed_name[3] = {"beam_closed", "diffuse_closed", "ground_closed"};
    for (int a = 0; a < 3; a++)
        if (!closed[a]) return failp(err, HEAT_E_INVALID_ARG, "blind 0: %s is NULL (n_blinds %lld)", closed_name[a], (long long)N);
    const int32_t NC = s->n_channels;
    std::vector<uint8_t> taken((size_t)NS, 0);
    for (int64_t i = 0; i < N; i++) {
        const int32_t j = bl->shade[i], pc = bl->pos_chan ? bl->pos_chan[i] : -1, z = bl->zone ? bl->zone[i] : -1;
        const int32_t ec = bl->enable_chan ? bl->enable_chan[i] : -1;
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(closed[a][i]) || closed[a][i] < 0.0)
                return failp(err, HEAT_E_INVALID_ARG, "blind %lld: %s = %g is negative or not finite", (long long)i, closed_name[a], closed[a][i]);
        if (bl->state && bl->state[i] > 1)
            return failp(err, HEAT_E_INVALID_ARG, "blind %lld: state %d is neither 0 (open) nor 1 (closed)", (long long)i, (int)bl->state[i]);
        if (j < 0 || j >= NS) return failp(err, HEAT_E_SIZE, "blind %lld: shade %d outside [0, %lld)", (long long)i, j, (long long)NS);
        if (taken[(size_t)j]) return failp(err, HEAT_E_SIZE, "blind %lld: shade %d carries a blind already (at most one blind per shade)", (long long)i, j);
        taken[(size_t)j] = 1;
        if (pc < -1 || pc >= NC) return failp(err, HEAT_E_SIZE, "blind %lld: position channel %d outside [-1, %d)", (long long)i, pc, NC);
        if (ec < -1 || ec >= NC) return failp(err, HEAT_E_SIZE, "blind %lld: enable channel %d outside [-1, %d)", (long long)i, ec, NC);
        if (z < -1 || z >= n_zones) return failp(err, HEAT_E_SIZE, "blind %lld: zone %d outside [-1, %lld)", (long long)i, z, (long long)n_zones);
        if (pc < 0) {  // (controlled; the thresholds of a scheduled blind are not read)
            if (!bl->irr_close || !bl->irr_open)
                return failp(err, HEAT_E_INVALID_ARG, "blind %lld: controlled (no position channel), but %s is NULL", (long long)i,
                             !bl->irr_close ? "irr_close" : "irr_open");
            if (!std::isfinite(bl->irr_close[i]) || !std::isfinite(bl->irr_open[i]))
                return failp(err, HEAT_E_INVALID_ARG, "blind %lld: irr_close = %g / irr_open = %g is not finite", (long long)i, bl->irr_close[i],
                             bl->irr_open[i]);
            if (bl->irr_open[i] > bl->irr_close[i])
                return failp(err, HEAT_E_INVALID_ARG, "blind %lld: irr_open = %g is above irr_close = %g", (long long)i, bl->irr_open[i],
                             bl->irr_close[i]);
        }
        if (z < 0) continue;  // (no room condition: setpoint channel and band are not read)
        if (!bl->set_chan || !bl->band)
            return failp(err, HEAT_E_INVALID_ARG, "blind %lld: gated by zone %d, but %s is NULL", (long long)i, z, !bl->set_chan ? "set_chan" : "band");
        if (!std::isfinite(bl->band[i]) || bl->band[i] < 0.0)
            return failp(err, HEAT_E_INVALID_ARG, "blind %lld: band = %g is negative or not finite", (long long)i, bl->band[i]);
        if (bl->set_chan[i] < 0 || bl->set_chan[i] >= NC)
            return failp(err, HEAT_E_SIZE, "blind %lld: setpoint channel %d outside [0, %d)", (long long)i, bl->set_chan[i], NC);
    }
    return HEAT_OK;
}

void build_blind_tables(int64_t n_shades, const heat_blinds *bl, BlindTables &t) {
    t = BlindTables();
    const size_t N = bl && bl->n_blinds > 0 ? (size_t)bl->n_blinds : 0;
    if (N == 0) return;
    t.blind_of_shade.assign((size_t)n_shades, -1);
    t.i32.assign(kBlindI32Rows * N, -1);
    t.f64.assign(kBlindF64Rows * N, 0.0);
    for (size_t i = 0; i < N; i++) {
        t.blind_of_shade[(size_t)bl->shade[i]] = (int32_t)i;
        const int32_t pc = bl->pos_chan ? bl->pos_chan[i] : -1;
        const int32_t z = pc < 0 && bl->zone ? bl->zone[i] : -1;
        t.i32[BL_POS_CHAN * N + i] = pc;
        t.i32[BL_ZONE * N + i] = z;
        t.i32[BL_SET_CHAN * N + i] = z >= 0 ? bl->set_chan[i] : -1;
        t.i32[BL_ENABLE_CHAN * N + i] = pc < 0 && bl->enable_chan ? bl->enable_chan[i] : -1;
        t.f64[BL_BEAM * N + i] = bl->beam_closed[i];
        t.f64[BL_DIFFUSE * N + i] = bl->diffuse_closed[i];
        t.f64[BL_GROUND * N + i] = bl->ground_closed[i];
        t.f64[BL_IRR_CLOSE * N + i] = pc < 0 ? bl->irr_close[i] : 0.0;
        t.f64[BL_IRR_OPEN * N + i] = pc < 0 ? bl->irr_open[i] : 0.0;
        t.f64[BL_HALF_BAND * N + i] = z >= 0 ? bl->band[i] / 2.0 : 0.0;
    }
}

int check_blind_tables(int64_t n_shades, const heat_blinds *bl, const BlindTables &t, std::string &err) {
    const size_t N = bl && bl->n_blinds > 0 ? (size_t)bl->n_blinds : 0, NS = N ? (size_t)n_shades : 0;
    if (t.blind_of_shade.size() != NS || t.i32.size() != kBlindI32Rows * N || t.f64.size() != kBlindF64Rows * N)
        return failp(err, HEAT_E_SIZE, "blind tables: %zu shades, %zu integers and %zu reals for blind i < %zu on %zu shades",
                     t.blind_of_shade.size(), t.i32.size(), t.f64.size(), N, NS);
    size_t carried = 0;
    for (size_t j = 0; j < NS; j++) {
        const int32_t i = t.blind_of_shade[j];
        if (i == -1) continue;
        if (i < 0 || (size_t)i >= N || bl->shade[i] != (int32_t)j)
            return failp(err, HEAT_E_SIZE, "blind tables: shade %zu carries blind %d, which is not on it", j, i);
        carried++;
    }
    if (carried != N) return failp(err, HEAT_E_SIZE, "blind tables: %zu shades carry a blind i, of %zu blinds", carried, N);
    for (size_t i = 0; i < N; i++) {
        const int32_t pc = t.i32[BL_POS_CHAN * N + i], z = t.i32[BL_ZONE * N + i];
        const bool same = pc == (bl->pos_chan ? bl->pos_chan[i] : -1) && t.f64[BL_BEAM * N + i] == bl->beam_closed[i] &&
                          t.f64[BL_DIFFUSE * N + i] == bl->diffuse_closed[i] && t.f64[BL_GROUND * N + i] == bl->ground_closed[i] &&
                          (pc >= 0 || (z == (bl->zone ? bl->zone[i] : -1) && t.f64[BL_IRR_CLOSE * N + i] == bl->irr_close[i] &&
                                       t.f64[BL_IRR_OPEN * N + i] == bl->irr_open[i] &&
                                       t.i32[BL_ENABLE_CHAN * N + i] == (bl->enable_chan ? bl->enable_chan[i] : -1))) &&
                          (z < 0 || (t.i32[BL_SET_CHAN * N + i] == bl->set_chan[i] && t.f64[BL_HALF_BAND * N + i] == bl->band[i] / 2.0));
        if (!same) return failp(err, HEAT_E_SIZE, "blind tables: blind %zu is not the caller's", i);
    }
    return HEAT_OK;
}

// ---- comfort of a series (include/heat_amd.h, heat_comfort) ----
int check_comfort(int64_t n_surfaces, int64_t n_zones, const heat_series *s, const heat_comfort *c, std::string &err) {
    if (!c) return HEAT_OK;
    const int64_t N = c->n_sensors, E = c->n_entries;
    if (N < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count of comfort sensors (n_sensors %lld): no comfort sensor i", (long long)N);
    if (E < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count of comfort entries (n_entries %lld): no comfort entry j", (long long)E);
    // (the tables number sensors and entries with 32 bits)
    if (N > INT32_MAX || E > INT32_MAX)
        return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 comfort sensors i or comfort entries j (n_sensors %lld, n_entries %lld)",
                     (long long)N, (long long)E);
    if (N == 0) return HEAT_OK;  // (no sensor: the term is absent, whatever its entry list holds)
    if (!c->zone) return failp(err, HEAT_E_INVALID_ARG, "comfort sensor 0: zone is NULL (n_sensors %lld)", (long long)N);
    if ((c->step_min && !c->min_operative) || (c->step_max && !c->max_operative) || (c->step_max_above && !c->max_above))
        return failp(err, HEAT_E_INVALID_ARG, "comfort sensor 0: %s without %s: a step array records where its extremum was taken",
                     c->step_min && !c->min_operative ? "step_min" : (c->step_max && !c->max_operative ? "step_max" : "step_max_above"),
                     c->step_min && !c->min_operative ? "min_operative" : (c->step_max && !c->max_operative ? "max_operative" : "max_above"));
    const int32_t NC = s->n_channels;
    std::vector<uint8_t> controlled((size_t)std::max<int64_t>(n_zones, 0), 0);
    const int32_t *const chans[3] = {c->occ_chan, c->lo_chan, c->hi_chan};
    static const char *const chan_name[3] = {"occupancy", "lower limit", "upper limit"};
    for (int64_t i = 0; i < N; i++) {
        const int32_t z = c->zone[i];
        if (c->air_weight && !(std::isfinite(c->air_weight[i]) && c->air_weight[i] >= 0.0 && c->air_weight[i] <= 1.0))
            return failp(err, HEAT_E_INVALID_ARG, "comfort sensor %lld: air_weight = %g is not finite or outside [0, 1]", (long long)i, c->air_weight[i]);
        if (c->control && c->control[i] > 1)
            return failp(err, HEAT_E_INVALID_ARG, "comfort sensor %lld: control %d is neither 0 nor 1", (long long)i, (int)c->control[i]);
        if (z < 0 || z >= n_zones) return failp(err, HEAT_E_SIZE, "comfort sensor %lld: zone %d outside [0, %lld)", (long long)i, z, (long long)n_zones);
        for (int a = 0; a < 3; a++) {
            const int32_t ch = chans[a] ? chans[a][i] : -1;
            if (ch < -1 || ch >= NC)
                return failp(err, HEAT_E_SIZE, "comfort sensor %lld: %s channel %d outside [-1, %d)", (long long)i, chan_name[a], ch, NC);
        }
        if (c->control && c->control[i]) {
            if (controlled[(size_t)z])
                return failp(err, HEAT_E_SIZE, "comfort sensor %lld: zone %d has a control sensor already (at most one per zone)", (long long)i, z);
            controlled[(size_t)z] = 1;
        }
    }
    if (E == 0) return HEAT_OK;
    if (!c->en_sensor || !c->en_surface || !c->en_side || !c->en_weight)
        return failp(err, HEAT_E_INVALID_ARG, "comfort entry 0: %s is NULL (n_entries %lld)",
                     !c->en_sensor ? "en_sensor" : (!c->en_surface ? "en_surface" : (!c->en_side ? "en_side" : "en_weight")), (long long)E);
    for (int64_t j = 0; j < E; j++) {
        if (!std::isfinite(c->en_weight[j])) return failp(err, HEAT_E_INVALID_ARG, "comfort entry %lld: en_weight = %g is not finite", (long long)j, c->en_weight[j]);
        if (c->en_sensor[j] < 0 || c->en_sensor[j] >= N)
            return failp(err, HEAT_E_SIZE, "comfort entry %lld: sensor %d outside [0, %lld)", (long long)j, c->en_sensor[j], (long long)N);
        if (c->en_surface[j] < 0 || c->en_surface[j] >= n_surfaces)
            return failp(err, HEAT_E_SIZE, "comfort entry %lld: surface %lld outside [0, %lld)", (long long)j, (long long)c->en_surface[j], (long long)n_surfaces);
        if (c->en_side[j] > 1) return failp(err, HEAT_E_SIZE, "comfort entry %lld: side %d is neither 0 (first node) nor 1 (last node)", (long long)j, (int)c->en_side[j]);
    }
    return HEAT_OK;
}

void build_comfort_tables(int64_t n_zones, const heat_comfort *c, const int64_t *node_tile_base, const int32_t *node_geom,
                          const int64_t *first_node_slot, const int64_t *node_count, ComfortTables &t) {
    t = ComfortTables();
    const size_t N = c && c->n_sensors > 0 ? (size_t)c->n_sensors : 0, E = N ? (size_t)c->n_entries : 0;
    if (N == 0) return;
    t.off.assign(N + 1, 0);
    t.face.assign(E, 0);
    t.weight.assign(E, 0.0);
    t.orig.assign(E, -1);
    t.i32.assign(kComfortI32Rows * N, -1);
    t.air_weight.assign(N, 0.5);
    t.ctl_sensor.assign((size_t)n_zones, -1);
    // a counting sort by sensor: stable, so the caller's order survives inside a sensor
    for (size_t j = 0; j < E; j++) t.off[(size_t)c->en_sensor[j] + 1]++;
    for (size_t i = 0; i < N; i++) t.off[i + 1] += t.off[i];
    std::vector<int32_t> next(t.off.begin(), t.off.begin() + N);
    for (size_t j = 0; j < E; j++) {
        const size_t p = (size_t)next[(size_t)c->en_sensor[j]]++;
        const int64_t q = c->en_surface[j];
        const int node = c->en_side[j] ? (int)node_count[q] - 1 : 0;
        t.face[p] = (uint32_t)(node_tile_base ? node_slot_index(node_tile_base[q], node_geom[q], node) : first_node_slot[q] + node);
        t.weight[p] = c->en_weight[j];
        t.orig[p] = (int32_t)j;
    }
    for (size_t i = 0; i < N; i++) {
        t.i32[CF_ZONE * N + i] = c->zone[i];
        if (c->occ_chan) t.i32[CF_OCC_CHAN * N + i] = c->occ_chan[i];
        if (c->lo_chan) t.i32[CF_LO_CHAN * N + i] = c->lo_chan[i];
        if (c->hi_chan) t.i32[CF_HI_CHAN * N + i] = c->hi_chan[i];
        if (c->air_weight) t.air_weight[i] = c->air_weight[i];
        if (c->control && c->control[i]) t.ctl_sensor[(size_t)c->zone[i]] = (int32_t)i, t.any_control = true;
    }
}

int check_comfort_tables(int64_t n_zones, const heat_comfort *c, const ComfortTables &t, std::string &err) {
    const size_t N = c && c->n_sensors > 0 ? (size_t)c->n_sensors : 0, E = N ? (size_t)c->n_entries : 0, Z = N ? (size_t)n_zones : 0;
    if (t.off.size() != (N ? N + 1 : 0) || t.face.size() != E || t.weight.size() != E || t.orig.size() != E || t.i32.size() != kComfortI32Rows * N ||
        t.air_weight.size() != N || t.ctl_sensor.size() != Z)
        return failp(err, HEAT_E_SIZE, "comfort tables: %zu offsets, %zu faces, %zu weights, %zu rows and %zu zones for comfort sensor i < %zu, comfort entry j < %zu",
                     t.off.size(), t.face.size(), t.weight.size(), t.air_weight.size(), t.ctl_sensor.size(), N, E);
    if (N == 0) return HEAT_OK;
    if (t.off[0] != 0 || t.off[N] != (int32_t)E) return failp(err, HEAT_E_SIZE, "comfort tables: the offsets run from %d to %d for %zu entries", t.off[0], t.off[N], E);
    for (size_t i = 0; i < N; i++)
        if (t.off[i + 1] < t.off[i] || t.off[i + 1] > (int32_t)E)
            return failp(err, HEAT_E_SIZE, "comfort tables: comfort sensor %zu runs from %d to %d", i, t.off[i], t.off[i + 1]);
    // every entry of the caller's, in the caller's order, is the next element of its sensor's range ...
    std::vector<int32_t> cursor(t.off.begin(), t.off.begin() + N);
    for (size_t j = 0; j < E; j++) {
        const size_t i = (size_t)c->en_sensor[j];
        const int32_t p = cursor[i]++;
        if (p >= t.off[i + 1]) return failp(err, HEAT_E_SIZE, "comfort tables: comfort entry %zu: comfort sensor %zu has no room for it", j, i);
        if (t.orig[(size_t)p] != (int32_t)j || std::memcmp(&t.weight[(size_t)p], &c->en_weight[j], sizeof(double)) != 0)
            return failp(err, HEAT_E_SIZE, "comfort tables: comfort entry %zu is not element %d of comfort sensor %zu", j, p - t.off[i], i);
    }
    // ... and every range is full: with n_entries elements in all, each entry is present exactly once
    std::vector<int32_t> ctl(Z, -1);
    for (size_t i = 0; i < N; i++) {
        if (cursor[i] != t.off[i + 1]) return failp(err, HEAT_E_SIZE, "comfort tables: comfort sensor %zu holds %d entries of %d", i, cursor[i] - t.off[i], t.off[i + 1] - t.off[i]);
        const double a = c->air_weight ? c->air_weight[i] : 0.5;
        const bool same = t.i32[CF_ZONE * N + i] == c->zone[i] && t.i32[CF_OCC_CHAN * N + i] == (c->occ_chan ? c->occ_chan[i] : -1) &&
                          t.i32[CF_LO_CHAN * N + i] == (c->lo_chan ? c->lo_chan[i] : -1) && t.i32[CF_HI_CHAN * N + i] == (c->hi_chan ? c->hi_chan[i] : -1) &&
                          t.air_weight[i] == a;
        if (!same) return failp(err, HEAT_E_SIZE, "comfort tables: comfort sensor %zu is not the caller's", i);
        if (c->control && c->control[i]) ctl[(size_t)c->zone[i]] = (int32_t)i;
    }
    bool any = false;
    for (size_t z = 0; z < Z; z++) {
        if (ctl[z] != t.ctl_sensor[z]) return failp(err, HEAT_E_SIZE, "comfort tables: zone %zu is controlled by comfort sensor %d, not %d", z, t.ctl_sensor[z], ctl[z]);
        any = any || ctl[z] >= 0;
    }
    if (any != t.any_control) return failp(err, HEAT_E_SIZE, "comfort tables: any_control is %d with%s a control comfort sensor i", (int)t.any_control, any ? "" : "out");
    return HEAT_OK;
}

// ---- room radiation of a series (include/heat_amd.h, heat_room_radiation) ----
int check_room_radiation(int64_t n_surfaces, const heat_series *s, const heat_sky *sky, const heat_room_radiation *rr, std::string &err) {
    if (!rr) return HEAT_OK;
    const int64_t NR = rr->n_receivers, NE = rr->n_entries;
    if (NR < 0 || NE < 0)
        return failp(err, HEAT_E_INVALID_ARG, "negative count in room radiation (n_receivers %lld, n_entries %lld): no receiver r, no entry i",
                     (long long)NR, (long long)NE);
    if (NR > INT32_MAX || NE > INT32_MAX)
        return failp(err, HEAT_E_INVALID_ARG,
                     "more than 2^31 - 1 in room radiation (n_receivers %lld, n_entries %lld): receiver r and entry i are 32-bit", (long long)NR,
                     (long long)NE);
    if (NR > 0) {
        if (!rr->rc_surface) return failp(err, HEAT_E_INVALID_ARG, "receiver 0: rc_surface is NULL (n_receivers %lld)", (long long)NR);
        if (!rr->rc_side) return failp(err, HEAT_E_INVALID_ARG, "receiver 0: rc_side is NULL (n_receivers %lld)", (long long)NR);
    }
    if (NE > 0) {
        const void *need[4] = {rr->en_receiver, rr->en_surface, rr->en_side, rr->en_factor};
        static const char *const name[4] = {"en_receiver", "en_surface", "en_side", "en_factor"};
        for (int a = 0; a < 4; a++)
            if (!need[a]) return failp(err, HEAT_E_INVALID_ARG, "entry 0: %s is NULL (n_entries %lld)", name[a], (long long)NE);
    }
    const int32_t *chan[2] = {s->ir_front_chan, s->ir_back_chan};
    std::vector<int32_t> receiver_of(NR > 0 ? 2 * (size_t)n_surfaces : 0, -1);  // (surface, side) -> its receiver
    for (int64_t r = 0; r < NR; r++) {
        const int64_t q = rr->rc_surface[r];
        const unsigned side = rr->rc_side[r];
        if (side > 1) return failp(err, HEAT_E_INVALID_ARG, "receiver %lld: side %u above 1 (0 front, 1 back)", (long long)r, side);
        if (q < 0 || q >= n_surfaces)
            return failp(err, HEAT_E_SIZE, "receiver %lld: surface %lld outside [0, %lld)", (long long)r, (long long)q, (long long)n_surfaces);
        int32_t &seen = receiver_of[(size_t)side * n_surfaces + q];
        if (seen >= 0)
            return failp(err, HEAT_E_SIZE, "receiver %lld: the %s of surface %lld is receiver %d already", (long long)r, side ? "back" : "front",
                         (long long)q, seen);
        seen = (int32_t)r;
        if (chan[side] && chan[side][q] >= 0)
            return failp(err, HEAT_E_SIZE,
                         "receiver %lld: the long-wave %s input of surface %lld is driven by channel %d already: an input has one source",
                         (long long)r, side ? "back" : "front", (long long)q, chan[side][q]);
        if (sky && sky->mode && (sky->mode[q] >> (2 + side) & 1))
            return failp(err, HEAT_E_SIZE,
                         "receiver %lld: the long-wave %s input of surface %lld is driven by the sky (mode bit %u) already: an input has one source",
                         (long long)r, side ? "back" : "front", (long long)q, 2 + side);
    }
    for (int64_t i = 0; i < NE; i++) {
        const int64_t e = rr->en_surface[i];
        if (!std::isfinite(rr->en_factor[i]))
            return failp(err, HEAT_E_INVALID_ARG, "entry %lld: factor = %g is not finite", (long long)i, rr->en_factor[i]);
        if (e >= 0) {
            const unsigned side = rr->en_side[i];
            if (side > 1) return failp(err, HEAT_E_INVALID_ARG, "entry %lld: side %u above 1 (0 front, 1 back)", (long long)i, side);
            if (rr->en_chan && rr->en_chan[i] != -1)
                return failp(err, HEAT_E_INVALID_ARG, "entry %lld: channel %d beside emitter surface %lld (-1 where the emitter is a surface)",
                             (long long)i, rr->en_chan[i], (long long)e);
        } else if (e == -1 && !rr->en_chan) {
            return failp(err, HEAT_E_INVALID_ARG, "entry %lld: its emitter is -1 (a channel), but en_chan is NULL", (long long)i);
        }
        if (e < -1 || e >= n_surfaces)
            return failp(err, HEAT_E_SIZE, "entry %lld: emitter surface %lld outside [-1, %lld)", (long long)i, (long long)e, (long long)n_surfaces);
        if (rr->en_receiver[i] < 0 || rr->en_receiver[i] >= NR)
            return failp(err, HEAT_E_SIZE, "entry %lld: receiver %lld outside [0, %lld)", (long long)i, (long long)rr->en_receiver[i], (long long)NR);
        if (e == -1 && (rr->en_chan[i] < 0 || rr->en_chan[i] >= s->n_channels))
            return failp(err, HEAT_E_SIZE, "entry %lld: channel %d outside [0, %d)", (long long)i, rr->en_chan[i], s->n_channels);
    }
    return HEAT_OK;
}

void build_room_radiation_tables(int64_t n_surfaces, const heat_room_radiation *rr, RoomRadiationTables &t) {
    t.off.clear();
    t.src.clear();
    t.factor.clear();
    t.emitter.clear();
    const int64_t NR = rr ? rr->n_receivers : 0, NE = rr ? rr->n_entries : 0;
    if (NR <= 0) return;
    // the distinct emitter sides, ascending by key: a mark per side, then a prefix count (key -> emitter number)
    std::vector<int32_t> number_of(2 * (size_t)n_surfaces, -1);
    for (int64_t i = 0; i < NE; i++)
        if (rr->en_surface[i] >= 0) number_of[(size_t)rr->en_side[i] * n_surfaces + rr->en_surface[i]] = 0;
    for (size_t k = 0; k < number_of.size(); k++)
        if (number_of[k] == 0) {
            number_of[k] = (int32_t)t.emitter.size();
            t.emitter.push_back((int64_t)k);
        }
    // a counting sort by receiver: stable by construction
    t.off.assign((size_t)NR + 1, 0);
    for (int64_t i = 0; i < NE; i++) t.off[(size_t)rr->en_receiver[i] + 1]++;
    for (int64_t r = 0; r < NR; r++) t.off[(size_t)r + 1] += t.off[(size_t)r];
    t.src.assign((size_t)NE, 0);
    t.factor.assign((size_t)NE, 0.0);
    std::vector<int32_t> cursor(t.off.begin(), t.off.end() - 1);
    for (int64_t i = 0; i < NE; i++) {
        const size_t at = (size_t)cursor[(size_t)rr->en_receiver[i]]++;
        const int64_t e = rr->en_surface[i];
        t.src[at] = e >= 0 ? number_of[(size_t)rr->en_side[i] * n_surfaces + e] : ~rr->en_chan[i];
        t.factor[at] = rr->en_factor[i];
    }
}

int check_room_radiation_tables(int64_t n_surfaces, const heat_room_radiation *rr, const RoomRadiationTables &t, std::string &err) {
    const int64_t NR = rr ? rr->n_receivers : 0, NE = rr ? rr->n_entries : 0;
    if (NR <= 0) {
        if (!t.off.empty() || !t.src.empty() || !t.factor.empty() || !t.emitter.empty())
            return failp(err, HEAT_E_SIZE, "room radiation tables: tables without a receiver r");
        return HEAT_OK;
    }
    if (t.off.size() != (size_t)NR + 1 || t.off[0] != 0 || t.off.back() != NE || t.src.size() != (size_t)NE || t.factor.size() != (size_t)NE)
        return failp(err, HEAT_E_SIZE, "room radiation tables: %zu offsets, %zu sources and %zu factors for receiver r < %lld, entry i < %lld",
                     t.off.size(), t.src.size(), t.factor.size(), (long long)NR, (long long)NE);
    for (int64_t r = 0; r < NR; r++)
        if (t.off[(size_t)r + 1] < t.off[(size_t)r])
            return failp(err, HEAT_E_SIZE, "room radiation tables: receiver %lld runs from %d to %d", (long long)r, t.off[(size_t)r], t.off[(size_t)r + 1]);
    const size_t NM = t.emitter.size();
    for (size_t j = 0; j < NM; j++)
        if (t.emitter[j] < 0 || t.emitter[j] >= 2 * n_surfaces || (j > 0 && t.emitter[j] <= t.emitter[j - 1]))
            return failp(err, HEAT_E_SIZE, "room radiation tables: emitter %zu is side %lld, not above the one before or outside the %lld sides", j,
                         (long long)t.emitter[j], (long long)(2 * n_surfaces));
    // every entry of the caller's, in the caller's order, is the next element of its receiver's range
    std::vector<int32_t> cursor(t.off.begin(), t.off.end() - 1);
    std::vector<uint8_t> named(NM, 0);
    for (int64_t i = 0; i < NE; i++) {
        const size_t r = (size_t)rr->en_receiver[i];
        if (cursor[r] >= t.off[r + 1]) return failp(err, HEAT_E_SIZE, "room radiation tables: entry %lld: receiver %zu has no room for it", (long long)i, r);
        const size_t at = (size_t)cursor[r]++;
        const int64_t e = rr->en_surface[i];
        bool same = std::memcmp(&t.factor[at], &rr->en_factor[i], sizeof(double)) == 0;
        if (e >= 0) {
            const int32_t j = t.src[at];
            same = same && j >= 0 && (size_t)j < NM && t.emitter[(size_t)j] == (int64_t)rr->en_side[i] * n_surfaces + e;
            if (same) named[(size_t)j] = 1;
        } else {
            same = same && t.src[at] == ~rr->en_chan[i];
        }
        if (!same)
            return failp(err, HEAT_E_SIZE, "room radiation tables: entry %lld is not element %d of receiver %zu", (long long)i, (int)at - t.off[r], r);
    }
    for (int64_t r = 0; r < NR; r++)
        if (cursor[(size_t)r] != t.off[(size_t)r + 1])
            return failp(err, HEAT_E_SIZE, "room radiation tables: receiver %lld holds %d elements no entry i put there", (long long)r,
                         t.off[(size_t)r + 1] - cursor[(size_t)r]);
    for (size_t j = 0; j < NM; j++)
        if (!named[j]) return failp(err, HEAT_E_SIZE, "room radiation tables: emitter %zu is named by no entry i", j);
    return HEAT_OK;
}

// ---- ambient temperatures after creation (include/heat_amd.h, heat_batch_set_ambient and heat_ambient_drive) ----
int check_ambient_sides(int64_t n_surfaces, const int32_t *const kind[2], int64_t n, const int64_t *surface, const uint8_t *side,
                        const char *what, std::string &err) {
    if (n < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count (%lld): no %s i", (long long)n, what);
    if (n == 0) return HEAT_OK;
    if (n > INT32_MAX) return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 sides (%lld): %s i is 32-bit", (long long)n, what);
    if (!surface) return failp(err, HEAT_E_INVALID_ARG, "%s 0: surface is NULL (count %lld)", what, (long long)n);
    if (!side) return failp(err, HEAT_E_INVALID_ARG, "%s 0: side is NULL (count %lld)", what, (long long)n);
    std::vector<int32_t> seen(2 * (size_t)n_surfaces, -1);  // (surface, side) -> the element that names it
    for (int64_t i = 0; i < n; i++) {
        const int64_t q = surface[i];
        const unsigned sd = side[i];
        if (sd > 1) return failp(err, HEAT_E_INVALID_ARG, "%s %lld: side %u above 1 (0 front, 1 back)", what, (long long)i, sd);
        if (q < 0 || q >= n_surfaces)
            return failp(err, HEAT_E_SIZE, "%s %lld: surface %lld outside [0, %lld)", what, (long long)i, (long long)q, (long long)n_surfaces);
        if (kind[sd][q] != HEAT_BOUNDARY_AMBIENT)
            return failp(err, HEAT_E_SIZE, "%s %lld: the %s of surface %lld is of kind %d, not HEAT_BOUNDARY_AMBIENT (%d)", what, (long long)i,
                         sd ? "back" : "front", (long long)q, kind[sd][q], (int)HEAT_BOUNDARY_AMBIENT);
        int32_t &first = seen[(size_t)sd * n_surfaces + q];
        if (first >= 0)
            return failp(err, HEAT_E_SIZE, "%s %lld: the %s of surface %lld is %s %d already: an input has one source", what, (long long)i,
                         sd ? "back" : "front", (long long)q, what, first);
        first = (int32_t)i;
    }
    return HEAT_OK;
}

int check_ambient(int64_t n_surfaces, const int32_t *const kind[2], int64_t n_zones, const heat_series *s, const heat_ambient_drive *a,
                  std::string &err) {
    if (!a) return HEAT_OK;
    const int64_t N = a->n_sides;
    int rc = check_ambient_sides(n_surfaces, kind, N, a->surface, a->side, "ambient side", err);
    if (rc || N == 0) return rc;
    if (!a->chan) return failp(err, HEAT_E_INVALID_ARG, "ambient side 0: chan is NULL (n_sides %lld)", (long long)N);
    for (int64_t i = 0; i < N; i++) {
        if (a->gain && !std::isfinite(a->gain[i]))
            return failp(err, HEAT_E_INVALID_ARG, "ambient side %lld: gain = %g is not finite", (long long)i, a->gain[i]);
        if (a->offset && !std::isfinite(a->offset[i]))
            return failp(err, HEAT_E_INVALID_ARG, "ambient side %lld: offset = %g is not finite", (long long)i, a->offset[i]);
        const int32_t z = a->mix_zone ? a->mix_zone[i] : -1;
        if (z >= 0 && !a->mix)
            return failp(err, HEAT_E_INVALID_ARG, "ambient side %lld: mix_zone %d, but mix is NULL", (long long)i, z);
        if (z >= 0 && z < n_zones && !std::isfinite(a->mix[i]))
            return failp(err, HEAT_E_INVALID_ARG, "ambient side %lld: mix = %g is not finite", (long long)i, a->mix[i]);
        if (a->chan[i] < 0 || a->chan[i] >= s->n_channels)
            return failp(err, HEAT_E_SIZE, "ambient side %lld: channel %d outside [0, %d)", (long long)i, a->chan[i], s->n_channels);
        if (z < -1 || z >= n_zones)
            return failp(err, HEAT_E_SIZE, "ambient side %lld: mix_zone %d outside [-1, %lld)", (long long)i, z, (long long)n_zones);
    }
    return HEAT_OK;
}

void build_ambient_tables(int64_t n_surfaces, const int32_t *dev_of, const int32_t *const kind[2], int64_t n, const int64_t *surface,
                          const uint8_t *side, AmbientTables &t) {
    t.rec.clear();
    t.peer.clear();
    if (n <= 0) return;
    t.rec.resize((size_t)n);
    t.peer.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int64_t q = surface[i], d = dev_of ? (int64_t)dev_of[q] : q;
        t.rec[(size_t)i] = (uint32_t)((int64_t)side[i] * n_surfaces + d);
        // a FRONT whose surface's BACK is Ambient too: that back record's `forced` slot carries this temperature
        t.peer[(size_t)i] = (side[i] == 0 && kind[1][q] == HEAT_BOUNDARY_AMBIENT) ? (uint32_t)(n_surfaces + d) : kNoAmbientPeer;
    }
}

int check_ambient_tables(int64_t n_surfaces, const int32_t *dev_of, const int32_t *const kind[2], int64_t n, const int64_t *surface,
                         const uint8_t *side, const AmbientTables &t, std::string &err) {
    if (n <= 0) {
        if (!t.rec.empty() || !t.peer.empty()) return failp(err, HEAT_E_SIZE, "ambient tables: tables without an ambient side i");
        return HEAT_OK;
    }
    if (t.rec.size() != (size_t)n || t.peer.size() != (size_t)n)
        return failp(err, HEAT_E_SIZE, "ambient tables: %zu records and %zu peers for ambient side i < %lld", t.rec.size(), t.peer.size(),
                     (long long)n);
    // device surface -> the caller's (the inverse of dev_of), to read the kinds of a record
    std::vector<int64_t> orig_of((size_t)n_surfaces, -1);
    for (int64_t q = 0; q < n_surfaces; q++) {
        const int64_t d = dev_of ? (int64_t)dev_of[q] : q;
        if (d < 0 || d >= n_surfaces || orig_of[(size_t)d] >= 0)
            return failp(err, HEAT_E_SIZE, "ambient tables: surface %lld has device surface %lld, taken or outside [0, %lld)", (long long)q,
                         (long long)d, (long long)n_surfaces);
        orig_of[(size_t)d] = q;
    }
    std::vector<uint8_t> named(2 * (size_t)n_surfaces, 0);
    for (int64_t i = 0; i < n; i++) {
        const uint64_t rec = t.rec[(size_t)i];
        if (rec >= 2 * (uint64_t)n_surfaces)
            return failp(err, HEAT_E_SIZE, "ambient tables: ambient side %lld has record %llu outside [0, %lld)", (long long)i,
                         (unsigned long long)rec, (long long)(2 * n_surfaces));
        const int sd = rec >= (uint64_t)n_surfaces;
        const int64_t d = (int64_t)rec - (int64_t)sd * n_surfaces, q = orig_of[(size_t)d];
        if (q != surface[i] || sd != (int)side[i] || kind[sd][q] != HEAT_BOUNDARY_AMBIENT)
            return failp(err, HEAT_E_SIZE, "ambient tables: ambient side %lld has the record of the %s of surface %lld", (long long)i,
                         sd ? "back" : "front", (long long)q);
        if (named[(size_t)rec]) return failp(err, HEAT_E_SIZE, "ambient tables: ambient side %lld: record %llu is named twice", (long long)i, (unsigned long long)rec);
        named[(size_t)rec] = 1;
        const uint32_t want = (sd == 0 && kind[1][q] == HEAT_BOUNDARY_AMBIENT) ? (uint32_t)(n_surfaces + d) : kNoAmbientPeer;
        if (t.peer[(size_t)i] != want)
            return failp(err, HEAT_E_SIZE, "ambient tables: ambient side %lld has peer %u, not %u", (long long)i, t.peer[(size_t)i], want);
    }
    return HEAT_OK;
}

static inline int64_t gain_key(int64_t n_surfaces, const int32_t *dev_of, const heat_solar_gains *g, int64_t i) {
    const int64_t q = g->en_surface[i];
    return (int64_t)g->en_side[i] * n_surfaces + (dev_of ? (int64_t)dev_of[q] : q);
}

void build_solar_gain_tables(int64_t n_surfaces, const int32_t *dev_of, const heat_solar_gains *g, SolarGainTables &t) {
    t.rec.clear();
    t.slice_off.assign(1, 0);
    t.ap.clear();
    t.share.clear();
    const int64_t NE = g ? g->n_entries : 0;
    if (NE <= 0) return;
    // a counting sort by receiver: stable by construction — the caller's order survives inside a receiver
    std::vector<int32_t> count(2 * (size_t)n_surfaces, 0);
    for (int64_t i = 0; i < NE; i++) count[(size_t)gain_key(n_surfaces, dev_of, g, i)]++;
    std::vector<int32_t> len;                 // entries of every receiver
    std::vector<int32_t> &recv_of = count;    // (reused: key -> receiver)
    for (size_t k = 0; k < 2 * (size_t)n_surfaces; k++) {
        const int32_t c = count[k];
        if (c > 0) {
            recv_of[k] = (int32_t)t.rec.size();
            t.rec.push_back((uint32_t)k);
            len.push_back(c);
        }
    }
    const size_t R = t.rec.size(), n_slices = (R + kGainSlice - 1) / kGainSlice;
    for (size_t q = 0; q < n_slices; q++) {
        int32_t rows = 0;
        for (size_t r = q * kGainSlice; r < std::min(R, (q + 1) * kGainSlice); r++) rows = std::max(rows, len[r]);
        t.slice_off.push_back(t.slice_off.back() + (int64_t)rows * kGainSlice);
    }
    t.ap.assign((size_t)t.slice_off.back(), -1);
    t.share.assign(2 * (size_t)t.slice_off.back(), 0.0);
    std::vector<int32_t> &cursor = len;  // (reused: the next row of every receiver)
    std::fill(cursor.begin(), cursor.end(), 0);
    for (int64_t i = 0; i < NE; i++) {
        const size_t r = (size_t)recv_of[(size_t)gain_key(n_surfaces, dev_of, g, i)];
        const size_t at = (size_t)t.slice_off[r / kGainSlice] + (size_t)cursor[r]++ * kGainSlice + r % kGainSlice;
        t.ap[at] = g->en_aperture[i];
        t.share[2 * at] = g->en_beam[i];
        t.share[2 * at + 1] = g->en_diffuse[i];
    }
}

int check_solar_gain_tables(int64_t n_surfaces, const int32_t *dev_of, const heat_solar_gains *g, const SolarGainTables &t,
                            std::string &err) {
    const int64_t NE = g ? g->n_entries : 0;
    const size_t R = t.rec.size(), n_slices = (R + kGainSlice - 1) / kGainSlice;
    if (t.slice_off.size() != n_slices + 1 || t.slice_off[0] != 0)
        return failp(err, HEAT_E_SIZE, "solar gain tables: %zu slice offsets for %zu receivers", t.slice_off.size(), R);
    for (size_t q = 0; q < n_slices; q++)
        if (t.slice_off[q + 1] < t.slice_off[q] || (t.slice_off[q + 1] - t.slice_off[q]) % kGainSlice != 0)
            return failp(err, HEAT_E_SIZE, "solar gain tables: slice %zu runs from %lld to %lld", q, (long long)t.slice_off[q], (long long)t.slice_off[q + 1]);
    if (t.ap.size() != (size_t)t.slice_off.back() || t.share.size() != 2 * t.ap.size())
        return failp(err, HEAT_E_SIZE, "solar gain tables: %zu apertures and %zu shares for %lld elements", t.ap.size(), t.share.size(),
                     (long long)t.slice_off.back());
    for (size_t r = 0; r < R; r++)
        if (t.rec[r] >= 2 * (uint64_t)n_surfaces || (r > 0 && t.rec[r] <= t.rec[r - 1]))
            return failp(err, HEAT_E_SIZE, "solar gain tables: receiver %zu is record %u, not above the one before or outside the %lld sides", r,
                         t.rec[r], (long long)(2 * n_surfaces));
    // every entry of the caller's, in the caller's order, is the next row of its receiver's lane
    std::vector<int32_t> cursor(R, 0);
    for (int64_t i = 0; i < NE; i++) {
        const uint32_t key = (uint32_t)gain_key(n_surfaces, dev_of, g, i);
        const auto it = std::lower_bound(t.rec.begin(), t.rec.end(), key);
        if (it == t.rec.end() || *it != key) return failp(err, HEAT_E_SIZE, "solar gain tables: entry %lld: its receiver is not in the tables", (long long)i);
        const size_t r = (size_t)(it - t.rec.begin()), q = r / kGainSlice;
        const int64_t rows = (t.slice_off[q + 1] - t.slice_off[q]) / kGainSlice;
        if (cursor[r] >= rows) return failp(err, HEAT_E_SIZE, "solar gain tables: entry %lld: receiver %zu has no row %d", (long long)i, r, cursor[r]);
        const size_t at = (size_t)t.slice_off[q] + (size_t)cursor[r]++ * kGainSlice + r % kGainSlice;
        if (t.ap[at] != g->en_aperture[i] || std::memcmp(&t.share[2 * at], &g->en_beam[i], sizeof(double)) != 0 ||
            std::memcmp(&t.share[2 * at + 1], &g->en_diffuse[i], sizeof(double)) != 0)
            return failp(err, HEAT_E_SIZE, "solar gain tables: entry %lld is not row %d of receiver %zu", (long long)i, cursor[r] - 1, r);
    }
    // ... and nothing else is: a receiver has an entry, the rest of every column is padding
    int64_t n_used = 0;
    for (size_t r = 0; r < R; r++) {
        const size_t q = r / kGainSlice;
        const int64_t rows = (t.slice_off[q + 1] - t.slice_off[q]) / kGainSlice;
        if (cursor[r] < 1) return failp(err, HEAT_E_SIZE, "solar gain tables: receiver %zu has no entry", r);
        for (int64_t i = cursor[r]; i < rows; i++)
            if (t.ap[(size_t)t.slice_off[q] + (size_t)i * kGainSlice + r % kGainSlice] != -1)
                return failp(err, HEAT_E_SIZE, "solar gain tables: receiver %zu: row %lld is neither an entry nor padding", r, (long long)i);
        n_used += cursor[r];
    }
    for (size_t r = R; r < n_slices * kGainSlice; r++) {  // the lanes past the last receiver
        const size_t q = r / kGainSlice;
        for (int64_t at = t.slice_off[q] + (int64_t)(r % kGainSlice); at < t.slice_off[q + 1]; at += kGainSlice)
            if (t.ap[(size_t)at] != -1) return failp(err, HEAT_E_SIZE, "solar gain tables: lane %zu past the last receiver holds an entry", r);
    }
    if (n_used != NE) return failp(err, HEAT_E_SIZE, "solar gain tables: %lld entries for %lld", (long long)n_used, (long long)NE);
    return HEAT_OK;
}

// ---- report of a series (include/heat_amd.h, heat_series_report) ----
int check_series_report(SlotResolver &res, const heat_zone_loads *l, const heat_series_report *r, std::string &err,
                        std::vector<ResolvedSlot> *resolved) {
    if (!r) return HEAT_OK;
    if (r->n_groups < 0) return failp(err, HEAT_E_INVALID_ARG, "negative count in series report (n_groups %lld)", (long long)r->n_groups);
    if (r->n_groups > INT32_MAX) return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 groups in series report");
    int64_t n_entries = 0;
    if (r->n_groups > 0) {
        if (!r->group_offset) return failp(err, HEAT_E_INVALID_ARG, "group_offset is NULL");
        if (r->group_offset[0] != 0)
            return failp(err, HEAT_E_INVALID_ARG, "group 0: group_offset starts at %lld, not 0", (long long)r->group_offset[0]);
        for (int64_t g = 0; g < r->n_groups; g++)
            if (r->group_offset[g + 1] < r->group_offset[g])
                return failp(err, HEAT_E_INVALID_ARG, "group %lld: group_offset decreases (%lld after %lld)", (long long)g,
                             (long long)r->group_offset[g + 1], (long long)r->group_offset[g]);
        n_entries = r->group_offset[r->n_groups];
    }
    // (the tables number their entries with 32 bits)
    if (n_entries > INT32_MAX) return failp(err, HEAT_E_INVALID_ARG, "more than 2^31 - 1 group entries in series report");
    if (n_entries > 0 && !r->group_slot) return failp(err, HEAT_E_INVALID_ARG, "group_slot is NULL");
    if ((r->q_step_min && !r->q_min) || (r->q_step_max && !r->q_max))
        return failp(err, HEAT_E_INVALID_ARG, "q_step_min / q_step_max without q_min / q_max");
    if ((r->q_n_below || r->q_deg_below) && !r->q_lo) return failp(err, HEAT_E_INVALID_ARG, "q_n_below or q_deg_below without q_lo");
    if ((r->q_n_above || r->q_deg_above) && !r->q_hi) return failp(err, HEAT_E_INVALID_ARG, "q_n_above or q_deg_above without q_hi");
    const bool th = r->th_steps_heating || r->th_steps_cooling || r->th_switches || r->th_sum_heating || r->th_sum_cooling;
    if (th && (!l || l->n_thermostats <= 0)) return failp(err, HEAT_E_INVALID_ARG, "thermostat statistics without thermostats");
    if (r->group_weight)
        for (int64_t i = 0; i < n_entries; i++)
            if (!std::isfinite(r->group_weight[i]))
                return failp(err, HEAT_E_INVALID_ARG, "group entry %lld: weight %g is not finite", (long long)i, r->group_weight[i]);
    // every entry resolved once: the march and the host-only check build their tables from `resolved`
    std::vector<ResolvedSlot> local;
    std::vector<ResolvedSlot> &out = resolved ? *resolved : local;
    out.resize((size_t)n_entries);
    int64_t bad = -1;
    for (int64_t i = 0; i < n_entries && bad < 0; i++) {
        int kind = 0, node = 0;
        int64_t index = 0;
        if (!res.resolve(r->group_slot[i], kind, index, node)) bad = i;
        else out[(size_t)i] = ResolvedSlot{kind, node, index};
    }
    if (bad >= 0)
        return failp(err, HEAT_E_SIZE, "group entry %lld: slot %lld is not a node-temperature, hs, flow or zone slot of the descriptor",
                     (long long)bad, (long long)r->group_slot[bad]);
    return HEAT_OK;
}

void build_group_tables(int64_t n_groups, const int64_t *offset, const double *weight, const uint64_t *key, GroupTables &t) {
    t = GroupTables();
    t.part_off.assign((size_t)n_groups + 1, 0);
    if (n_groups <= 0) return;
    const size_t n_entries = (size_t)offset[n_groups];
    t.key.resize(n_entries);
    if (weight) t.weight.resize(n_entries);
    std::vector<int64_t> order;
    uint32_t n_part = 0;
    for (int64_t g = 0; g < n_groups; g++) {
        const int64_t e0 = offset[g], e1 = offset[g + 1], n = e1 - e0;
        order.resize((size_t)n);
        for (int64_t i = 0; i < n; i++) order[(size_t)i] = e0 + i;
        // (a slot that enters a group several times: by weight, so that the order is a function of the entries, not of how
        // the caller listed them)
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
            return key[a] != key[b] ? key[a] < key[b] : (weight != nullptr && weight[a] < weight[b]);
        });
        for (int64_t i = 0; i < n; i++) {
            t.key[(size_t)(e0 + i)] = key[order[(size_t)i]];
            if (weight) t.weight[(size_t)(e0 + i)] = weight[order[(size_t)i]];
        }
        t.part_off[(size_t)g] = n_part;
        if (n == 0) continue;
        if (n <= kGroupRowEntries) {
            t.row_seg.insert(t.row_seg.end(), {(uint32_t)e0, (uint32_t)e1, n_part++});
        } else {
            for (int64_t a = e0; a < e1; a += kGroupSegment)
                t.wave_seg.insert(t.wave_seg.end(), {(uint32_t)a, (uint32_t)std::min<int64_t>(a + kGroupSegment, e1), n_part++});
        }
    }
    t.part_off[(size_t)n_groups] = n_part;
}

int check_group_tables(int64_t n_groups, const int64_t *offset, const GroupTables &t, std::string &err) {
    if (t.part_off.size() != (size_t)n_groups + 1) return failp(err, HEAT_E_SIZE, "group tables: %zu partial offsets for %lld groups", t.part_off.size(), (long long)n_groups);
    const size_t n_part = t.part_off[(size_t)n_groups];
    const size_t n_entries = n_groups > 0 ? (size_t)offset[n_groups] : 0;
    if (t.key.size() != n_entries || (!t.weight.empty() && t.weight.size() != n_entries))
        return failp(err, HEAT_E_SIZE, "group tables: %zu keys, %zu weights for %zu entries", t.key.size(), t.weight.size(), n_entries);
    if (t.wave_seg.size() % 3 || t.row_seg.size() % 3 || t.wave_seg.size() / 3 + t.row_seg.size() / 3 != n_part)
        return failp(err, HEAT_E_SIZE, "group tables: %zu + %zu segments for %zu partial sums", t.wave_seg.size() / 3, t.row_seg.size() / 3, n_part);
    // every partial sum has one segment, and a group's segments tile its entries in order
    std::vector<uint32_t> first(n_part, 0), end(n_part, 0);
    std::vector<uint8_t> seen(n_part, 0);
    for (const std::vector<uint32_t> *v : {&t.wave_seg, &t.row_seg})
        for (size_t i = 0; i < v->size(); i += 3) {
            const uint32_t e0 = (*v)[i], e1 = (*v)[i + 1], p = (*v)[i + 2];
            const uint32_t longest = v == &t.row_seg ? kGroupRowEntries : kGroupSegment;
            if (p >= n_part || seen[p] || e1 <= e0 || e1 - e0 > longest || e1 > n_entries)
                return failp(err, HEAT_E_SIZE, "group tables: segment %zu [%u, %u) -> partial %u is inconsistent", i / 3, e0, e1, p);
            seen[p] = 1, first[p] = e0, end[p] = e1;
        }
    for (int64_t g = 0; g < n_groups; g++) {
        int64_t at = offset[g];
        if (t.part_off[(size_t)g] > t.part_off[(size_t)g + 1]) return failp(err, HEAT_E_SIZE, "group %lld: partial offsets decrease", (long long)g);
        for (uint32_t p = t.part_off[(size_t)g]; p < t.part_off[(size_t)g + 1]; p++) {
            if (!seen[p] || first[p] != at) return failp(err, HEAT_E_SIZE, "group %lld: its segments do not tile its entries", (long long)g);
            at = end[p];
        }
        if (at != offset[g + 1]) return failp(err, HEAT_E_SIZE, "group %lld: its segments end at %lld, not %lld", (long long)g, (long long)at, (long long)offset[g + 1]);
        for (int64_t i = offset[g] + 1; i < offset[g + 1]; i++)
            if (t.key[(size_t)i] < t.key[(size_t)i - 1]) return failp(err, HEAT_E_SIZE, "group %lld: entries not in device order", (long long)g);
    }
    return HEAT_OK;
}

// What a series may probe, from a descriptor that passed check_desc (node_count: storage the model points into).
static SeriesModel series_model_of(const heat_batch_desc *desc, std::vector<int64_t> &node_count) {
    const int64_t S = desc->n_surfaces;
    node_count.resize((size_t)S);
    for (int64_t q = 0; q < S; q++) node_count[q] = desc->node_offset[q + 1] - desc->node_offset[q];
    SeriesModel m;
    m.n_surfaces = S;
    m.n_zones = desc->n_zones;
    m.first_node_slot = desc->first_node_slot;
    m.node_count = node_count.data();
    m.out_slot[0] = desc->hs_front_slot;
    m.out_slot[1] = desc->hs_back_slot;
    m.out_slot[2] = desc->flow_front_slot;
    m.out_slot[3] = desc->flow_back_slot;
    m.zone_slot = desc->zone_slot;
    return m;
}

std::string &last_error() {
    thread_local std::string e;
    return e;
}

}  // namespace heat

// ---------------------------------------------------------------------------
// Host-only entry points of the C ABI (include/heat_amd.h): no device needed.
extern "C" {

const char *heat_last_error(void) { return heat::last_error().c_str(); }
int heat_amd_abi_version(void) { return HEAT_AMD_ABI_VERSION; }

int heat_partition(const heat_batch_desc *desc, int32_t n_ranks, int32_t *rank_of_surface, int64_t *n_shared_zones) {
    return heat::partition_surfaces(desc, n_ranks, rank_of_surface, n_shared_zones, heat::last_error());
}

static int plan_check_impl(const heat_batch_desc *desc, const heat_batch_options *opt_in, int32_t n_sites,
                           const int32_t *site_of_surface, bool sites, int64_t summary[8]) {
    heat_batch_options opt;
    memset(&opt, 0, sizeof opt);
    opt.device = -1;
    opt.n_ranks = 1;
    if (opt_in) opt = *opt_in;
    int rc;
    if (sites) {
        rc = heat::check_sites(desc, opt, n_sites, site_of_surface, heat::last_error());
        if (rc) return rc;
    }
    heat::Plan p;
    rc = heat::make_plan(desc, opt, p, heat::last_error(), n_sites, site_of_surface);
    if (rc) return rc;
    rc = heat::check_plan(p, desc, heat::last_error(), site_of_surface);
    if (rc) return rc;
    if (summary) {
        int64_t n_blocks = 0, n_fast_tiles = 0;
        for (int c = 0; c < heat::kNumFast; c++) {
            n_fast_tiles += (int64_t)p.fast_tiles[c].size();
            for (int g2 = 0; g2 < 4; g2++) n_blocks += (int64_t)p.fblocks[c][g2].size();
            n_blocks += (int64_t)p.team_blocks[c].size();
        }
        summary[0] = p.class_counts[0];
        summary[1] = p.class_counts[1];
        summary[2] = p.class_counts[2];
        summary[3] = p.class_counts[3];
        summary[4] = p.class_counts[4];
        summary[5] = p.n_fused_surfaces;
        summary[6] = n_blocks;
        summary[7] = n_fast_tiles + (int64_t)p.gen_tiles.size();
    }
    return HEAT_OK;
}

int heat_series_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s) {
    int rc = heat::check_desc(desc, heat::last_error());
    if (rc) return rc;
    std::vector<int64_t> node_count;
    const heat::SeriesModel m = heat::series_model_of(desc, node_count);
    heat::SlotResolver res(m);
    return heat::check_series(m, res, n_sites, s, heat::last_error());
}

int heat_zone_loads_check(const heat_batch_desc *desc, const heat_series *s, const heat_zone_loads *l) {
    int rc = heat::check_desc(desc, heat::last_error());
    if (rc) return rc;
    if (!s) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "series is NULL");
    if (s->n_channels < 0) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "negative count in series (n_channels %d)", s->n_channels);
    rc = heat::check_zone_loads(desc->n_zones, s->n_channels, l, heat::last_error());
    if (rc || !l) return rc;
    // ... and the tables the march would upload, laid out and checked against the counts (this is the build the sanitizers see)
    heat::ZoneLoadTables t;
    heat::build_zone_load_tables(desc->n_zones, l, t);
    const size_t Z1 = (size_t)desc->n_zones + 1;
    const int64_t n[3] = {l->n_gains, l->n_flows, l->n_thermostats};
    for (int a = 0; a < 3; a++)
        for (size_t z = 0; z < Z1; z++)
            if (t.off[a * Z1 + z] < (z ? t.off[a * Z1 + z - 1] : 0) || t.off[a * Z1 + z] > n[a] || (z + 1 == Z1 && t.off[a * Z1 + z] != n[a]))
                return heat::failp(heat::last_error(), HEAT_E_SIZE, "zone load tables: offsets of list %d are inconsistent at zone %zu", a, z);
    return HEAT_OK;
}

int heat_ideal_loads_check(const heat_batch_desc *desc, const heat_series *s, const heat_ideal_loads *il) {
    int rc = heat::check_desc(desc, heat::last_error());
    if (rc) return rc;
    if (!s) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "series is NULL");
    if (s->n_channels < 0) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "negative count in series (n_channels %d)", s->n_channels);
    // ... and the table the march would upload, checked against the loads (this is the build the sanitizers see)
    std::vector<int32_t> load_of_zone;
    rc = heat::check_ideal_loads(desc->n_zones, s->n_channels, il, heat::last_error(), &load_of_zone);
    if (rc || !il) return rc;
    if (load_of_zone.size() != (size_t)desc->n_zones)
        return heat::failp(heat::last_error(), HEAT_E_SIZE, "ideal load table: %zu entries for %lld zones", load_of_zone.size(), (long long)desc->n_zones);
    int64_t n_set = 0;
    for (int32_t i : load_of_zone) n_set += i >= 0;
    if (n_set != il->n_loads)
        return heat::failp(heat::last_error(), HEAT_E_SIZE, "ideal load table: %lld zones with a load for %lld loads", (long long)n_set, (long long)il->n_loads);
    for (int64_t i = 0; i < il->n_loads; i++)
        if (load_of_zone[(size_t)il->zone[i]] != (int32_t)i)
            return heat::failp(heat::last_error(), HEAT_E_SIZE, "ideal load %lld: the table gives its zone %d load %d", (long long)i, il->zone[i],
                               load_of_zone[(size_t)il->zone[i]]);
    return HEAT_OK;
}

int heat_sky_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky) {
    int rc = heat_series_check(desc, n_sites, s);
    if (rc) return rc;
    return heat::check_sky(desc->n_surfaces, s, sky, heat::last_error());
}

int heat_solar_gains_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky,
                           const heat_solar_gains *gains) {
    int rc = heat_sky_check(desc, n_sites, s, sky);
    if (rc) return rc;
    rc = heat::check_solar_gains(desc->n_surfaces, s, sky, gains, heat::last_error());
    if (rc || !gains) return rc;
    // ... and the tables the march would upload (this is the build the sanitizers see). Without a batch there is no device
    // layout: the receivers stand in the caller's surface order.
    heat::SolarGainTables t;
    heat::build_solar_gain_tables(desc->n_surfaces, nullptr, gains, t);
    return heat::check_solar_gain_tables(desc->n_surfaces, nullptr, gains, t, heat::last_error());
}

int heat_shades_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky,
                      const heat_solar_gains *gains, const heat_shades *shades) {
    int rc = heat_solar_gains_check(desc, n_sites, s, sky, gains);
    if (rc) return rc;
    rc = heat::check_shades(desc->n_surfaces, s, sky, gains, shades, heat::last_error());
    if (rc || !shades) return rc;
    // ... and the table the march would upload, laid out and checked against the counts (this is the build the sanitizers see)
    heat::ShadeTables t;
    heat::build_shade_tables(shades, t);
    const size_t NS = shades->n_shades > 0 ? (size_t)shades->n_shades : 0;
    if (t.f64.size() != heat::kShadeRows * NS || t.horizon.size() != NS)
        return heat::failp(heat::last_error(), HEAT_E_SIZE, "shade tables: %zu values and %zu horizon numbers for shade j < %zu", t.f64.size(),
                           t.horizon.size(), NS);
    return HEAT_OK;
}

int heat_blinds_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky,
                      const heat_solar_gains *gains, const heat_shades *shades, const heat_blinds *blinds) {
    int rc = heat_shades_check(desc, n_sites, s, sky, gains, shades);
    if (rc) return rc;
    rc = heat::check_blinds(desc->n_zones, s, shades, blinds, heat::last_error());
    if (rc || !blinds) return rc;
    // ... and the tables the march would upload, built and checked against the caller's lists (this is the build the
    // sanitizers see)
    const int64_t NS = shades ? shades->n_shades : 0;
    heat::BlindTables t;
    heat::build_blind_tables(NS, blinds, t);
    return heat::check_blind_tables(NS, blinds, t, heat::last_error());
}

int heat_sky_aniso_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky,
                         const heat_solar_gains *gains, const heat_shades *shades, const heat_sky_aniso *aniso) {
    int rc = heat_shades_check(desc, n_sites, s, sky, gains, shades);
    if (rc) return rc;
    return heat::check_sky_aniso(desc->n_surfaces, s, sky, gains, shades, aniso, heat::last_error());
}

int heat_room_radiation_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_sky *sky,
                              const heat_room_radiation *radiation) {
    int rc = heat_sky_check(desc, n_sites, s, sky);
    if (rc) return rc;
    rc = heat::check_room_radiation(desc->n_surfaces, s, sky, radiation, heat::last_error());
    if (rc || !radiation) return rc;
    // ... and the tables the march would upload, built and checked against the caller's lists (this is the build the
    // sanitizers see)
    heat::RoomRadiationTables t;
    heat::build_room_radiation_tables(desc->n_surfaces, radiation, t);
    return heat::check_room_radiation_tables(desc->n_surfaces, radiation, t, heat::last_error());
}

int heat_ambient_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_ambient_drive *a) {
    int rc = heat_series_check(desc, n_sites, s);
    if (rc) return rc;
    const int32_t *const kind[2] = {desc->front_kind, desc->back_kind};
    rc = heat::check_ambient(desc->n_surfaces, kind, desc->n_zones, s, a, heat::last_error());
    if (rc || !a) return rc;
    // ... and the tables the march would upload, built and checked against the caller's lists (this is the build the
    // sanitizers see). Without a batch there is no device layout: the records stand in the caller's surface order.
    heat::AmbientTables t;
    heat::build_ambient_tables(desc->n_surfaces, nullptr, kind, a->n_sides, a->surface, a->side, t);
    return heat::check_ambient_tables(desc->n_surfaces, nullptr, kind, a->n_sides, a->surface, a->side, t, heat::last_error());
}

int heat_air_paths_check(const heat_batch_desc *desc, int32_t n_sites, const heat_series *s, const heat_air_paths *air) {
    int rc = heat_series_check(desc, n_sites, s);
    if (rc) return rc;
    rc = heat::check_air_paths(desc->n_zones, s->n_channels, air, heat::last_error());
    if (rc || !air) return rc;
    // ... and the tables the march would upload, built and checked against the caller's lists (this is the build the
    // sanitizers see)
    heat::AirPathTables t;
    heat::build_air_path_tables(desc->n_zones, air, t);
    return heat::check_air_path_tables(desc->n_zones, air, t, heat::last_error());
}

int heat_comfort_check(const heat_batch_desc *desc, const heat_series *s, const heat_comfort *c) {
    int rc = heat::check_desc(desc, heat::last_error());
    if (rc) return rc;
    if (!s) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "series is NULL");
    if (s->n_channels < 0) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "negative count in series (n_channels %d)", s->n_channels);
    rc = heat::check_comfort(desc->n_surfaces, desc->n_zones, s, c, heat::last_error());
    if (rc || !c) return rc;
    // ... and the tables the march would upload, built and checked against the caller's lists (this is the build the
    // sanitizers see). Without a batch there is no device layout: a face stands as the caller's state slot.
    std::vector<int64_t> node_count;
    const heat::SeriesModel m = heat::series_model_of(desc, node_count);
    heat::ComfortTables t;
    heat::build_comfort_tables(desc->n_zones, c, nullptr, nullptr, m.first_node_slot, m.node_count, t);
    return heat::check_comfort_tables(desc->n_zones, c, t, heat::last_error());
}

int heat_air_handlers_check(const heat_batch_desc *desc, const heat_series *s, const heat_air_handlers *h) {
    int rc = heat::check_desc(desc, heat::last_error());
    if (rc) return rc;
    if (!s) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "series is NULL");
    if (s->n_channels < 0) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "negative count in series (n_channels %d)", s->n_channels);
    rc = heat::check_air_handlers(desc->n_zones, s->n_channels, h, heat::last_error());
    if (rc || !h) return rc;
    // ... and the tables the march would upload, built and checked against the caller's lists (this is the build the
    // sanitizers see)
    heat::HandlerTables t;
    heat::build_air_handler_tables(desc->n_zones, h, t);
    return heat::check_air_handler_tables(desc->n_zones, h, t, heat::last_error());
}

int heat_air_species_check(const heat_batch_desc *desc, const heat_series *s, const heat_zone_loads *l, const heat_air_paths *air,
                           const heat_air_handlers *h, const heat_air_species *sp) {
    int rc = heat::check_desc(desc, heat::last_error());
    if (rc) return rc;
    if (!s) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "series is NULL");
    if (s->n_channels < 0) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "negative count in series (n_channels %d)", s->n_channels);
    // the three terms whose air the species ride on, as their own checks take them
    if ((rc = heat::check_zone_loads(desc->n_zones, s->n_channels, l, heat::last_error()))) return rc;
    if ((rc = heat::check_air_paths(desc->n_zones, s->n_channels, air, heat::last_error()))) return rc;
    if ((rc = heat::check_air_handlers(desc->n_zones, s->n_channels, h, heat::last_error()))) return rc;
    rc = heat::check_air_species(desc->n_zones, s->n_channels, sp, heat::last_error());
    if (rc || !sp) return rc;
    // ... and the tables the march would upload, built and checked against the caller's lists (this is the build the
    // sanitizers see)
    heat::SpeciesTables t;
    heat::build_air_species_tables(desc->n_zones, h, sp, t);
    return heat::check_air_species_tables(desc->n_zones, h, sp, t, heat::last_error());
}

int heat_openings_check(const heat_batch_desc *desc, const heat_series *s, const heat_openings *op) {
    int rc = heat::check_desc(desc, heat::last_error());
    if (rc) return rc;
    if (!s) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "series is NULL");
    if (s->n_channels < 0) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "negative count in series (n_channels %d)", s->n_channels);
    rc = heat::check_openings(desc->n_zones, s->n_channels, op, heat::last_error());
    if (rc || !op) return rc;
    // ... and the tables the march would upload, built and checked against the caller's lists (this is the build the
    // sanitizers see)
    heat::OpeningTables t;
    heat::build_opening_tables(op, t);
    return heat::check_opening_tables(desc->n_zones, s->n_channels, op, t, heat::last_error());
}

int heat_controllers_check(const heat_batch_desc *desc, const heat_series *s, const heat_openings *op, const heat_controllers *ct) {
    int rc = heat::check_desc(desc, heat::last_error());
    if (rc) return rc;
    if (!s) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "series is NULL");
    if (s->n_channels < 0) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "negative count in series (n_channels %d)", s->n_channels);
    if ((rc = heat::check_openings(desc->n_zones, s->n_channels, op, heat::last_error()))) return rc;
    std::vector<int64_t> node_count;
    const heat::SeriesModel m = heat::series_model_of(desc, node_count);
    rc = heat::check_controllers(m, s->n_channels, op, ct, heat::last_error());
    if (rc || !ct) return rc;
    // ... and the tables the march would upload, with the nodes numbered as the descriptor numbers them (the device's layout
    // is the batch's), built and checked against the caller's lists (this is the build the sanitizers see)
    heat::ControllerTables t;
    const int64_t *const node_offset = desc->node_offset;
    heat::build_controller_tables(m, ct, [node_offset](int64_t q, int node) { return (uint32_t)(node_offset[q] + node); }, t);
    return heat::check_controller_tables(m, s->n_channels, node_offset[desc->n_surfaces], ct, t, heat::last_error());
}

int heat_air_networks_check(const heat_batch_desc *desc, const heat_series *s, const heat_openings *op, const heat_controllers *ct,
                            const heat_air_networks *nw) {
    int rc = heat_controllers_check(desc, s, op, ct);
    if (rc) return rc;
    rc = heat::check_air_networks(desc->n_zones, s->n_channels, op, ct, nw, heat::last_error());
    if (rc || !nw) return rc;
    // ... and the tables the march would upload, built and checked against the caller's lists (this is the build the sanitizers see)
    heat::NetworkTables t;
    heat::build_network_tables(nw, t);
    return heat::check_network_tables(desc->n_zones, s->n_channels, nw, t, heat::last_error());
}

int heat_series_report_check(const heat_batch_desc *desc, const heat_series *s, const heat_zone_loads *l,
                             const heat_series_report *r) {
    int rc = heat_zone_loads_check(desc, s, l);
    if (rc) return rc;
    if (s->n_probes < 0) return heat::failp(heat::last_error(), HEAT_E_INVALID_ARG, "negative count in series (n_probes %lld)", (long long)s->n_probes);
    std::vector<int64_t> node_count;
    const heat::SeriesModel m = heat::series_model_of(desc, node_count);
    heat::SlotResolver res(m);
    std::vector<heat::ResolvedSlot> resolved;
    rc = heat::check_series_report(res, l, r, heat::last_error(), &resolved);
    if (rc || !r) return rc;
    // ... and the group tables the march would upload (this is the build the sanitizers see). Without a batch there is no
    // device layout: the entries are ordered by (kind, surface or zone, node) instead.
    const int64_t n_entries = r->n_groups > 0 ? r->group_offset[r->n_groups] : 0;
    std::vector<uint64_t> key((size_t)n_entries);
    for (int64_t i = 0; i < n_entries; i++)
        key[(size_t)i] = (uint64_t)resolved[(size_t)i].kind << 56 | (uint64_t)resolved[(size_t)i].index << 16 | (uint64_t)resolved[(size_t)i].node;
    heat::GroupTables t;
    heat::build_group_tables(r->n_groups, r->group_offset, r->group_weight, key.data(), t);
    return heat::check_group_tables(r->n_groups, r->group_offset, t, heat::last_error());
}

int heat_plan_check(const heat_batch_desc *desc, const heat_batch_options *opt, int64_t summary[8]) {
    return plan_check_impl(desc, opt, 1, nullptr, false, summary);
}

int heat_plan_check_sites(const heat_batch_desc *desc, const heat_batch_options *opt, int32_t n_sites,
                          const int32_t *site_of_surface, int64_t summary[8]) {
    return plan_check_impl(desc, opt, n_sites, site_of_surface, true, summary);
}

int heat_plan_ideal_resident(const heat_batch_desc *desc, const heat_batch_options *opt_in, int32_t n_sites,
                             const int32_t *site_of_surface, int32_t *reason) {
    if (reason) *reason = HEAT_IDEAL_RESIDENT_NONE_PLANNED;
    heat_batch_options opt;
    memset(&opt, 0, sizeof opt);
    opt.device = -1;
    opt.n_ranks = 1;
    if (opt_in) opt = *opt_in;
    int rc;
    if (site_of_surface != nullptr || n_sites != 1) {
        rc = heat::check_sites(desc, opt, n_sites, site_of_surface, heat::last_error());
        if (rc) return rc;
    }
    heat::Plan p;
    rc = heat::make_plan(desc, opt, p, heat::last_error(), n_sites, site_of_surface);
    if (rc) return rc;
    size_t n_blocks[heat::kNumFast][4], n_supers[heat::kNumFast];
    bool has_chunks[heat::kNumFast];
    for (int c = 0; c < heat::kNumFast; c++) {
        for (int g2 = 0; g2 < 4; g2++) n_blocks[c][g2] = p.fblocks[c][g2].size();
        n_supers[c] = p.team_supers[c].size();
        has_chunks[c] = false;
        for (const heat::FastTile &ft : p.fast_tiles[c]) has_chunks[c] = has_chunks[c] || (ft.k & heat::kTileChunkyBit) != 0;
    }
    const int why = heat::ideal_resident_reason(n_blocks, n_supers, has_chunks);
    if (reason) *reason = why;
    return why == HEAT_IDEAL_RESIDENT_OK ? 1 : 0;
}

}  // extern "C"
