// ideal_resident_host_main.cpp — a stand-alone driver of heat_plan_ideal_resident (include/heat_amd.h) for the sanitizers:
// tests/test_ideal_resident_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out small buildings — rooms of a few two-node walls each, side by side, or all
// joined into one chain by interior walls — and asks the planner, under every fusion option and with weather sites, whether an
// ideal series could keep the resident clusters resident. Every answer is checked against what the header promises of it: the
// return value is 1 exactly when the reason is HEAT_IDEAL_RESIDENT_OK, "nothing planned resident" exactly when
// heat_plan_check counts no resident surface, the reason pointer is optional, no_fusion = 1 plans nothing resident, bad
// site arguments come back as heat_plan_check_sites returns them. No device, no HIP.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "heat_amd.h"

namespace {

int n_failed = 0;

void expect(bool ok, const char *what, long long a = 0, long long b = 0) {
    if (!ok) {
        std::printf("FAILED %s (%lld, %lld): \"%s\"\n", what, a, b, heat_last_error() ? heat_last_error() : "");
        n_failed++;
    }
}

// S walls of n_nodes massive nodes; wall s stands between the outdoors and room s / per_room, or — chain — between room
// s % Z and room (s + 1) % Z, so that every room is joined to the next
struct Model {
    int64_t S, Z;
    std::vector<int64_t> node_offset, slot[9], zone_slot;
    std::vector<double> mass, uvalue, alpha, zeros, ones, zone_volume;
    std::vector<int32_t> kind_front, kind_back, zone_front, zone_back;
    heat_batch_desc desc;
    Model(int64_t S_, int64_t per_room, int64_t n_nodes, bool chain) : S(S_), Z((S_ + per_room - 1) / per_room) {
        node_offset.resize(S + 1);
        for (int64_t s = 0; s <= S; s++) node_offset[s] = n_nodes * s;
        mass.assign(n_nodes * S, 5000.0);
        uvalue.assign(n_nodes * S, 2.0);
        alpha.assign(n_nodes * S, 0.0);
        zeros.assign(S, 0.0);
        ones.assign(S, 1.0);
        kind_front.assign(S, chain ? HEAT_BOUNDARY_SPACE : HEAT_BOUNDARY_OUTDOOR);
        kind_back.assign(S, HEAT_BOUNDARY_SPACE);
        zone_front.assign(S, 0);
        zone_back.resize(S);
        for (int64_t s = 0; s < S; s++) {
            zone_back[s] = (int32_t)(chain ? s % Z : s / per_room);
            if (chain) zone_front[s] = (int32_t)((s + 1) % Z);
        }
        zone_slot.resize(Z);
        for (int64_t z = 0; z < Z; z++) zone_slot[z] = z;
        for (int a = 0; a < 9; a++) {
            slot[a].resize(S);
            for (int64_t s = 0; s < S; s++) slot[a][s] = Z + s * (8 + n_nodes) + (a < 8 ? a : 8);
        }
        zone_volume.assign(Z, 300.0);
        std::memset(&desc, 0, sizeof desc);
        desc.abi_version = HEAT_AMD_ABI_VERSION;
        desc.n_surfaces = S, desc.n_zones = Z, desc.n_cavities = 0, desc.n_state = Z + S * (8 + n_nodes);
        desc.dt = 60.0;
        desc.node_offset = node_offset.data(), desc.mass = mass.data(), desc.uvalue = uvalue.data();
        desc.front_alpha = alpha.data(), desc.back_alpha = alpha.data();
        desc.front_kind = kind_front.data(), desc.back_kind = kind_back.data();
        desc.front_zone = zone_front.data(), desc.back_zone = zone_back.data();
        desc.front_ambient = zeros.data(), desc.back_ambient = zeros.data();
        desc.front_emissivity = ones.data(), desc.back_emissivity = ones.data();
        desc.area = ones.data(), desc.perimeter = ones.data(), desc.cos_tilt = zeros.data();
        desc.normal_x = ones.data(), desc.normal_y = zeros.data(), desc.wind_modifier = ones.data();
        desc.hs_front_slot = slot[0].data(), desc.hs_back_slot = slot[1].data();
        desc.flow_front_slot = slot[2].data(), desc.flow_back_slot = slot[3].data();
        desc.solar_front_slot = slot[4].data(), desc.solar_back_slot = slot[5].data();
        desc.ir_front_slot = slot[6].data(), desc.ir_back_slot = slot[7].data();
        desc.first_node_slot = slot[8].data();
        desc.zone_volume = zone_volume.data(), desc.zone_slot = zone_slot.data();
    }
};

heat_batch_options options(int no_fusion, int no_palette = 0, int nodes_per_lane = 0) {
    heat_batch_options opt;
    std::memset(&opt, 0, sizeof opt);
    opt.device = -1, opt.n_ranks = 1, opt.no_fusion = no_fusion, opt.no_palette = no_palette, opt.nodes_per_lane = nodes_per_lane;
    return opt;
}

// One question, every way it can be put; returns the reason (or -1 after a failure).
int ask(const char *name, const Model &m, const heat_batch_options &opt) {
    int32_t reason = -7, again = -7;
    const int rc = heat_plan_ideal_resident(&m.desc, &opt, 1, nullptr, &reason);
    expect(rc == 0 || rc == 1, "status is 0 or 1", rc);
    if (rc != 0 && rc != 1) return -1;
    expect((rc == 1) == (reason == HEAT_IDEAL_RESIDENT_OK), "1 exactly when the reason is OK", rc, reason);
    expect(reason >= HEAT_IDEAL_RESIDENT_OK && reason <= HEAT_IDEAL_RESIDENT_CHUNK_LOOP_CLASS, "reason in the enum", reason);
    expect(heat_plan_ideal_resident(&m.desc, &opt, 1, nullptr, nullptr) == rc, "the reason pointer is optional", rc);
    expect(heat_plan_ideal_resident(&m.desc, &opt, 1, nullptr, &again) == rc && again == reason, "the same answer twice", reason, again);
    int64_t summary[8];
    std::memset(summary, 0, sizeof summary);
    expect(heat_plan_check(&m.desc, &opt, summary) == HEAT_OK, "heat_plan_check");
    expect((summary[5] == 0) == (reason == HEAT_IDEAL_RESIDENT_NONE_PLANNED), "none planned exactly when no surface is resident", summary[5], reason);
    // sites: every room's walls are of one site; the answer is a plan's, so it may differ from the single-site one, but
    // it obeys the same rules
    std::vector<int32_t> site((size_t)m.S);
    for (int64_t s = 0; s < m.S; s++) site[(size_t)s] = (int32_t)(m.zone_back[(size_t)s] % 3);
    bool one_site_per_cluster = true;
    for (int64_t s = 0; s < m.S; s++)
        if (m.kind_front[(size_t)s] == HEAT_BOUNDARY_SPACE) one_site_per_cluster = false;  // (a chain: one cluster, one site)
    if (!one_site_per_cluster) std::fill(site.begin(), site.end(), 2);
    int32_t r_sites = -7;
    const int rc_sites = heat_plan_ideal_resident(&m.desc, &opt, 3, site.data(), &r_sites);
    expect((rc_sites == 1) == (r_sites == HEAT_IDEAL_RESIDENT_OK) && (rc_sites == 0 || rc_sites == 1), "with sites", rc_sites, r_sites);
    std::memset(summary, 0, sizeof summary);
    expect(heat_plan_check_sites(&m.desc, &opt, 3, site.data(), summary) == HEAT_OK, "heat_plan_check_sites");
    expect((summary[5] == 0) == (r_sites == HEAT_IDEAL_RESIDENT_NONE_PLANNED), "with sites: none planned exactly when no surface is resident", summary[5], r_sites);
    // bad site arguments: the codes of heat_plan_check_sites, before any planning
    site[0] = 3;
    expect(heat_plan_ideal_resident(&m.desc, &opt, 3, site.data(), &r_sites) == heat_plan_check_sites(&m.desc, &opt, 3, site.data(), nullptr),
           "a site out of range");
    expect(heat_plan_ideal_resident(&m.desc, &opt, 3, site.data(), &r_sites) < 0, "a site out of range is refused");
    site[0] = 0;
    expect(heat_plan_ideal_resident(&m.desc, &opt, 0, site.data(), &r_sites) < 0, "no site at all is refused");
    std::printf("%s no_fusion=%d: eligible %d, reason %d, resident surfaces %lld\n", name, opt.no_fusion, rc, reason, (long long)summary[5]);
    return reason;
}

}  // namespace

int main() {
    // rooms of six walls each, side by side: the walls of a dozen rooms make a workgroup
    for (int n_nodes : {2, 7, 20}) {
        Model rooms(1200, 6, n_nodes, false);
        const heat_batch_options always = options(2), never = options(1), plain = options(0);
        const int r_always = ask("rooms", rooms, always);
        expect(r_always == HEAT_IDEAL_RESIDENT_OK, "rooms of plain walls, resident always: eligible", r_always, n_nodes);
        expect(ask("rooms", rooms, never) == HEAT_IDEAL_RESIDENT_NONE_PLANNED, "no_fusion = 1 plans nothing resident", n_nodes);
        const int r_plain = ask("rooms", rooms, plain);  // (the cost model's choice: resident or not, never anything else)
        expect(r_plain == HEAT_IDEAL_RESIDENT_OK || r_plain == HEAT_IDEAL_RESIDENT_NONE_PLANNED, "rooms of plain walls, default options", r_plain, n_nodes);
        // per-node constants instead of palettes: nothing can march resident
        const heat_batch_options no_palette = options(2, 1);
        expect(ask("rooms without palettes", rooms, no_palette) == HEAT_IDEAL_RESIDENT_NONE_PLANNED, "without palettes nothing is resident", n_nodes);
        for (int npl : {4, 8, 16}) {
            const heat_batch_options lanes = options(2, 0, npl);
            // (walls of fewer nodes than a lane takes are not fast-path walls at that blocking factor: nothing resident then)
            const int r = ask("rooms, nodes per lane forced", rooms, lanes);
            expect(n_nodes < npl ? (r == HEAT_IDEAL_RESIDENT_OK || r == HEAT_IDEAL_RESIDENT_NONE_PLANNED) : r == HEAT_IDEAL_RESIDENT_OK,
                   "every blocking factor has its instantiation", n_nodes, npl);
        }
    }
    // every room joined to the next by an interior wall: one cluster, larger than a workgroup
    {
        Model chain(3000, 10, 12, true);
        const heat_batch_options always = options(2);
        const int r = ask("chain", chain, always);
        expect(r == HEAT_IDEAL_RESIDENT_TEAMS || r == HEAT_IDEAL_RESIDENT_NONE_PLANNED, "a cluster larger than a workgroup: teams or streamed", r);
    }
    // a NULL descriptor is refused, not dereferenced
    {
        int32_t reason = -7;
        const heat_batch_options opt = options(0);
        expect(heat_plan_ideal_resident(nullptr, &opt, 1, nullptr, &reason) < 0, "NULL descriptor");
        expect(reason == HEAT_IDEAL_RESIDENT_NONE_PLANNED, "the reason of a refused call", reason);
    }
    if (n_failed) {
        std::printf("%d check(s) failed\n", n_failed);
        return 1;
    }
    std::printf("ideal resident host check: every answer as the header states it\n");
    return 0;
}
