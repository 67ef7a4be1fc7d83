// air_species_host_main.cpp — a stand-alone driver of heat_air_species_check (include/heat_amd.h) for the sanitizers:
// tests/test_air_species_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model, a good term — two species, a lane of 500 sources and lanes
// without any, a zone of 300 vents and zones without any, the sources of one lane at both ends of the list, handlers whose
// branches the species' tables copy — and damaged ones: zones, species and channels out of range, values that are not finite,
// NULL arrays, lists of no length. Every call's status is checked against the header; the table builder and its verification
// run inside the check. No device, no HIP.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "heat_amd.h"

namespace {

int n_failed = 0;

void expect(int rc, int want, const char *needle, const char *what) {
    const char *msg = heat_last_error();
    const bool ok = rc == want && (needle == nullptr || (msg != nullptr && std::strstr(msg, needle) != nullptr));
    if (!ok) {
        std::printf("FAILED %s: status %d (expected %d), message \"%s\" (expected \"%s\")\n", what, rc, want, msg ? msg : "", needle ? needle : "");
        n_failed++;
    }
}

struct Model {
    int64_t S, Z;
    std::vector<int64_t> node_offset, slot[9], zone_slot;
    std::vector<double> mass, uvalue, alpha, zeros, ones, zone_volume;
    std::vector<int32_t> kind_front, kind_back, zone_front, zone_back;
    heat_batch_desc desc;
    Model(int64_t S_, int64_t Z_) : S(S_), Z(Z_) {
        const int64_t n_nodes = 2;
        node_offset.resize(S + 1);
        for (int64_t s = 0; s <= S; s++) node_offset[s] = n_nodes * s;
        mass.assign(n_nodes * S, 5000.0);
        uvalue.assign(n_nodes * S, 2.0);
        alpha.assign(n_nodes * S, 0.0);
        zeros.assign(S, 0.0);
        ones.assign(S, 1.0);
        kind_front.assign(S, HEAT_BOUNDARY_OUTDOOR);
        kind_back.assign(S, HEAT_BOUNDARY_SPACE);
        zone_front.assign(S, 0);
        zone_back.resize(S);
        for (int64_t s = 0; s < S; s++) zone_back[s] = (int32_t)(s % Z);
        // state: zones, then per surface 8 scalars and its nodes
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


constexpr int32_t kChannels = 8;  // 0, 1 volumes; 2 outdoor temperature; 3, 4 outdoor levels; 5 a source; 6 enable / occupancy; 7 limit

struct Species {
    int64_t Z;
    std::vector<int32_t> outdoor_chan, src_zone, src_species, src_chan, vent_zone, vent_species, vent_temp_chan, vent_enable_chan, limit_chan, occ_chan;
    std::vector<double> src_factor, v_min, v_max, c_lo, c_hi, conc, sum_conc, max_conc, excess_above, sum_volume, sum_q;
    std::vector<int64_t> n_occupied, step_max, n_above, steps_saturated;
    Species(int64_t n_species, int64_t Z_) : Z(Z_) {
        const size_t L = (size_t)(n_species * Z);
        outdoor_chan.resize(L);
        for (size_t l = 0; l < L; l++) outdoor_chan[l] = l % 5 == 0 ? -1 : 3 + (int32_t)(l % 2);
        limit_chan.assign((size_t)n_species, -1);
        limit_chan[0] = 7;
        occ_chan.resize((size_t)Z);
        for (int64_t z = 0; z < Z; z++) occ_chan[(size_t)z] = z % 3 == 0 ? -1 : 6;
        conc.assign(L, 400.0), sum_conc.assign(L, 0.0), max_conc.assign(L, 0.0), excess_above.assign(L, 0.0);
        n_occupied.assign(L, 0), step_max.assign(L, -1), n_above.assign(L, 0);
    }
    void source(int32_t z, int32_t s) {
        const size_t i = src_zone.size();
        src_zone.push_back(z), src_species.push_back(s), src_chan.push_back(5), src_factor.push_back(-1.0 + 0.01 * (double)(i % 300));
    }
    void vent(int32_t z, int32_t s) {
        const size_t j = vent_zone.size();
        vent_zone.push_back(z), vent_species.push_back(s), vent_temp_chan.push_back(2), vent_enable_chan.push_back(j % 2 ? 6 : -1);
        v_min.push_back(0.001 * (double)(j % 4)), v_max.push_back(0.001 * (double)(j % 4) + 0.01 * (double)(j % 7));
        c_lo.push_back(500.0 + (double)(j % 50)), c_hi.push_back(900.0 + (double)(j % 90));
        sum_volume.push_back(0.0), sum_q.push_back(0.0), steps_saturated.push_back(0);
    }
    heat_air_species view() {
        heat_air_species sp;
        std::memset(&sp, 0, sizeof sp);
        sp.n_species = (int64_t)limit_chan.size(), sp.n_sources = (int64_t)src_zone.size(), sp.n_vents = (int64_t)vent_zone.size();
        sp.outdoor_chan = outdoor_chan.data(), sp.src_zone = src_zone.data(), sp.src_species = src_species.data(), sp.src_chan = src_chan.data();
        sp.src_factor = src_factor.data(), sp.vent_zone = vent_zone.data(), sp.vent_species = vent_species.data();
        sp.vent_temp_chan = vent_temp_chan.data(), sp.vent_enable_chan = vent_enable_chan.data(), sp.vent_v_min = v_min.data();
        sp.vent_v_max = v_max.data(), sp.vent_c_lo = c_lo.data(), sp.vent_c_hi = c_hi.data(), sp.limit_chan = limit_chan.data();
        sp.occ_chan = occ_chan.data(), sp.resume = 1, sp.step_base = 1000, sp.conc = conc.data(), sp.n_occupied = n_occupied.data();
        sp.sum_conc = sum_conc.data(), sp.max_conc = max_conc.data(), sp.step_max = step_max.data(), sp.n_above = n_above.data();
        sp.excess_above = excess_above.data(), sp.sum_volume = sum_volume.data(), sp.sum_q = sum_q.data(), sp.steps_saturated = steps_saturated.data();
        return sp;
    }
};

}  // namespace

int main() {
    const int64_t S = 90, Z = 37, NS = 2;
    const int n_steps = 3;
    Model m(S, Z);
    std::vector<heat_weather> weather((size_t)n_steps, heat_weather{10.0, 0.0, 1.0});
    std::vector<double> channel((size_t)n_steps * kChannels, 20.0);
    heat_series s;
    std::memset(&s, 0, sizeof s);
    s.n_steps = n_steps, s.n_sub = 1, s.n_channels = kChannels;
    s.weather = weather.data(), s.channel = channel.data();
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // ---- the terms whose air the species ride on ----
    std::vector<int32_t> flow_zone = {3, 36, 0, 3}, flow_vol = {0, 1, 0, 1}, flow_temp = {2, 2, 2, 2};
    heat_zone_loads l;
    std::memset(&l, 0, sizeof l);
    l.n_flows = 4, l.flow_zone = flow_zone.data(), l.flow_volume_chan = flow_vol.data(), l.flow_temp_chan = flow_temp.data();
    std::vector<int32_t> target = {3, 4, 36}, source = {4, -1, 0}, temp_chan = {-1, 2, -1}, volume_chan = {0, 1, 0}, open_chan = {-1, 2, -1};
    std::vector<int8_t> sense = {1, 1, 1};
    std::vector<double> band = {0.0, 0.5, 0.0}, min_delta = {0.0, 0.1, 0.0};
    heat_air_paths air;
    std::memset(&air, 0, sizeof air);
    air.n_paths = 3, air.target = target.data(), air.source = source.data(), air.temp_chan = temp_chan.data(), air.volume_chan = volume_chan.data();
    air.open_chan = open_chan.data(), air.sense = sense.data(), air.band = band.data(), air.min_delta = min_delta.data();
    std::vector<int32_t> outdoor = {2, 2}, br_unit, br_zone, br_chan;
    std::vector<double> br_gain;
    for (int i = 0; i < 400; i++) br_unit.push_back(i % 2), br_zone.push_back(i % 30), br_chan.push_back(i % 2), br_gain.push_back(0.5 + 0.001 * i);
    heat_air_handlers h;
    std::memset(&h, 0, sizeof h);
    h.n_units = 2, h.outdoor_chan = outdoor.data(), h.n_branches = 400, h.br_unit = br_unit.data(), h.br_zone = br_zone.data();
    h.br_volume_chan = br_chan.data(), h.br_volume_gain = br_gain.data();

    // ---- a good term ----
    Species good(NS, Z);
    good.source(36, 1);                                                  // the last lane: its sources stand at both ends of the list
    for (int32_t z = 0; z < 30; z++)                                     // zones 30-35 have no source and no vent
        for (int32_t i = 0; i < 1 + z % 4; i++) good.source(z, (z + i) % 2);
    for (int i = 0; i < 500; i++) good.source(7, 0);                     // a lane of 500 sources
    good.source(36, 1);
    good.vent(36, 0);
    for (int32_t z = 0; z < 30; z += 2)
        for (int32_t i = 0; i < 1 + z % 3; i++) good.vent(z, (z + i) % 2);
    for (int i = 0; i < 300; i++) good.vent(11, i % 2);                  // a zone of 300 vents
    good.vent(36, 1);
    heat_air_species sp = good.view();
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &sp), HEAT_OK, nullptr, "a good term beside loads, paths and handlers");
    expect(heat_air_species_check(&m.desc, &s, nullptr, nullptr, nullptr, &sp), HEAT_OK, nullptr, "a good term alone");
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, nullptr), HEAT_OK, nullptr, "no term");
    sp.src_factor = nullptr, sp.vent_enable_chan = nullptr, sp.limit_chan = nullptr, sp.occ_chan = nullptr, sp.n_occupied = nullptr;
    sp.sum_conc = nullptr, sp.max_conc = nullptr, sp.step_max = nullptr, sp.n_above = nullptr, sp.excess_above = nullptr;
    sp.sum_volume = nullptr, sp.sum_q = nullptr, sp.steps_saturated = nullptr;
    heat_air_handlers plain = h;
    plain.br_volume_gain = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &plain, &sp), HEAT_OK, nullptr, "no factors, optional channels or accumulators");
    good.conc[5] = nan, good.conc[6] = inf;
    sp = good.view();
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &sp), HEAT_OK, nullptr, "a concentration that is not finite is data");

    // ---- lists of no length ----
    heat_air_species e;
    std::memset(&e, 0, sizeof e);
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_OK, nullptr, "an empty term");
    e = good.view();
    e.n_sources = 0, e.n_vents = 0;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_OK, nullptr, "species without sources or vents");
    e.n_species = 0;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_OK, nullptr, "arrays of no length");
    e = good.view();
    e.n_species = 0, e.n_vents = 0;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "species source 0", "sources without species");
    e = good.view();
    e.n_species = 0, e.n_sources = 0;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "demand vent 0", "vents without species");
    e = good.view();
    e.n_species = -1;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "air species", "a negative count of species");
    e = good.view();
    e.n_sources = -1;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "species source", "a negative count of sources");
    e = good.view();
    e.n_vents = -1;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "demand vent", "a negative count of vents");
    e = good.view();
    e.n_species = 1;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_SIZE, "species source 0:", "a source of a species past the count");

    // ---- NULLs ----
    e = good.view(), e.outdoor_chan = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "outdoor_chan", "NULL outdoor_chan");
    e = good.view(), e.conc = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "conc", "NULL conc");
    e = good.view(), e.src_zone = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "src_zone", "NULL src_zone");
    e = good.view(), e.src_species = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "src_species", "NULL src_species");
    e = good.view(), e.src_chan = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "src_chan", "NULL src_chan");
    e = good.view(), e.vent_zone = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "vent_zone", "NULL vent_zone");
    e = good.view(), e.vent_species = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "vent_species", "NULL vent_species");
    e = good.view(), e.vent_temp_chan = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "vent_temp_chan", "NULL vent_temp_chan");
    e = good.view(), e.vent_v_min = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "vent_v_min", "NULL vent_v_min");
    e = good.view(), e.vent_v_max = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "vent_v_max", "NULL vent_v_max");
    e = good.view(), e.vent_c_lo = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "vent_c_lo", "NULL vent_c_lo");
    e = good.view(), e.vent_c_hi = nullptr;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "vent_c_hi", "NULL vent_c_hi");
    expect(heat_air_species_check(&m.desc, nullptr, &l, &air, &h, &sp), HEAT_E_INVALID_ARG, "series", "NULL series");

    // ---- out of range ----
    {
        Species bad = good;
        bad.src_zone[40] = (int32_t)Z;
        e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_SIZE, "species source 40:", "a source's zone past the end");
        bad = good, bad.src_species[41] = -1, e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_SIZE, "species source 41:", "a negative species");
        bad = good, bad.src_chan[42] = kChannels, e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_SIZE, "species source 42:", "a source's channel past the end");
        bad = good, bad.vent_zone[9] = -1, e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_SIZE, "demand vent 9:", "a negative zone");
        bad = good, bad.vent_species[9] = 2, e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_SIZE, "demand vent 9:", "a vent's species past the end");
        bad = good, bad.vent_temp_chan[9] = -1, e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_SIZE, "demand vent 9:", "no temperature channel");
        bad = good, bad.vent_enable_chan[9] = -2, e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_SIZE, "demand vent 9:", "an enable channel below -1");
        bad = good, bad.outdoor_chan[(size_t)Z + 3] = kChannels, e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_SIZE, "air species 1:", "an outdoor channel past the end");
        bad = good, bad.limit_chan[1] = -2, e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_SIZE, "air species 1:", "a limit channel below -1");
        bad = good, bad.occ_chan[4] = kChannels + 5, e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_SIZE, "air species", "an occupancy channel past the end");
        // ---- values ----
        for (const double v : {nan, inf, -inf}) {
            bad = good, bad.src_factor[3] = v, e = bad.view();
            expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "species source 3:", "a factor that is not finite");
            bad = good, bad.v_min[5] = v, e = bad.view();
            expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "demand vent 5:", "a v_min that is not finite");
            bad = good, bad.v_max[5] = v, e = bad.view();
            expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "demand vent 5:", "a v_max that is not finite");
            bad = good, bad.c_lo[5] = v, e = bad.view();
            expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "demand vent 5:", "a c_lo that is not finite");
            bad = good, bad.c_hi[5] = v, e = bad.view();
            expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "demand vent 5:", "a c_hi that is not finite");
        }
        bad = good, bad.v_min[6] = -0.001, e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "demand vent 6:", "a negative v_min");
        bad = good, bad.v_max[6] = bad.v_min[6] - 1e-9, e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "demand vent 6:", "v_max below v_min");
        bad = good, bad.c_hi[6] = bad.c_lo[6], e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_E_INVALID_ARG, "demand vent 6:", "c_hi equal to c_lo");
        bad = good, bad.v_max[6] = bad.v_min[6], e = bad.view();
        expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &e), HEAT_OK, nullptr, "v_max equal to v_min: a constant vent");
    }
    // ---- the other terms are checked as their own checks do ----
    flow_zone[1] = (int32_t)Z;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &sp), HEAT_E_SIZE, nullptr, "a bad flow of the zone loads");
    flow_zone[1] = 36;
    target[2] = -1;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &sp), HEAT_E_SIZE, nullptr, "a bad air path");
    target[2] = 36;
    br_unit[7] = 2;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &sp), HEAT_E_SIZE, "air handler branch 7:", "a bad branch of the handlers");
    br_unit[7] = 1;
    expect(heat_air_species_check(&m.desc, &s, &l, &air, &h, &sp), HEAT_OK, nullptr, "the good term again");

    if (n_failed) {
        std::printf("%d checks failed\n", n_failed);
        return 1;
    }
    std::printf("air species host check: all statuses as the header states them\n");
    return 0;
}
