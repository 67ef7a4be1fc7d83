// comfort_host_main.cpp — a stand-alone driver of heat_comfort_check (include/heat_amd.h) for the sanitizers:
// tests/test_comfort_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model and a good comfort term — sensors with many, one and no entry,
// entries in a scrambled order, two sensors in one zone of which one controls, zones without a sensor, with and without the
// nullable arrays — and damaged copies: numbers out of range, weights that are not finite, a second control sensor on a zone,
// NULL arrays, step arrays without their extremum, lists of no length. Every call's status is checked against the header; the
// table builder (the counting sort and the CSR offsets) and its verification run inside the check. No device, no HIP.
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
        // walls of 1, 2 and 3 nodes in turn: the last node of a one-node wall is its first
        node_offset.resize(S + 1);
        node_offset[0] = 0;
        for (int64_t s = 0; s < S; s++) node_offset[s + 1] = node_offset[s] + 1 + s % 3;
        const int64_t n_nodes = node_offset[S];
        mass.assign(n_nodes, 5000.0);
        uvalue.assign(n_nodes, 2.0);
        alpha.assign(n_nodes, 0.0);
        zeros.assign(S, 0.0);
        ones.assign(S, 1.0);
        kind_front.assign(S, HEAT_BOUNDARY_OUTDOOR);
        kind_back.assign(S, HEAT_BOUNDARY_SPACE);
        zone_front.assign(S, 0);
        zone_back.resize(S);
        for (int64_t s = 0; s < S; s++) zone_back[s] = (int32_t)(s % Z);
        zone_slot.resize(Z);
        for (int64_t z = 0; z < Z; z++) zone_slot[z] = z;
        for (int a = 0; a < 9; a++) {
            slot[a].resize(S);
            for (int64_t s = 0; s < S; s++) slot[a][s] = Z + 8 * s + node_offset[s] + (a < 8 ? a : 8);
        }
        zone_volume.assign(Z, 300.0);
        std::memset(&desc, 0, sizeof desc);
        desc.abi_version = HEAT_AMD_ABI_VERSION;
        desc.n_surfaces = S, desc.n_zones = Z, desc.n_cavities = 0, desc.n_state = Z + 8 * S + n_nodes;
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

// n sensors: sensor i stands in zone i % (Z - 1) (the last zone has none; with n > Z - 1 some zones have two, of which the
// first controls); sensor 1 has no entry, sensor 2 has 130, the others a few; the entries are listed in a scrambled order
struct Comfort {
    int64_t n, ne;
    std::vector<int32_t> zone, en_sensor, occ, lo, hi;
    std::vector<int64_t> en_surface;
    std::vector<uint8_t> control, en_side;
    std::vector<double> air_weight, en_weight;
    std::vector<int64_t> i64[6];
    std::vector<double> f64[6];
    Comfort(int64_t n_, int64_t S, int64_t Z) : n(n_) {
        std::vector<int32_t> owner;
        for (int64_t i = 0; i < n; i++) {
            zone.push_back((int32_t)(i % (Z - 1)));
            control.push_back(i < Z - 1 && i % 2 == 0 ? 1 : 0);
            air_weight.push_back(i % 5 == 0 ? 0.0 : (i % 5 == 1 ? 1.0 : 0.1 * (double)(i % 10)));
            occ.push_back(i % 3 == 0 ? -1 : 0), lo.push_back(i % 4 == 0 ? -1 : 1), hi.push_back(i % 4 == 1 ? -1 : 2);
            const int64_t count = i == 1 ? 0 : (i == 2 ? 130 : 1 + i % 6);
            for (int64_t a = 0; a < count; a++) owner.push_back((int32_t)i);
        }
        ne = (int64_t)owner.size();
        en_sensor.resize((size_t)ne), en_surface.resize((size_t)ne), en_side.resize((size_t)ne), en_weight.resize((size_t)ne);
        for (int64_t j = 0; j < ne; j++) {
            const int64_t p = (j * 7919 + 13) % ne;  // (a permutation when ne and 7919 are coprime; checked below)
            en_sensor[(size_t)p] = owner[(size_t)j];
            en_surface[(size_t)p] = (j * 31) % S;
            en_side[(size_t)p] = (uint8_t)(j % 2);
            en_weight[(size_t)p] = j % 9 == 0 ? -0.25 : 0.01 * (double)(1 + j % 50);
        }
        for (auto &v : i64) v.assign((size_t)n, 3);
        for (auto &v : f64) v.assign((size_t)n, 2.5);
    }
    heat_comfort view() {
        heat_comfort c;
        std::memset(&c, 0, sizeof c);
        c.n_sensors = n, c.zone = zone.data(), c.air_weight = air_weight.data(), c.control = control.data();
        c.n_entries = ne, c.en_sensor = en_sensor.data(), c.en_surface = en_surface.data(), c.en_side = en_side.data();
        c.en_weight = en_weight.data(), c.occ_chan = occ.data(), c.lo_chan = lo.data(), c.hi_chan = hi.data();
        c.resume = 1, c.step_base = 40;
        c.n_occupied = i64[0].data(), c.step_min = i64[1].data(), c.step_max = i64[2].data(), c.n_below = i64[3].data();
        c.n_above = i64[4].data(), c.step_max_above = i64[5].data();
        c.sum_operative = f64[0].data(), c.min_operative = f64[1].data(), c.max_operative = f64[2].data(), c.deg_below = f64[3].data();
        c.deg_above = f64[4].data(), c.max_above = f64[5].data();
        return c;
    }
};

}  // namespace

int main() {
    const int64_t S = 333, Z = 7, NF = 300;
    const int n_steps = 3, NC = 3;
    Model m(S, Z);
    std::vector<heat_weather> weather((size_t)n_steps, heat_weather{10.0, 0.0, 1.0});
    std::vector<double> channel((size_t)n_steps * NC, 0.5);
    heat_series s;
    std::memset(&s, 0, sizeof s);
    s.n_steps = n_steps, s.n_sub = 1, s.n_channels = NC, s.channel = channel.data();
    s.weather = weather.data();
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
#define CHECK(cf) heat_comfort_check(&m.desc, &s, cf)

    // ---- a good term ----
    Comfort good(NF, S, Z);
    {
        std::vector<uint8_t> seen((size_t)good.ne, 0);
        for (int64_t j = 0; j < good.ne; j++) seen[(size_t)((j * 7919 + 13) % good.ne)] = 1;
        for (int64_t j = 0; j < good.ne; j++)
            if (!seen[(size_t)j]) std::printf("FAILED the scrambled order is no permutation (%lld entries)\n", (long long)good.ne), n_failed++;
    }
    heat_comfort c = good.view();
    expect(CHECK(&c), HEAT_OK, nullptr, "a good term");
    expect(CHECK(nullptr), HEAT_OK, nullptr, "no term");
    c.air_weight = nullptr, c.control = nullptr, c.occ_chan = nullptr, c.lo_chan = nullptr, c.hi_chan = nullptr;
    expect(CHECK(&c), HEAT_OK, nullptr, "no air weights, control bytes or channels");
    c = good.view();
    c.n_occupied = nullptr, c.sum_operative = nullptr, c.min_operative = nullptr, c.step_min = nullptr, c.max_operative = nullptr;
    c.step_max = nullptr, c.n_below = nullptr, c.deg_below = nullptr, c.n_above = nullptr, c.deg_above = nullptr, c.max_above = nullptr;
    c.step_max_above = nullptr;
    expect(CHECK(&c), HEAT_OK, nullptr, "no accumulators");
    c = good.view();
    c.step_min = nullptr, c.step_max = nullptr, c.step_max_above = nullptr;
    expect(CHECK(&c), HEAT_OK, nullptr, "extrema without their steps");
    c = good.view();
    c.n_entries = 0, c.en_sensor = nullptr, c.en_surface = nullptr, c.en_side = nullptr, c.en_weight = nullptr;
    expect(CHECK(&c), HEAT_OK, nullptr, "sensors without any entry");
    {
        Comfort one(1, S, Z);
        heat_comfort v = one.view();
        expect(CHECK(&v), HEAT_OK, nullptr, "one sensor");
    }

    // ---- lists of no length, counts, NULL arrays ----
    heat_comfort e;
    std::memset(&e, 0, sizeof e);
    expect(CHECK(&e), HEAT_OK, nullptr, "an empty term");
    e = good.view();
    e.n_sensors = -1;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "comfort sensor", "a negative count of sensors");
    e = good.view();
    e.n_entries = -1;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "comfort entry", "a negative count of entries");
    e = good.view();
    e.zone = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "comfort sensor 0", "zone NULL");
    {
        const char *const name[4] = {"en_sensor", "en_surface", "en_side", "en_weight"};
        for (int a = 0; a < 4; a++) {
            e = good.view();
            if (a == 0) e.en_sensor = nullptr;
            if (a == 1) e.en_surface = nullptr;
            if (a == 2) e.en_side = nullptr;
            if (a == 3) e.en_weight = nullptr;
            expect(CHECK(&e), HEAT_E_INVALID_ARG, name[a], "an entry array NULL");
            expect(CHECK(&e), HEAT_E_INVALID_ARG, "comfort entry 0", "an entry array NULL names the entry");
        }
    }
    e = good.view();
    e.min_operative = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "step_min", "step_min without min_operative");
    e = good.view();
    e.max_operative = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "step_max", "step_max without max_operative");
    e = good.view();
    e.max_above = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "step_max_above", "step_max_above without max_above");

    // ---- values ----
    for (const double bad : {nan, inf, -inf}) {
        Comfort d(NF, S, Z);
        d.en_weight[77] = bad;
        heat_comfort v = d.view();
        expect(CHECK(&v), HEAT_E_INVALID_ARG, "comfort entry 77:", "a weight that is not finite");
    }
    for (const double bad : {nan, inf, -inf, -1e-9, 1.0 + 1e-9}) {
        Comfort d(NF, S, Z);
        d.air_weight[255] = bad;
        heat_comfort v = d.view();
        expect(CHECK(&v), HEAT_E_INVALID_ARG, "comfort sensor 255:", "an air weight outside [0, 1] or not finite");
    }
    {
        Comfort d(NF, S, Z);
        d.control[9] = 2;
        heat_comfort v = d.view();
        expect(CHECK(&v), HEAT_E_INVALID_ARG, "comfort sensor 9:", "a control byte above 1");
    }

    // ---- numbers out of range ----
    for (const int32_t bad : {-1, (int32_t)Z, INT32_MAX}) {
        Comfort d(NF, S, Z);
        d.zone[299] = bad;
        heat_comfort v = d.view();
        expect(CHECK(&v), HEAT_E_SIZE, "comfort sensor 299:", "a zone out of range");
    }
    for (const int32_t bad : {-2, (int32_t)NC, INT32_MAX}) {
        for (int a = 0; a < 3; a++) {
            Comfort d(NF, S, Z);
            (a == 0 ? d.occ : (a == 1 ? d.lo : d.hi))[64] = bad;
            heat_comfort v = d.view();
            expect(CHECK(&v), HEAT_E_SIZE, "comfort sensor 64:", "a channel out of range");
        }
    }
    for (const int32_t bad : {-1, (int32_t)NF, INT32_MAX}) {
        Comfort d(NF, S, Z);
        d.en_sensor[500] = bad;
        heat_comfort v = d.view();
        expect(CHECK(&v), HEAT_E_SIZE, "comfort entry 500:", "a sensor out of range");
    }
    for (const int64_t bad : {(int64_t)-1, S, (int64_t)1 << 40}) {
        Comfort d(NF, S, Z);
        d.en_surface[0] = bad;
        heat_comfort v = d.view();
        expect(CHECK(&v), HEAT_E_SIZE, "comfort entry 0:", "a surface out of range");
    }
    {
        Comfort d(NF, S, Z);
        d.en_side[good.ne - 1] = 2;
        heat_comfort v = d.view();
        char who[64];
        std::snprintf(who, sizeof who, "comfort entry %lld:", (long long)(good.ne - 1));
        expect(CHECK(&v), HEAT_E_SIZE, who, "a side above 1");
    }
    {
        Comfort d(NF, S, Z);
        d.control[6] = 1;  // sensors 0 and 6 stand in zone 0, and sensor 0 controls it already
        heat_comfort v = d.view();
        expect(CHECK(&v), HEAT_E_SIZE, "comfort sensor 6:", "a second control sensor on a zone");
        d.control[0] = 0;  // ... the other one alone is fine
        v = d.view();
        expect(CHECK(&v), HEAT_OK, nullptr, "the second sensor of a zone controls it");
    }
    {
        heat_comfort v = good.view();  // no sensor: the term is absent, its entries are not read
        v.n_sensors = 0;
        expect(CHECK(&v), HEAT_OK, nullptr, "entries without sensors");
    }
    expect(heat_comfort_check(&m.desc, nullptr, &c), HEAT_E_INVALID_ARG, "series", "no series");

    if (n_failed) {
        std::printf("%d checks failed\n", n_failed);
        return 1;
    }
    std::printf("comfort host check: all statuses as the header states them\n");
    return 0;
}
