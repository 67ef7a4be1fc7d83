// solar_gains_host_main.cpp — a stand-alone driver of heat_solar_gains_check (include/heat_amd.h) for the sanitizers:
// tests/test_solar_gains_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model, a good set of gains — receivers with one entry and with
// hundreds, entries of one receiver far apart in the list, slices without a full 64 receivers — and damaged ones: indices
// out of range, values that are not finite, NULL arrays, lists of no length. Every call's status is checked against the
// header; the table builder and its verification run inside the check. No device, no HIP.
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

struct Gains {
    std::vector<int64_t> ap_surface, en_surface;
    std::vector<double> nx, ny, nz, coef, tau, scale, sum, beam, diffuse;
    std::vector<uint8_t> side;
    std::vector<int32_t> aperture;
    void add_aperture(int64_t surface) {
        const double k = (double)ap_surface.size();
        ap_surface.push_back(surface);
        nx.push_back(std::cos(k)), ny.push_back(std::sin(k)), nz.push_back(0.0);
        for (int j = 0; j < 6; j++) coef.push_back(j == 0 ? 0.7 : 0.01 * j);
        tau.push_back(0.6), scale.push_back(2.0 + k), sum.push_back(0.0);
    }
    void add_entry(int64_t surface, int s, int32_t ap, double b, double d) {
        en_surface.push_back(surface), side.push_back((uint8_t)s), aperture.push_back(ap), beam.push_back(b), diffuse.push_back(d);
    }
    heat_solar_gains view() {
        heat_solar_gains g;
        std::memset(&g, 0, sizeof g);
        g.n_apertures = (int64_t)ap_surface.size();
        g.ap_surface = ap_surface.data(), g.ap_normal_x = nx.data(), g.ap_normal_y = ny.data(), g.ap_normal_z = nz.data();
        g.ap_tau_coef = coef.data(), g.ap_tau_diffuse = tau.data(), g.ap_scale = scale.data(), g.ap_sum = sum.data();
        g.n_entries = (int64_t)en_surface.size();
        g.en_surface = en_surface.data(), g.en_side = side.data(), g.en_aperture = aperture.data();
        g.en_beam = beam.data(), g.en_diffuse = diffuse.data();
        return g;
    }
};

}  // namespace

int main() {
    const int64_t S = 333, Z = 7;
    const int n_steps = 3, n_sites = 2;
    Model m(S, Z);
    std::vector<heat_weather> weather((size_t)n_steps * n_sites, heat_weather{10.0, 0.0, 1.0});
    std::vector<double> channel((size_t)n_steps * 2, 100.0);
    std::vector<int32_t> chan_front(S, -1), chan_back(S, -1);
    chan_front[200] = 1;  // surface 200's front is channel-driven
    heat_series s;
    std::memset(&s, 0, sizeof s);
    s.n_steps = n_steps, s.n_sub = 1, s.n_channels = 2;
    s.weather = weather.data(), s.channel = channel.data();
    s.solar_front_chan = chan_front.data(), s.solar_back_chan = chan_back.data();
    std::vector<heat_sky_record> record((size_t)n_steps * n_sites, heat_sky_record{0.6, 0.0, 0.8, 700.0, 100.0, 30.0, 350.0, 400.0});
    std::vector<uint8_t> mode(S, 0);
    mode[201] = 2;  // surface 201's back takes its solar input from the sky
    std::vector<double> normal(S, 0.0);
    heat_sky sky;
    std::memset(&sky, 0, sizeof sky);
    sky.record = record.data(), sky.mode = mode.data();
    sky.normal_x = normal.data(), sky.normal_y = normal.data(), sky.normal_z = normal.data();

    // ---- a good model ----
    Gains good;
    for (int64_t a = 0; a < 40; a++) good.add_aperture((a * 8) % S);
    for (int64_t q = 0; q < S; q++) {  // every back but the sky's, from the apertures of its zone (at least one each)
        if (q == 201) continue;
        for (int32_t a = (int32_t)(q % Z); a < 40; a += (int32_t)Z) good.add_entry(q, 1, a, 0.01 * (a + 1), 0.02);
    }
    good.add_entry(5, 0, 3, 0.5, 0.25);                                          // a receiver with exactly one entry
    for (int i = 0; i < 700; i++) good.add_entry(77, 0, i % 40, 1e-3 * i, 0.5);  // a receiver with hundreds
    good.add_entry(0, 1, 39, 0.125, 0.0);                                        // far from surface 0's other entries
    heat_solar_gains g = good.view();
    expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &g), HEAT_OK, nullptr, "a good model");
    expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, nullptr), HEAT_OK, nullptr, "no gains");
    g.ap_sum = nullptr;
    expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &g), HEAT_OK, nullptr, "no ap_sum");

    // ---- lists of no length ----
    heat_solar_gains e;
    std::memset(&e, 0, sizeof e);
    expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_OK, nullptr, "empty gains");
    expect(heat_solar_gains_check(&m.desc, n_sites, &s, nullptr, &e), HEAT_OK, nullptr, "empty gains without a sky");
    e = good.view();
    e.n_entries = 0;
    expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_OK, nullptr, "apertures without entries");
    e.en_surface = nullptr, e.en_side = nullptr, e.en_aperture = nullptr, e.en_beam = nullptr, e.en_diffuse = nullptr;
    expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_OK, nullptr, "apertures without entry arrays");
    e = good.view();
    e.n_apertures = 0;
    expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "entry 0", "entries without apertures");
    e = good.view();
    e.n_apertures = -1;
    expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "aperture", "a negative aperture count");
    e = good.view();
    e.n_entries = -5;
    expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "entry", "a negative entry count");

    // ---- NULLs ----
    {
        e = good.view();
        e.ap_surface = nullptr;
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "ap_surface", "NULL ap_surface");
        e = good.view();
        e.ap_tau_coef = nullptr;
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "ap_tau_coef", "NULL ap_tau_coef");
        e = good.view();
        e.en_side = nullptr;
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "en_side", "NULL en_side");
        e = good.view();
        e.en_diffuse = nullptr;
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "en_diffuse", "NULL en_diffuse");
        e = good.view();
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, nullptr, &e), HEAT_E_INVALID_ARG, "aperture 0", "apertures without a sky");
        heat_sky no_record = sky;
        no_record.record = nullptr;
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &no_record, &e), HEAT_E_INVALID_ARG, "record", "apertures without records");
        heat_series none = s;
        none.n_steps = 0;
        expect(heat_solar_gains_check(&m.desc, n_sites, &none, &no_record, &e), HEAT_OK, nullptr, "no steps need no records");
    }

    // ---- values that are not finite ----
    const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                           -std::numeric_limits<double>::infinity()};
    for (double v : bad) {
        std::vector<double> *ap_arrays[6] = {&good.nx, &good.ny, &good.nz, &good.tau, &good.scale, &good.coef};
        for (std::vector<double> *a : ap_arrays) {
            const size_t at = a == &good.coef ? 6 * 17 + 4 : 17;
            const double keep = (*a)[at];
            (*a)[at] = v;
            e = good.view();
            expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "aperture 17:", "an aperture value that is not finite");
            (*a)[at] = keep;
        }
        std::vector<double> *en_arrays[2] = {&good.beam, &good.diffuse};
        for (std::vector<double> *a : en_arrays) {
            const double keep = (*a)[123];
            (*a)[123] = v;
            e = good.view();
            expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "entry 123:", "a share that is not finite");
            (*a)[123] = keep;
        }
    }

    // ---- indices out of range, a side above 1, an input with two sources ----
    const int64_t bad_surface[4] = {-1, S, S + 100000, INT64_MIN};
    for (int64_t q : bad_surface) {
        const int64_t keep_a = good.ap_surface[9], keep_e = good.en_surface[1000];
        good.ap_surface[9] = q;
        e = good.view();
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "aperture 9:", "an aperture's surface out of range");
        good.ap_surface[9] = keep_a;
        good.en_surface[1000] = q;
        e = good.view();
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "entry 1000:", "an entry's surface out of range");
        good.en_surface[1000] = keep_e;
    }
    const int32_t bad_aperture[4] = {-1, 40, INT32_MAX, INT32_MIN};
    for (int32_t a : bad_aperture) {
        const int32_t keep = good.aperture[55];
        good.aperture[55] = a;
        e = good.view();
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "entry 55:", "an entry's aperture out of range");
        good.aperture[55] = keep;
    }
    {
        const uint8_t keep = good.side[60];
        good.side[60] = 2;
        e = good.view();
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "entry 60:", "a side above 1");
        good.side[60] = 255;
        e = good.view();
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "entry 60:", "a side of 255");
        good.side[60] = keep;
        const size_t last = good.en_surface.size();
        good.add_entry(200, 0, 1, 0.1, 0.1);
        e = good.view();
        char name[32];
        std::snprintf(name, sizeof name, "entry %zu:", last);
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, name, "a receiver that has a channel");
        good.en_surface[last] = 201, good.side[last] = 1;
        e = good.view();
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, name, "a receiver that has a sky bit");
        good.side[last] = 0;  // surface 201's front is free
        e = good.view();
        expect(heat_solar_gains_check(&m.desc, n_sites, &s, &sky, &e), HEAT_OK, nullptr, "the other side of a sky-driven surface");
    }
    if (n_failed) {
        std::printf("%d checks FAILED\n", n_failed);
        return 1;
    }
    std::printf("solar gains host check: all statuses as the header states them\n");
    return 0;
}
