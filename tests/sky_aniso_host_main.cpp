// sky_aniso_host_main.cpp — a stand-alone driver of heat_sky_aniso_check (include/heat_amd.h) and of the checks
// heat_batch_march_series_call makes of its struct (heat_amd/csrc/plan.hpp, check_series_call) for the sanitizers:
// tests/test_sky_aniso_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model of two sites, a sky, a few apertures, shades, a coefficient table
// and bands of exactly the lengths the header gives — a read past any of them is the sanitizer's to find — and damaged copies:
// bands that are negative or not finite on consumers that read them and on consumers that do not, NULL tables, bands without
// their term, a struct of another size. Every call's status is checked against the header. No device, no HIP.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "heat_amd.h"
#include "../heat_amd/csrc/plan.hpp"

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

// n shades: walls turning round the compass, without horizon profiles
struct Shades {
    int64_t n;
    std::vector<int64_t> surface;
    std::vector<double> col[19];
    std::vector<int32_t> front, back, aperture;
    Shades(int64_t n_, int64_t S, int64_t n_apertures) : n(n_) {
        for (int64_t j = 0; j < n; j++) {
            const double az = 0.37 * (double)j;
            const double v[19] = {std::cos(az), std::sin(az), 0.0, -std::sin(az), std::cos(az), 0.0, 0.0, 0.0, 1.0, 1.2 + 0.01 * (double)j,
                                  1.5,          0.6,          0.2, 0.3,           0.0,          0.0, 0.1, 0.8, 0.9};
            surface.push_back((j * 7) % S);
            for (int a = 0; a < 19; a++) col[a].push_back(v[a]);
        }
        front.assign((size_t)S, -1);
        back.assign((size_t)S, -1);
        aperture.assign((size_t)n_apertures, -1);
    }
    heat_shades view() {
        heat_shades h;
        std::memset(&h, 0, sizeof h);
        h.n_shades = n;
        h.sh_surface = surface.data();
        const double **dst[19] = {&h.sh_normal_x, &h.sh_normal_y, &h.sh_normal_z, &h.sh_right_x, &h.sh_right_y, &h.sh_right_z, &h.sh_up_x,
                                  &h.sh_up_y, &h.sh_up_z, &h.sh_width, &h.sh_height, &h.overhang_depth, &h.overhang_gap, &h.fin_pos_depth,
                                  &h.fin_pos_gap, &h.fin_neg_depth, &h.fin_neg_gap, &h.diffuse_factor, &h.ground_factor};
        for (int a = 0; a < 19; a++) *dst[a] = col[a].data();
        h.front_shade = front.data(), h.back_shade = back.data(), h.aperture_shade = aperture.data();
        return h;
    }
};

// The coefficient table and the four bands, each of exactly its length
struct Aniso {
    std::vector<heat_sky_coef> coef;
    std::vector<double> front, back, aperture, shade;
    Aniso(int n_steps, int n_sites, int64_t S, int64_t NA, int64_t NS) {
        for (int i = 0; i < n_steps * n_sites; i++) coef.push_back(heat_sky_coef{0.1 + 0.05 * i, 0.02 * i});
        for (int64_t q = 0; q < S; q++) front.push_back(0.01 * (double)(q % 90)), back.push_back(q % 4 ? 0.5 : 0.0);
        for (int64_t a = 0; a < NA; a++) aperture.push_back(1.0 - 0.1 * (double)a);
        for (int64_t j = 0; j < NS; j++) shade.push_back(j % 3 ? 0.8 : 0.0);
    }
    heat_sky_aniso view() {
        heat_sky_aniso a;
        std::memset(&a, 0, sizeof a);
        a.coef = coef.data(), a.front_band = front.data(), a.back_band = back.data();
        a.aperture_band = aperture.data(), a.shade_band = shade.data();
        return a;
    }
};

}  // namespace

int main() {
    const int64_t S = 333, Z = 7, NA = 9, NS = 70;
    const int n_steps = 3, n_sites = 2, NC = 3;
    Model m(S, Z);
    std::vector<heat_weather> weather((size_t)n_steps * n_sites, heat_weather{10.0, 0.0, 1.0});
    std::vector<int32_t> none(S, -1);
    std::vector<double> channel((size_t)n_steps * NC, 0.5);
    heat_series s;
    std::memset(&s, 0, sizeof s);
    s.n_steps = n_steps, s.n_sub = 1, s.n_channels = NC, s.channel = channel.data();
    s.weather = weather.data();
    s.solar_front_chan = none.data(), s.solar_back_chan = none.data();
    std::vector<heat_sky_record> record((size_t)n_steps * n_sites, heat_sky_record{0.6, 0.0, 0.8, 700.0, 100.0, 30.0, 350.0, 400.0});
    std::vector<uint8_t> mode(S, 0);
    for (int64_t q = 0; q < S; q++) mode[q] = (uint8_t)(q % 4);  // surface 4n: nothing; 4n + 1: front; 4n + 2: back; 4n + 3: both
    std::vector<double> normal(S, 0.5);
    heat_sky sky;
    std::memset(&sky, 0, sizeof sky);
    sky.record = record.data(), sky.mode = mode.data();
    sky.normal_x = normal.data(), sky.normal_y = normal.data(), sky.normal_z = normal.data();
    std::vector<int64_t> ap_surface;
    for (int64_t a = 0; a < NA; a++) ap_surface.push_back(a * 30);
    std::vector<double> ap_one(NA, 1.0), ap_coef(6 * NA, 0.1);
    heat_solar_gains g;
    std::memset(&g, 0, sizeof g);
    g.n_apertures = NA, g.ap_surface = ap_surface.data();
    g.ap_normal_x = ap_one.data(), g.ap_normal_y = ap_one.data(), g.ap_normal_z = ap_one.data();
    g.ap_tau_coef = ap_coef.data(), g.ap_tau_diffuse = ap_one.data(), g.ap_scale = ap_one.data();
    Shades shades(NS, S, NA);
    for (int64_t q = 0; q < S; q++) {
        if (mode[q] & 1) shades.front[q] = (int32_t)(q % NS);
        if (mode[q] & 2) shades.back[q] = (int32_t)((q * 3) % NS);
    }
    for (int64_t a = 0; a < NA; a++) shades.aperture[a] = a % 2 ? (int32_t)(a * 5) : -1;
    heat_shades h = shades.view();
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
#define CHECK(an) heat_sky_aniso_check(&m.desc, n_sites, &s, &sky, &g, &h, an)

    // ---- good ----
    Aniso good(n_steps, n_sites, S, NA, NS);
    heat_sky_aniso a = good.view();
    expect(CHECK(&a), HEAT_OK, nullptr, "a good anisotropic sky");
    expect(CHECK(nullptr), HEAT_OK, nullptr, "no anisotropic sky");
    a.front_band = nullptr, a.back_band = nullptr, a.aperture_band = nullptr, a.shade_band = nullptr;
    expect(CHECK(&a), HEAT_OK, nullptr, "no bands: zeros");
    a = good.view();
    expect(heat_sky_aniso_check(&m.desc, n_sites, &s, &sky, nullptr, nullptr, &a), HEAT_E_INVALID_ARG, "aperture_band", "an aperture band without gains");
    a.aperture_band = nullptr;
    expect(heat_sky_aniso_check(&m.desc, n_sites, &s, &sky, nullptr, nullptr, &a), HEAT_E_INVALID_ARG, "shade_band", "a shade band without shades");
    a.shade_band = nullptr;
    expect(heat_sky_aniso_check(&m.desc, n_sites, &s, &sky, nullptr, nullptr, &a), HEAT_OK, nullptr, "sides alone");

    // ---- what the coefficients need ----
    a = good.view();
    expect(heat_sky_aniso_check(&m.desc, n_sites, &s, nullptr, nullptr, nullptr, &a), HEAT_E_INVALID_ARG, "sky is NULL", "no sky");
    {
        heat_sky bare = sky;
        bare.record = nullptr;
        std::vector<uint8_t> off(S, 0);
        bare.mode = off.data();
        expect(heat_sky_aniso_check(&m.desc, n_sites, &s, &bare, nullptr, nullptr, &a), HEAT_E_INVALID_ARG, "sky->record is NULL", "a sky without records");
    }
    a.coef = nullptr;
    expect(CHECK(&a), HEAT_E_INVALID_ARG, "coef is NULL", "NULL coef");
    {
        heat_series empty = s;
        empty.n_steps = 0;
        expect(heat_sky_aniso_check(&m.desc, n_sites, &empty, &sky, &g, &h, &a), HEAT_OK, nullptr, "NULL coef of a series of no steps");
    }
    {   // the coefficients are the caller's: not checked
        Aniso d(n_steps, n_sites, S, NA, NS);
        d.coef[1] = heat_sky_coef{nan, -inf};
        a = d.view();
        expect(CHECK(&a), HEAT_OK, nullptr, "coefficients that are not finite");
    }

    // ---- bands ----
    for (double bad : {nan, inf, -inf, -1e-9}) {
        Aniso d(n_steps, n_sites, S, NA, NS);
        d.front[4] = bad, d.front[6] = bad;  // (mode 0 and mode 2: the front's band is not read)
        d.back[8] = bad, d.back[9] = bad;    // (mode 0 and mode 1)
        a = d.view();
        expect(CHECK(&a), HEAT_OK, nullptr, "bad bands on sides that do not read them");
        d.front[5] = bad;
        a = d.view();
        expect(CHECK(&a), HEAT_E_INVALID_ARG, "surface 5:", "a bad front band");
        d.front[5] = 0.0, d.back[331] = bad;  // (mode 3)
        a = d.view();
        expect(CHECK(&a), HEAT_E_INVALID_ARG, "surface 331:", "a bad back band");
        d.back[331] = 0.0, d.aperture[NA - 1] = bad;
        a = d.view();
        expect(CHECK(&a), HEAT_E_INVALID_ARG, "aperture 8:", "a bad aperture band");
        d.aperture[NA - 1] = 0.0, d.shade[NS - 1] = bad;
        a = d.view();
        expect(CHECK(&a), HEAT_E_INVALID_ARG, "shade 69:", "a bad shade band");
    }
    // ---- the terms' own refusals come first ----
    {
        Shades d(NS, S, NA);
        d.col[9][3] = -1.0;
        heat_shades bad = d.view();
        a = good.view();
        expect(heat_sky_aniso_check(&m.desc, n_sites, &s, &sky, &g, &bad, &a), HEAT_E_INVALID_ARG, "shade 3:", "bad shades under a good anisotropic sky");
    }

    // ---- the struct of heat_batch_march_series_call ----
    {
        std::string &err = heat::last_error();
        expect(heat::check_series_call(nullptr, err), HEAT_E_INVALID_ARG, "series call is NULL", "a NULL call");
        heat_series_call call;
        std::memset(&call, 0, sizeof call);
        expect(heat::check_series_call(&call, err), HEAT_E_INVALID_ARG, "size 0", "a call that was not sized");
        call.size = sizeof call - sizeof(void *);
        expect(heat::check_series_call(&call, err), HEAT_E_INVALID_ARG, "sizeof(heat_series_call)", "a call of an older size");
        call.size = sizeof call + sizeof(void *);
        expect(heat::check_series_call(&call, err), HEAT_E_INVALID_ARG, "sizeof(heat_series_call)", "a call of a newer size");
        call.size = sizeof call;
        expect(heat::check_series_call(&call, err), HEAT_E_INVALID_ARG, "s is NULL", "a call without a series");
        call.s = &s;
        expect(heat::check_series_call(&call, err), HEAT_OK, nullptr, "a good call");
        {   // a smaller struct on the heap, as an older caller would pass it: only its size field is read
            const size_t small = sizeof(size_t);
            heat_series_call *old = static_cast<heat_series_call *>(std::malloc(small));
            std::memcpy(old, &small, small);
            expect(heat::check_series_call(old, err), HEAT_E_INVALID_ARG, "size 8", "a call of eight bytes");
            std::free(old);
        }
    }
    if (n_failed) {
        std::printf("%d checks failed\n", n_failed);
        return 1;
    }
    std::printf("sky aniso host check: all statuses as the header states them\n");
    return 0;
}
