// shades_host_main.cpp — a stand-alone driver of heat_shades_check (include/heat_amd.h) for the sanitizers:
// tests/test_shades_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model, a sky, a few apertures and a good set of shades — with and
// without horizon profiles, factors and index arrays — and damaged ones: numbers out of range, values that are not finite or
// of the wrong sign, NULL arrays, lists of no length. Every call's status is checked against the header; the table builder
// runs inside the check. No device, no HIP.
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

// n shades: walls turning round the compass, every third one with a horizon profile
struct Shades {
    int64_t n;
    std::vector<int64_t> surface;
    std::vector<double> col[19];
    std::vector<int32_t> horizon, front, back, aperture;
    std::vector<double> tan2;
    Shades(int64_t n_, int64_t S, int64_t n_apertures, int64_t n_horizons) : n(n_) {
        for (int64_t j = 0; j < n; j++) {
            const double az = 0.37 * (double)j;
            const double v[19] = {std::cos(az), std::sin(az), 0.0, -std::sin(az), std::cos(az), 0.0, 0.0, 0.0, 1.0, 1.2 + 0.01 * (double)j,
                                  1.5,          0.6,          0.2, 0.3,           0.0,          0.0, 0.1, 0.8, 0.9};
            surface.push_back((j * 7) % S);
            for (int a = 0; a < 19; a++) col[a].push_back(v[a]);
            horizon.push_back(j % 3 == 0 ? (int32_t)(j % n_horizons) : -1);
        }
        tan2.assign((size_t)(16 * n_horizons), 0.04);
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
        h.sh_horizon = horizon.data();
        h.n_horizons = (int64_t)(tan2.size() / 16);
        h.horizon_tan2 = tan2.data();
        h.front_shade = front.data(), h.back_shade = back.data(), h.aperture_shade = aperture.data();
        return h;
    }
};

}  // namespace

int main() {
    const int64_t S = 333, Z = 7, NA = 9, NS = 70, NH = 4;
    const int n_steps = 3, n_sites = 2;
    Model m(S, Z);
    std::vector<heat_weather> weather((size_t)n_steps * n_sites, heat_weather{10.0, 0.0, 1.0});
    std::vector<int32_t> none(S, -1);
    heat_series s;
    std::memset(&s, 0, sizeof s);
    s.n_steps = n_steps, s.n_sub = 1, s.n_channels = 0;
    s.weather = weather.data();
    s.solar_front_chan = none.data(), s.solar_back_chan = none.data();
    std::vector<heat_sky_record> record((size_t)n_steps * n_sites, heat_sky_record{0.6, 0.0, 0.8, 700.0, 100.0, 30.0, 350.0, 400.0});
    std::vector<uint8_t> mode(S, 0);
    for (int64_t q = 0; q < S; q++) mode[q] = (uint8_t)(q % 4);  // 0: nothing, 1: solar front, 2: solar back, 3: both
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

    // ---- good shades ----
    Shades good(NS, S, NA, NH);
    for (int64_t q = 0; q < S; q++) {
        if (mode[q] & 1) good.front[q] = (int32_t)(q % NS);
        if (mode[q] & 2) good.back[q] = (int32_t)((q * 3) % NS);
    }
    for (int64_t a = 0; a < NA; a++) good.aperture[a] = a % 2 ? (int32_t)(a * 5) : -1;
    heat_shades h = good.view();
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &h), HEAT_OK, nullptr, "good shades");
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, nullptr), HEAT_OK, nullptr, "no shades");
    h.diffuse_factor = nullptr, h.ground_factor = nullptr, h.sh_horizon = nullptr;
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &h), HEAT_OK, nullptr, "no factors, no horizon numbers");
    h.front_shade = nullptr, h.back_shade = nullptr, h.aperture_shade = nullptr, h.n_horizons = 0, h.horizon_tan2 = nullptr;
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &h), HEAT_OK, nullptr, "shades nobody refers to");
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, nullptr, &h), HEAT_OK, nullptr, "shades without gains");

    // ---- lists of no length ----
    heat_shades e;
    std::memset(&e, 0, sizeof e);
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_OK, nullptr, "empty shades");
    expect(heat_shades_check(&m.desc, n_sites, &s, nullptr, nullptr, &e), HEAT_OK, nullptr, "empty shades without a sky");
    e = good.view();
    e.n_shades = -1;
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_INVALID_ARG, "shade", "a negative shade count");
    e = good.view();
    e.n_horizons = -2;
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_INVALID_ARG, "horizon", "a negative horizon count");
    e = good.view();
    e.n_shades = 0;  // the sides still refer to shades
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_SIZE, "surface 1:", "sides that refer to shades there are none of");

    // ---- NULLs ----
    e = good.view();
    e.sh_surface = nullptr;
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_INVALID_ARG, "sh_surface", "NULL sh_surface");
    e = good.view();
    e.sh_up_y = nullptr;
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_INVALID_ARG, "sh_up_y", "NULL sh_up_y");
    e = good.view();
    e.fin_neg_gap = nullptr;
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_INVALID_ARG, "fin_neg_gap", "NULL fin_neg_gap");
    e = good.view();
    e.horizon_tan2 = nullptr;
    expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_INVALID_ARG, "horizon 0", "NULL horizon_tan2");
    e = good.view();
    e.front_shade = nullptr, e.back_shade = nullptr;
    expect(heat_shades_check(&m.desc, n_sites, &s, nullptr, nullptr, &e), HEAT_E_INVALID_ARG, "sky is NULL", "shades without a sky");
    {
        std::vector<uint8_t> no_mode(S, 0);  // (a sky that drives nothing needs no records of its own)
        heat_sky no_record = sky;
        no_record.record = nullptr, no_record.mode = no_mode.data();
        e.front_shade = nullptr, e.back_shade = nullptr;
        expect(heat_shades_check(&m.desc, n_sites, &s, &no_record, nullptr, &e), HEAT_E_INVALID_ARG, "sky->record is NULL", "shades without records");
        e = good.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, nullptr, &e), HEAT_E_INVALID_ARG, "aperture 0", "aperture_shade without gains");
    }

    // ---- values ----
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int a = 0; a < 19; a++)
        for (double bad : {nan, inf, -inf}) {
            Shades d(NS, S, NA, NH);
            d.col[a][41] = bad;
            e = d.view();
            expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_INVALID_ARG, "shade 41:", "a value that is not finite");
        }
    for (int a = 9; a < 17; a++) {
        Shades d(NS, S, NA, NH);
        d.col[a][13] = -0.25;
        e = d.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_INVALID_ARG, "shade 13:", "a negative length");
    }
    for (int a = 9; a < 11; a++) {
        Shades d(NS, S, NA, NH);
        d.col[a][69] = 0.0;
        e = d.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_INVALID_ARG, "shade 69:", "a width or height of zero");
    }
    for (double bad : {nan, inf, -1e-3}) {
        Shades d(NS, S, NA, NH);
        d.tan2[16 * 2 + 15] = bad;
        e = d.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_INVALID_ARG, "horizon 2:", "a bad tan2");
    }

    // ---- numbers out of range ----
    for (int64_t bad : {(int64_t)-1, S, S + 100000}) {
        Shades d(NS, S, NA, NH);
        d.surface[5] = bad;
        e = d.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_SIZE, "shade 5:", "a surface out of range");
    }
    for (int32_t bad : {(int32_t)-2, (int32_t)NH, INT32_MAX}) {
        Shades d(NS, S, NA, NH);
        d.horizon[6] = bad;
        e = d.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_SIZE, "shade 6:", "a horizon out of range");
    }
    for (int32_t bad : {(int32_t)-2, (int32_t)NS, INT32_MAX}) {
        Shades d(NS, S, NA, NH);
        d.front[201] = bad;  // (mode 1: its front is sky-driven)
        e = d.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_SIZE, "surface 201:", "a front shade out of range");
        d.front[201] = -1, d.back[202] = bad;
        e = d.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_SIZE, "surface 202:", "a back shade out of range");
        d.back[202] = -1, d.aperture[8] = bad;
        e = d.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_SIZE, "aperture 8:", "an aperture shade out of range");
    }
    {
        Shades d(NS, S, NA, NH);
        d.front[202] = 3;  // mode 2: only the back is sky-driven
        e = d.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_SIZE, "surface 202:", "a front shade without the sky bit");
        d.front[202] = -1, d.back[201] = 3;
        e = d.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_SIZE, "surface 201:", "a back shade without the sky bit");
        d.back[201] = -1, d.back[200] = 0;  // mode 0
        e = d.view();
        expect(heat_shades_check(&m.desc, n_sites, &s, &sky, &g, &e), HEAT_E_SIZE, "surface 200:", "a shade on a surface the sky does not drive");
    }
    if (n_failed) {
        std::printf("%d checks failed\n", n_failed);
        return 1;
    }
    std::printf("shades host check: all statuses as the header states them\n");
    return 0;
}
