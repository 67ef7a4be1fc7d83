// blinds_host_main.cpp — a stand-alone driver of heat_blinds_check (include/heat_amd.h) for the sanitizers:
// tests/test_blinds_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model, a sky, a few apertures, shades and a good set of blinds of every
// kind — scheduled, controlled, gated by a zone, with an enable channel, with and without the nullable arrays — and damaged
// copies: numbers out of range, a shade named twice, values that are not finite or of the wrong sign, thresholds in the wrong
// order, NULL arrays, lists of no length. Every call's status is checked against the header; the table builder and its
// verification run inside the check. No device, no HIP.
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


// n blinds on shades in a scrambled order; kind i % 4: scheduled, controlled, controlled and gated by a zone, the same with an
// enable channel
struct Blinds {
    int64_t n;
    std::vector<int32_t> shade, pos_chan, zone, set_chan, enable_chan;
    std::vector<double> closed[3], irr_close, irr_open, band, sum_position;
    std::vector<uint8_t> state;
    std::vector<int64_t> steps_closed, switches;
    Blinds(int64_t n_, int64_t n_shades, int64_t Z) : n(n_) {
        for (int64_t i = 0; i < n; i++) {
            const int kind = (int)(i % 4);
            shade.push_back((int32_t)((i * 37 + 11) % n_shades));  // (37 and n_shades = 70 are coprime: no shade twice)
            pos_chan.push_back(kind == 0 ? 0 : -1);
            zone.push_back(kind >= 2 ? (int32_t)(i % Z) : -1);
            set_chan.push_back(kind >= 2 ? 1 : -1);
            enable_chan.push_back(kind == 3 ? 2 : -1);
            for (int a = 0; a < 3; a++) closed[a].push_back(i % 5 == 0 ? 0.0 : (i % 7 == 0 ? 1.0 : 0.1 * (a + 1)));
            irr_close.push_back(250.0 + (double)i), irr_open.push_back(120.0);
            band.push_back(i % 6 == 2 ? 0.0 : 0.5);
            state.push_back((uint8_t)(i % 2));
        }
        steps_closed.assign((size_t)n, 3), switches.assign((size_t)n, 1), sum_position.assign((size_t)n, 2.5);
    }
    heat_blinds view() {
        heat_blinds b;
        std::memset(&b, 0, sizeof b);
        b.n_blinds = n, b.shade = shade.data();
        b.beam_closed = closed[0].data(), b.diffuse_closed = closed[1].data(), b.ground_closed = closed[2].data();
        b.pos_chan = pos_chan.data(), b.irr_close = irr_close.data(), b.irr_open = irr_open.data();
        b.zone = zone.data(), b.set_chan = set_chan.data(), b.band = band.data(), b.enable_chan = enable_chan.data();
        b.state = state.data(), b.steps_closed = steps_closed.data(), b.switches = switches.data(), b.sum_position = sum_position.data();
        return b;
    }
};

}  // namespace

int main() {
    const int64_t S = 333, Z = 7, NA = 9, NS = 70, NH = 4, NB = 45;
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
    for (int64_t q = 0; q < S; q++) mode[q] = (uint8_t)(q % 4);
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
    Shades shades(NS, S, NA, NH);
    for (int64_t q = 0; q < S; q++) {
        if (mode[q] & 1) shades.front[q] = (int32_t)(q % NS);
        if (mode[q] & 2) shades.back[q] = (int32_t)((q * 3) % NS);
    }
    for (int64_t a = 0; a < NA; a++) shades.aperture[a] = a % 2 ? (int32_t)(a * 5) : -1;
    heat_shades h = shades.view();
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
#define CHECK(bl) heat_blinds_check(&m.desc, n_sites, &s, &sky, &g, &h, bl)

    // ---- good blinds ----
    Blinds good(NB, NS, Z);
    heat_blinds b = good.view();
    expect(CHECK(&b), HEAT_OK, nullptr, "good blinds");
    expect(CHECK(nullptr), HEAT_OK, nullptr, "no blinds");
    b.state = nullptr, b.steps_closed = nullptr, b.switches = nullptr, b.sum_position = nullptr;
    expect(CHECK(&b), HEAT_OK, nullptr, "no state, no accumulators");
    b.enable_chan = nullptr;
    expect(CHECK(&b), HEAT_OK, nullptr, "no enable channels");
    {
        Blinds d(NB, NS, Z);  // every blind controlled and without a zone: pos_chan, zone, set_chan and band may be NULL
        b = d.view();
        b.pos_chan = nullptr, b.zone = nullptr, b.set_chan = nullptr, b.band = nullptr;
        expect(CHECK(&b), HEAT_OK, nullptr, "controlled blinds without a room condition");
        std::fill(d.pos_chan.begin(), d.pos_chan.end(), 1);  // every blind scheduled: the thresholds may be NULL
        std::fill(d.zone.begin(), d.zone.end(), -1);
        b = d.view();
        b.irr_close = nullptr, b.irr_open = nullptr, b.set_chan = nullptr, b.band = nullptr;
        expect(CHECK(&b), HEAT_OK, nullptr, "scheduled blinds without thresholds");
    }

    // ---- lists of no length, counts ----
    heat_blinds e;
    std::memset(&e, 0, sizeof e);
    expect(CHECK(&e), HEAT_OK, nullptr, "empty blinds");
    expect(heat_blinds_check(&m.desc, n_sites, &s, nullptr, nullptr, nullptr, &e), HEAT_OK, nullptr, "empty blinds without shades");
    e = good.view();
    e.n_blinds = -1;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "blind", "a negative count");
    e = good.view();
    expect(heat_blinds_check(&m.desc, n_sites, &s, &sky, &g, nullptr, &e), HEAT_E_INVALID_ARG, "blind 0", "blinds without shades");
    {
        heat_shades empty;
        std::memset(&empty, 0, sizeof empty);
        expect(heat_blinds_check(&m.desc, n_sites, &s, &sky, &g, &empty, &e), HEAT_E_INVALID_ARG, "blind 0", "blinds on shades of no length");
    }

    // ---- NULLs ----
    e = good.view(), e.shade = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "shade is NULL", "NULL shade");
    e = good.view(), e.beam_closed = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "beam_closed", "NULL beam_closed");
    e = good.view(), e.diffuse_closed = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "diffuse_closed", "NULL diffuse_closed");
    e = good.view(), e.ground_closed = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "ground_closed", "NULL ground_closed");
    e = good.view(), e.irr_close = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "blind 1:", "NULL irr_close with a controlled blind");
    e = good.view(), e.irr_open = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "blind 1:", "NULL irr_open with a controlled blind");
    e = good.view(), e.set_chan = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "blind 2:", "NULL set_chan with a gated blind");
    e = good.view(), e.band = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "blind 2:", "NULL band with a gated blind");

    // ---- values ----
    for (int a = 0; a < 3; a++)
        for (double bad : {nan, inf, -inf, -1e-9}) {
            Blinds d(NB, NS, Z);
            d.closed[a][31] = bad;
            e = d.view();
            expect(CHECK(&e), HEAT_E_INVALID_ARG, "blind 31:", "a closed factor that is negative or not finite");
        }
    for (double bad : {nan, inf, -inf}) {
        Blinds d(NB, NS, Z);
        d.irr_close[9] = bad;  // (controlled)
        e = d.view();
        expect(CHECK(&e), HEAT_E_INVALID_ARG, "blind 9:", "irr_close not finite");
        d.irr_close[9] = 250.0, d.irr_open[10] = bad;
        e = d.view();
        expect(CHECK(&e), HEAT_E_INVALID_ARG, "blind 10:", "irr_open not finite");
        d.irr_open[10] = 120.0, d.irr_close[8] = bad, d.irr_open[8] = bad;  // (scheduled: not read)
        e = d.view();
        expect(CHECK(&e), HEAT_OK, nullptr, "thresholds of a scheduled blind are not read");
    }
    {
        Blinds d(NB, NS, Z);
        d.irr_open[13] = 1000.0;
        e = d.view();
        expect(CHECK(&e), HEAT_E_INVALID_ARG, "blind 13:", "irr_open above irr_close");
        d.irr_open[13] = d.irr_close[13];
        e = d.view();
        expect(CHECK(&e), HEAT_OK, nullptr, "irr_open equal to irr_close");
    }
    for (double bad : {nan, inf, -0.5}) {
        Blinds d(NB, NS, Z);
        d.band[14] = bad;  // (gated)
        e = d.view();
        expect(CHECK(&e), HEAT_E_INVALID_ARG, "blind 14:", "a bad band");
        d.band[14] = 0.5, d.band[13] = bad;  // (no zone: not read)
        e = d.view();
        expect(CHECK(&e), HEAT_OK, nullptr, "the band of a blind without a zone is not read");
    }
    {
        Blinds d(NB, NS, Z);
        d.state[44] = 2;
        e = d.view();
        expect(CHECK(&e), HEAT_E_INVALID_ARG, "blind 44:", "a state byte above 1");
    }

    // ---- numbers out of range ----
    for (int32_t bad : {(int32_t)-1, (int32_t)NS, INT32_MAX}) {
        Blinds d(NB, NS, Z);
        d.shade[5] = bad;
        e = d.view();
        expect(CHECK(&e), HEAT_E_SIZE, "blind 5:", "a shade out of range");
    }
    {
        Blinds d(NB, NS, Z);
        d.shade[40] = d.shade[3];
        e = d.view();
        expect(CHECK(&e), HEAT_E_SIZE, "blind 40:", "a shade named twice");
    }
    for (int32_t bad : {(int32_t)-2, (int32_t)Z, INT32_MAX}) {
        Blinds d(NB, NS, Z);
        d.zone[6] = bad;
        e = d.view();
        expect(CHECK(&e), HEAT_E_SIZE, "blind 6:", "a zone out of range");
    }
    for (int32_t bad : {(int32_t)-2, (int32_t)NC, INT32_MAX}) {
        Blinds d(NB, NS, Z);
        d.pos_chan[7] = bad;
        e = d.view();
        expect(CHECK(&e), HEAT_E_SIZE, "blind 7:", "a position channel out of range");
        d.pos_chan[7] = -1, d.enable_chan[11] = bad;
        e = d.view();
        expect(CHECK(&e), HEAT_E_SIZE, "blind 11:", "an enable channel out of range");
    }
    for (int32_t bad : {(int32_t)-1, (int32_t)NC, INT32_MAX}) {
        Blinds d(NB, NS, Z);
        d.set_chan[18] = bad;  // (gated)
        e = d.view();
        expect(CHECK(&e), HEAT_E_SIZE, "blind 18:", "a setpoint channel out of range");
    }
    // ---- the shades' own refusals come first ----
    {
        Shades d(NS, S, NA, NH);
        d.col[9][3] = -1.0;
        heat_shades bad = d.view();
        e = good.view();
        expect(heat_blinds_check(&m.desc, n_sites, &s, &sky, &g, &bad, &e), HEAT_E_INVALID_ARG, "shade 3:", "bad shades under good blinds");
    }
    if (n_failed) {
        std::printf("%d checks failed\n", n_failed);
        return 1;
    }
    std::printf("blinds host check: all statuses as the header states them\n");
    return 0;
}
