// openings_host_main.cpp — a stand-alone driver of heat_openings_check (include/heat_amd.h) for the sanitizers:
// tests/test_openings_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model, a good term — 699 openings to outside and between zones, with and
// without wind and open-fraction channels, every derived channel written once — and damaged ones: zones and channels out of
// range, a side with two temperatures or none, coefficients that are negative or not finite, NULL arrays, lists of no length,
// derived channels written twice or read by an opening. Every call's status is checked against the header; the table builder
// and its verification run inside the check. No device, no HIP.
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

constexpr int32_t kInputs = 6;  // 0, 1 outside temperatures; 2, 3 wind speeds; 4, 5 open fractions; the derived channels follow

struct Openings {
    std::vector<int32_t> zone_a, zone_b, temp_chan, wind_chan, frac_chan, out_chan;
    std::vector<double> area, cw, cs, ca, c0, sum_v, max_v;
    std::vector<int64_t> step_max;
    Openings(int64_t n, int64_t Z) {
        for (int64_t i = 0; i < n; i++) {
            const bool outside = i % 3 != 0;
            const int32_t a = (int32_t)(i % Z);
            zone_a.push_back(a), zone_b.push_back(outside ? -1 : (int32_t)((a + 1 + i % 5) % Z));
            temp_chan.push_back(outside ? (int32_t)(i % 2) : -1);
            wind_chan.push_back(i % 4 == 0 ? -1 : 2 + (int32_t)(i % 2)), frac_chan.push_back(i % 5 == 0 ? -1 : 4 + (int32_t)(i % 2));
            out_chan.push_back(kInputs + (int32_t)((i * 7) % n));  // (7 and n = 699 share no factor: every derived channel once)
            area.push_back(0.01 * (double)(i % 9)), cw.push_back(0.001 * (double)(i % 3)), cs.push_back(2.0 * (double)(i % 4));
            ca.push_back(0.0035 * (double)(i % 2)), c0.push_back(0.01 * (double)(i % 2));
            sum_v.push_back(0.0), max_v.push_back(0.0), step_max.push_back(-1);
        }
    }
    heat_openings view() {
        heat_openings op;
        std::memset(&op, 0, sizeof op);
        op.n_openings = (int64_t)zone_a.size();
        op.zone_a = zone_a.data(), op.zone_b = zone_b.data(), op.temp_chan = temp_chan.data(), op.wind_chan = wind_chan.data();
        op.frac_chan = frac_chan.data(), op.out_chan = out_chan.data(), op.area = area.data(), op.cw = cw.data(), op.cs = cs.data();
        op.ca = ca.data(), op.c0 = c0.data(), op.resume = 1, op.step_base = 1000;
        op.sum_v = sum_v.data(), op.max_v = max_v.data(), op.step_max = step_max.data();
        return op;
    }
};

}  // namespace

int main() {
    const int64_t S = 90, Z = 37, N = 699;  // (699 = 3 * 233 shares no factor with 7)
    const int32_t n_channels = kInputs + (int32_t)N;
    const int n_steps = 3;
    Model m(S, Z);
    std::vector<heat_weather> weather((size_t)n_steps, heat_weather{10.0, 0.0, 1.0});
    std::vector<double> channel((size_t)n_steps * n_channels, 20.0);
    heat_series s;
    std::memset(&s, 0, sizeof s);
    s.n_steps = n_steps, s.n_sub = 1, s.n_channels = n_channels;
    s.weather = weather.data(), s.channel = channel.data();
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // ---- a good term ----
    Openings good(N, Z);
    heat_openings op = good.view(), e;
    expect(heat_openings_check(&m.desc, &s, &op), HEAT_OK, nullptr, "a good term");
    expect(heat_openings_check(&m.desc, &s, nullptr), HEAT_OK, nullptr, "no term");
    op.wind_chan = nullptr, op.frac_chan = nullptr, op.cw = nullptr, op.cs = nullptr, op.ca = nullptr, op.c0 = nullptr;
    op.sum_v = nullptr, op.max_v = nullptr, op.step_max = nullptr;
    expect(heat_openings_check(&m.desc, &s, &op), HEAT_OK, nullptr, "no optional channels, coefficients or accumulators");
    {
        Openings inner(N, Z);
        for (size_t i = 0; i < (size_t)N; i++) inner.zone_b[i] = (inner.zone_a[i] + 1) % (int32_t)Z, inner.temp_chan[i] = -1;
        e = inner.view(), e.temp_chan = nullptr;
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_OK, nullptr, "zone-to-zone openings only: no temperature channels");
    }

    // ---- lists of no length ----
    std::memset(&e, 0, sizeof e);
    expect(heat_openings_check(&m.desc, &s, &e), HEAT_OK, nullptr, "an empty term");
    e = good.view(), e.n_openings = 0;
    expect(heat_openings_check(&m.desc, &s, &e), HEAT_OK, nullptr, "arrays of no length");
    e = good.view(), e.n_openings = -1;
    expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "opening", "a negative count");
    e = good.view(), e.n_openings = 1;
    expect(heat_openings_check(&m.desc, &s, &e), HEAT_OK, nullptr, "the first opening alone");

    // ---- NULLs ----
    e = good.view(), e.zone_a = nullptr;
    expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "opening 0: zone_a", "NULL zone_a");
    e = good.view(), e.zone_b = nullptr;
    expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "opening 0: zone_b", "NULL zone_b");
    e = good.view(), e.out_chan = nullptr;
    expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "opening 0: out_chan", "NULL out_chan");
    e = good.view(), e.area = nullptr;
    expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "opening 0: area", "NULL area");
    e = good.view(), e.temp_chan = nullptr;
    expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 1:", "NULL temp_chan beside an opening to outside");
    expect(heat_openings_check(&m.desc, nullptr, &op), HEAT_E_INVALID_ARG, "series", "NULL series");

    // ---- out of range, sides, values, derived channels ----
    {
        Openings bad = good;
        bad.zone_a[40] = (int32_t)Z, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 40:", "zone_a past the end");
        bad = good, bad.zone_a[41] = -1, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 41:", "a negative zone_a");
        bad = good, bad.zone_b[42] = (int32_t)Z, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 42:", "zone_b past the end");
        bad = good, bad.zone_b[43] = -2, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 43:", "zone_b below -1");
        bad = good, bad.zone_b[45] = bad.zone_a[45], bad.temp_chan[45] = -1, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "opening 45:", "zone_a equal to zone_b");
        bad = good, bad.out_chan[46] = n_channels, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 46:", "out_chan past the end");
        bad = good, bad.out_chan[46] = -1, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 46:", "a negative out_chan");
        bad = good, bad.temp_chan[46] = -1, e = bad.view();      // 46 % 3 != 0: an opening to outside
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 46:", "outside air without a temperature channel");
        bad = good, bad.temp_chan[46] = n_channels, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 46:", "a temperature channel past the end");
        bad = good, bad.temp_chan[45] = 0, e = bad.view();       // 45 % 3 == 0: zone to zone
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 45:", "a temperature channel on a zone-to-zone opening");
        bad = good, bad.wind_chan[47] = -2, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 47:", "a wind channel below -1");
        bad = good, bad.wind_chan[47] = n_channels, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 47:", "a wind channel past the end");
        bad = good, bad.frac_chan[48] = -2, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 48:", "an open-fraction channel below -1");
        bad = good, bad.frac_chan[48] = n_channels + 3, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 48:", "an open-fraction channel past the end");
        for (const double v : {nan, inf, -inf, -1e-300}) {
            std::vector<double> Openings::*const coef[5] = {&Openings::area, &Openings::cw, &Openings::cs, &Openings::ca, &Openings::c0};
            for (auto member : coef) {
                bad = good, (bad.*member)[5] = v, e = bad.view();
                expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "opening 5:", "an area or coefficient that is negative or not finite");
            }
        }
        bad = good, bad.area[5] = 0.0, bad.c0[5] = 0.0, e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_OK, nullptr, "an area and a coefficient of zero");
        bad = good, bad.out_chan[600] = bad.out_chan[3], e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 600:", "two openings with one derived channel");
        bad = good, bad.temp_chan[46] = bad.out_chan[698], e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 46:", "a temperature channel that is a derived channel");
        bad = good, bad.wind_chan[47] = bad.out_chan[0], e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 47:", "a wind channel that is a derived channel");
        bad = good, bad.frac_chan[48] = bad.out_chan[48], e = bad.view();
        expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 48:", "an open-fraction channel that is the opening's own derived channel");
    }
    s.n_channels = 0;
    e = good.view();
    expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_SIZE, "opening 0:", "a series without channels");
    s.n_channels = -1;
    expect(heat_openings_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "n_channels", "a negative count of channels");
    s.n_channels = n_channels;
    op = good.view();
    expect(heat_openings_check(&m.desc, &s, &op), HEAT_OK, nullptr, "the good term again");

    if (n_failed) {
        std::printf("%d checks failed\n", n_failed);
        return 1;
    }
    std::printf("openings host check: all statuses as the header states them\n");
    return 0;
}
