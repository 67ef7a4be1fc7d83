// air_handlers_host_main.cpp — a stand-alone driver of heat_air_handlers_check (include/heat_amd.h) for the sanitizers:
// tests/test_air_handlers_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model, a good term — a unit of 700 branches, a unit without any, a unit
// that only extracts and one that only supplies, a zone supplied by many units and zones by none, the branches of one unit at
// both ends of the list — and damaged ones: units, zones and channels out of range, values that are not finite, NULL arrays,
// lists of no length. Every call's status is checked against the header; the table builder and its verification run inside
// the check. No device, no HIP.
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

constexpr int32_t kChannels = 8;  // 0, 1 volumes; 2 outdoor; 3 effectiveness; 4 bypass setpoint; 5, 6 supply limits; 7 spare

struct Handlers {
    std::vector<int32_t> outdoor_chan, eff_chan, bypass_chan, heat_chan, cool_chan, br_unit, br_zone, br_volume_chan;
    std::vector<double> eff_gain, band, min_delta, heat_cap, cool_cap, br_gain, sum_recovered, sum_heating, sum_cooling, sum_branch_q;
    std::vector<uint8_t> br_kind, bypass;
    std::vector<int64_t> steps_bypass, switches, heat_sat, cool_sat;
    // every second unit bypasses, every third has a heating coil, every fourth a cooling coil
    void unit() {
        const size_t u = outdoor_chan.size();
        outdoor_chan.push_back(2), eff_chan.push_back(u % 2 ? 3 : -1), eff_gain.push_back(0.5 + 0.01 * (double)(u % 40));
        bypass_chan.push_back(u % 2 == 0 ? 4 : -1), band.push_back(0.1 * (double)(u % 5)), min_delta.push_back(0.05 * (double)(u % 3));
        heat_chan.push_back(u % 3 == 0 ? 5 : -1), cool_chan.push_back(u % 4 == 0 ? 6 : -1);
        heat_cap.push_back(u % 5 == 0 ? std::numeric_limits<double>::infinity() : 100.0 * (double)(u % 7));
        cool_cap.push_back(u % 7 == 0 ? std::numeric_limits<double>::infinity() : 50.0 * (double)(u % 3));
        bypass.push_back((uint8_t)(u % 2)), sum_recovered.push_back(0.0), sum_heating.push_back(0.0), sum_cooling.push_back(0.0);
        steps_bypass.push_back(0), switches.push_back(0), heat_sat.push_back(0), cool_sat.push_back(0);
    }
    void branch(int32_t u, int32_t z, uint8_t kind) {
        const size_t j = br_unit.size();
        br_unit.push_back(u), br_zone.push_back(z), br_volume_chan.push_back((int32_t)(j % 2));
        br_gain.push_back(0.5 + 0.001 * (double)(j % 1000)), br_kind.push_back(kind), sum_branch_q.push_back(0.0);
    }
    heat_air_handlers view() {
        heat_air_handlers h;
        std::memset(&h, 0, sizeof h);
        h.n_units = (int64_t)outdoor_chan.size(), h.n_branches = (int64_t)br_unit.size();
        h.outdoor_chan = outdoor_chan.data(), h.eff_chan = eff_chan.data(), h.eff_gain = eff_gain.data(), h.bypass_chan = bypass_chan.data();
        h.bypass_band = band.data(), h.bypass_min_delta = min_delta.data(), h.heat_chan = heat_chan.data(), h.cool_chan = cool_chan.data();
        h.heat_cap = heat_cap.data(), h.cool_cap = cool_cap.data(), h.br_unit = br_unit.data(), h.br_zone = br_zone.data();
        h.br_volume_chan = br_volume_chan.data(), h.br_volume_gain = br_gain.data(), h.br_kind = br_kind.data(), h.bypass = bypass.data();
        h.sum_recovered = sum_recovered.data(), h.sum_heating = sum_heating.data(), h.sum_cooling = sum_cooling.data();
        h.steps_bypass = steps_bypass.data(), h.switches = switches.data(), h.steps_heat_saturated = heat_sat.data();
        h.steps_cool_saturated = cool_sat.data(), h.sum_branch_q = sum_branch_q.data();
        return h;
    }
};

}  // namespace

int main() {
    const int64_t S = 90, Z = 37;
    const int32_t U = 24;
    const int n_steps = 3;
    Model m(S, Z);
    std::vector<heat_weather> weather((size_t)n_steps, heat_weather{10.0, 0.0, 1.0});
    std::vector<double> channel((size_t)n_steps * kChannels, 20.0);
    heat_series s;
    std::memset(&s, 0, sizeof s);
    s.n_steps = n_steps, s.n_sub = 1, s.n_channels = kChannels;
    s.weather = weather.data(), s.channel = channel.data();

    // ---- a good term ----
    Handlers good;
    for (int32_t u = 0; u < U; u++) good.unit();
    good.branch(U - 1, 0, 3);                                            // the last unit: its branches stand at both ends of the list
    good.branch(U - 1, 36, 1);
    for (int32_t u = 0; u < U - 1; u++) {                                // unit 5 has no branch, 6 only extracts, 7 only supplies
        if (u == 5) continue;
        for (int32_t i = 0; i < 1 + u % 6; i++)
            good.branch(u, (u * 5 + i * 3) % 30, u == 6 ? (uint8_t)2 : (u == 7 ? (uint8_t)1 : (uint8_t)(1 + (u + i) % 3)));
        good.branch(u, 33, 1);                                           // zone 33 is supplied by every unit; zones 30-32, 34, 35 by none
    }
    for (int i = 0; i < 700; i++) good.branch(11, i % 30, (uint8_t)(1 + i % 3));   // a unit of 700 branches
    good.branch(0, 36, 3);                                               // far from unit 0's other branches
    good.branch(U - 1, 1, 2);
    heat_air_handlers h = good.view();
    expect(heat_air_handlers_check(&m.desc, &s, &h), HEAT_OK, nullptr, "a good term");
    expect(heat_air_handlers_check(&m.desc, &s, nullptr), HEAT_OK, nullptr, "no term");
    h.bypass = nullptr, h.sum_recovered = nullptr, h.sum_heating = nullptr, h.sum_cooling = nullptr, h.steps_bypass = nullptr;
    h.switches = nullptr, h.steps_heat_saturated = nullptr, h.steps_cool_saturated = nullptr, h.sum_branch_q = nullptr;
    h.eff_gain = nullptr, h.eff_chan = nullptr, h.heat_cap = nullptr, h.cool_cap = nullptr, h.br_volume_gain = nullptr, h.br_kind = nullptr;
    expect(heat_air_handlers_check(&m.desc, &s, &h), HEAT_OK, nullptr, "no state, accumulators, gains, capacities or kinds");
    h.bypass_chan = nullptr, h.bypass_band = nullptr, h.bypass_min_delta = nullptr, h.heat_chan = nullptr, h.cool_chan = nullptr;
    expect(heat_air_handlers_check(&m.desc, &s, &h), HEAT_OK, nullptr, "no bypass and no coil");

    // ---- lists of no length ----
    heat_air_handlers e;
    std::memset(&e, 0, sizeof e);
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_OK, nullptr, "an empty term");
    e = good.view();
    e.n_branches = 0;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_OK, nullptr, "units without branches");
    e.n_units = 0;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_OK, nullptr, "arrays of no length");
    e = good.view();
    e.n_units = 0;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "air handler branch 0", "branches without units");
    e = good.view();
    e.n_units = -1;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "air handler", "a negative count of units");
    e = good.view();
    e.n_branches = -1;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "air handler branch", "a negative count of branches");
    e = good.view();
    e.n_units = U - 1;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_SIZE, "air handler branch 0:", "a branch of a unit past the count");

    // ---- NULLs ----
    e = good.view();
    e.outdoor_chan = nullptr;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "outdoor_chan", "NULL outdoor_chan");
    e = good.view();
    e.br_unit = nullptr;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "br_unit", "NULL br_unit");
    e = good.view();
    e.br_zone = nullptr;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "br_zone", "NULL br_zone");
    e = good.view();
    e.br_volume_chan = nullptr;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "br_volume_chan", "NULL br_volume_chan");
    e = good.view();
    e.bypass_band = nullptr;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "air handler 0:", "NULL bypass_band with a bypass");
    e = good.view();
    e.bypass_min_delta = nullptr;
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "bypass_min_delta", "NULL bypass_min_delta with a bypass");

    // ---- values that are not finite or negative, a bad kind, a bad bypass byte ----
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double bad[3] = {nan, inf, -inf};
    for (double v : bad) {
        std::vector<double> *arrays[3] = {&good.eff_gain, &good.band, &good.min_delta};
        for (std::vector<double> *arr : arrays) {
            const double keep = (*arr)[12];  // (unit 12 bypasses)
            (*arr)[12] = v;
            e = good.view();
            expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "air handler 12:", "a unit's value that is not finite");
            (*arr)[12] = keep;
        }
        const double keep = good.br_gain[300];
        good.br_gain[300] = v;
        e = good.view();
        expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "air handler branch 300:", "a branch gain that is not finite");
        good.br_gain[300] = keep;
    }
    {
        std::vector<double> *arrays[2] = {&good.band, &good.min_delta};
        for (std::vector<double> *arr : arrays) {
            const double keep = (*arr)[12];
            (*arr)[12] = -0.25;
            e = good.view();
            expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "air handler 12:", "a negative band or min_delta");
            (*arr)[12] = keep;
            (*arr)[13] = -0.25;  // (unit 13 has no bypass: not read)
            e = good.view();
            expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_OK, nullptr, "a negative band on a unit without a bypass");
            (*arr)[13] = 0.0;
        }
        std::vector<double> *caps[2] = {&good.heat_cap, &good.cool_cap};
        for (std::vector<double> *arr : caps) {
            const double bad_cap[3] = {-1.0, nan, -inf};
            for (double v : bad_cap) {
                const double keep = (*arr)[9];
                (*arr)[9] = v;
                e = good.view();
                expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "air handler 9:", "a negative or NaN capacity");
                (*arr)[9] = keep;
            }
            const double keep = (*arr)[9];
            (*arr)[9] = inf;
            e = good.view();
            expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_OK, nullptr, "a capacity of +inf");
            (*arr)[9] = 0.0;
            e = good.view();
            expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_OK, nullptr, "a capacity of 0");
            (*arr)[9] = keep;
        }
        const uint8_t bad_kind[3] = {0, 4, 255};
        for (uint8_t v : bad_kind) {
            const uint8_t keep = good.br_kind[77];
            good.br_kind[77] = v;
            e = good.view();
            expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "air handler branch 77:", "a kind outside 1..3");
            good.br_kind[77] = keep;
        }
        const uint8_t bad_state[2] = {2, 255};
        for (uint8_t v : bad_state) {
            const uint8_t keep = good.bypass[17];
            good.bypass[17] = v;
            e = good.view();
            expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_INVALID_ARG, "air handler 17:", "a bypass byte above 1");
            good.bypass[17] = keep;
        }
    }

    // ---- units, zones and channels out of range ----
    const int32_t bad_index[4] = {-1, 1000, INT32_MAX, INT32_MIN};
    for (int32_t v : bad_index) {
        int32_t keep = good.br_unit[40];
        good.br_unit[40] = v;
        e = good.view();
        expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_SIZE, "air handler branch 40:", "a unit out of range");
        good.br_unit[40] = keep;
        keep = good.br_zone[41];
        good.br_zone[41] = v;
        e = good.view();
        expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_SIZE, "air handler branch 41:", "a zone out of range");
        good.br_zone[41] = keep;
        keep = good.br_volume_chan[42];
        good.br_volume_chan[42] = v;
        e = good.view();
        expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_SIZE, "air handler branch 42:", "a volume channel out of range");
        good.br_volume_chan[42] = keep;
        keep = good.outdoor_chan[3];
        good.outdoor_chan[3] = v;
        e = good.view();
        expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_SIZE, "air handler 3:", "an outdoor channel out of range");
        good.outdoor_chan[3] = keep;
    }
    const int32_t bad_chan[4] = {-2, kChannels, INT32_MAX, INT32_MIN};
    for (int32_t v : bad_chan) {
        std::vector<int32_t> *arrays[4] = {&good.eff_chan, &good.bypass_chan, &good.heat_chan, &good.cool_chan};
        for (std::vector<int32_t> *arr : arrays) {
            const int32_t keep = (*arr)[8];
            (*arr)[8] = v;
            e = good.view();
            expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_E_SIZE, "air handler 8:", "an optional channel out of range");
            (*arr)[8] = -1;
            e = good.view();
            expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_OK, nullptr, "an optional channel of -1");
            (*arr)[8] = keep;
        }
    }
    e = good.view();
    expect(heat_air_handlers_check(&m.desc, &s, &e), HEAT_OK, nullptr, "the good term again, after every repair");
    if (n_failed) {
        std::printf("%d checks FAILED\n", n_failed);
        return 1;
    }
    std::printf("air handlers host check: all statuses as the header states them\n");
    return 0;
}
