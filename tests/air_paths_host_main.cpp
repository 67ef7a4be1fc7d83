// air_paths_host_main.cpp — a stand-alone driver of heat_air_paths_check (include/heat_amd.h) for the sanitizers:
// tests/test_air_paths_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model, a good list of paths — a zone that receives 700 of them, zones
// that receive none, paths of one zone at both ends of the list, zone sources and supply air, controlled and uncontrolled —
// and damaged ones: zones and channels out of range, values that are not finite, NULL arrays, lists of no length. Every
// call's status is checked against the header; the table builder and its verification run inside the check. No device, no HIP.
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

constexpr int32_t kChannels = 6;  // 0, 1 volumes; 2, 3 supply temperatures; 4, 5 setpoints

struct Paths {
    std::vector<int32_t> target, source, temp_chan, volume_chan, open_chan;
    std::vector<double> volume_gain, band, min_delta, sum_q;
    std::vector<int8_t> sense;
    std::vector<uint8_t> state;
    std::vector<int64_t> steps_open, switches;
    // source -1: supply air; controlled: every third path
    void add(int32_t t, int32_t s) {
        const size_t i = target.size();
        target.push_back(t), source.push_back(s);
        temp_chan.push_back(s < 0 ? 2 + (int32_t)(i % 2) : -1);
        volume_chan.push_back((int32_t)(i % 2));
        volume_gain.push_back(0.5 + 0.001 * (double)(i % 1000));
        open_chan.push_back(i % 3 == 0 ? 4 + (int32_t)(i % 2) : -1);
        sense.push_back(i % 2 ? (int8_t)1 : (int8_t)-1);
        band.push_back(0.1 * (double)(i % 5)), min_delta.push_back(0.05 * (double)(i % 3));
        state.push_back((uint8_t)(i % 2)), sum_q.push_back(0.0), steps_open.push_back(0), switches.push_back(0);
    }
    heat_air_paths view() {
        heat_air_paths a;
        std::memset(&a, 0, sizeof a);
        a.n_paths = (int64_t)target.size();
        a.target = target.data(), a.source = source.data(), a.temp_chan = temp_chan.data(), a.volume_chan = volume_chan.data();
        a.volume_gain = volume_gain.data(), a.open_chan = open_chan.data(), a.sense = sense.data(), a.band = band.data();
        a.min_delta = min_delta.data(), a.state = state.data(), a.sum_q = sum_q.data(), a.steps_open = steps_open.data();
        a.switches = switches.data();
        return a;
    }
};

}  // namespace

int main() {
    const int64_t S = 90, Z = 37;
    const int n_steps = 3, n_sites = 2;
    Model m(S, Z);
    std::vector<heat_weather> weather((size_t)n_steps * n_sites, heat_weather{10.0, 0.0, 1.0});
    std::vector<double> channel((size_t)n_steps * kChannels, 20.0);
    heat_series s;
    std::memset(&s, 0, sizeof s);
    s.n_steps = n_steps, s.n_sub = 1, s.n_channels = kChannels;
    s.weather = weather.data(), s.channel = channel.data();

    // ---- a good list ----
    Paths good;
    good.add(36, 0);                                                     // the last zone: its paths stand at both ends of the list
    good.add(36, -1);
    for (int32_t z = 0; z < Z; z++) {                                    // zones 5, 12, 19, ... receive none
        if (z % 7 == 5 || z == 36) continue;
        good.add(z, (z + 1) % (int32_t)Z);
        good.add(z, -1);
        if (z % 2) good.add(z, (z + 11) % (int32_t)Z);
    }
    for (int i = 0; i < 700; i++) good.add(17, i % 4 == 0 ? -1 : (int32_t)((18 + i) % 37 == 17 ? 3 : (18 + i) % 37));  // a zone with 700
    good.add(0, 36);                                                     // far from zone 0's other paths
    good.add(36, 1);
    heat_air_paths a = good.view();
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &a), HEAT_OK, nullptr, "a good list");
    expect(heat_air_paths_check(&m.desc, n_sites, &s, nullptr), HEAT_OK, nullptr, "no paths");
    a.state = nullptr, a.sum_q = nullptr, a.steps_open = nullptr, a.switches = nullptr, a.volume_gain = nullptr;
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &a), HEAT_OK, nullptr, "no state, accumulators or gains");

    // ---- lists of no length ----
    heat_air_paths e;
    std::memset(&e, 0, sizeof e);
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_OK, nullptr, "an empty list");
    e = good.view();
    e.n_paths = 0;
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_OK, nullptr, "arrays of no length");
    e.n_paths = -1;
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "air path", "a negative count");
    e = good.view();
    e.n_paths = 1;
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_OK, nullptr, "a list of one path");

    // ---- all uncontrolled, all from zones: the optional arrays are not read ----
    {
        Paths plain;
        for (int32_t z = 0; z < Z; z++) plain.add(z, (z + 3) % (int32_t)Z);
        e = plain.view();
        e.open_chan = nullptr, e.sense = nullptr, e.band = nullptr, e.min_delta = nullptr, e.temp_chan = nullptr;
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_OK, nullptr, "uncontrolled zone-to-zone paths without the optional arrays");
        std::vector<int32_t> none((size_t)Z, -1);
        e.open_chan = none.data();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_OK, nullptr, "open channels of -1 without a controller's arrays");
    }

    // ---- NULLs ----
    e = good.view();
    e.target = nullptr;
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "target", "NULL target");
    e = good.view();
    e.source = nullptr;
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "source", "NULL source");
    e = good.view();
    e.volume_chan = nullptr;
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "volume_chan", "NULL volume_chan");
    e = good.view();
    e.sense = nullptr;
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "air path 0:", "NULL sense with a controlled path");
    e = good.view();
    e.band = nullptr;
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "band", "NULL band with a controlled path");
    e = good.view();
    e.min_delta = nullptr;
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "min_delta", "NULL min_delta with a controlled path");
    e = good.view();
    e.temp_chan = nullptr;
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_SIZE, "air path 1:", "supply air without temp_chan");

    // ---- values that are not finite or negative, a bad sense, a bad state ----
    const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                           -std::numeric_limits<double>::infinity()};
    const size_t at = 300;  // (300 % 3 == 0: controlled)
    for (double v : bad) {
        std::vector<double> *arrays[3] = {&good.volume_gain, &good.band, &good.min_delta};
        for (std::vector<double> *arr : arrays) {
            const double keep = (*arr)[at];
            (*arr)[at] = v;
            e = good.view();
            expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "air path 300:", "a value that is not finite");
            (*arr)[at] = keep;
        }
    }
    {
        std::vector<double> *arrays[2] = {&good.band, &good.min_delta};
        for (std::vector<double> *arr : arrays) {
            const double keep = (*arr)[at];
            (*arr)[at] = -0.25;
            e = good.view();
            expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "air path 300:", "a negative band or min_delta");
            (*arr)[at + 1] = -0.25;  // (301 is uncontrolled: not read)
            (*arr)[at] = keep;
            e = good.view();
            expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_OK, nullptr, "a negative band on an uncontrolled path");
            (*arr)[at + 1] = 0.0;
        }
        const int8_t bad_sense[4] = {0, 2, -2, 127};
        for (int8_t v : bad_sense) {
            const int8_t keep = good.sense[at];
            good.sense[at] = v;
            e = good.view();
            expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "air path 300:", "a sense other than +1 / -1");
            good.sense[at] = keep;
        }
        good.sense[at + 1] = 0;  // (uncontrolled: not read)
        e = good.view();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_OK, nullptr, "any sense on an uncontrolled path");
        good.sense[at + 1] = 1;
        const uint8_t bad_state[2] = {2, 255};
        for (uint8_t v : bad_state) {
            const uint8_t keep = good.state[77];
            good.state[77] = v;
            e = good.view();
            expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "air path 77:", "a state byte above 1");
            good.state[77] = keep;
        }
    }

    // ---- zones and channels out of range, a path onto itself, two sources ----
    const int32_t bad_zone[4] = {-2, (int32_t)Z, INT32_MAX, INT32_MIN};
    for (int32_t z : bad_zone) {
        const int32_t keep_t = good.target[40], keep_s = good.source[41], keep_c = good.temp_chan[41];
        good.target[40] = z;
        e = good.view();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_SIZE, "air path 40:", "a target out of range");
        good.target[40] = keep_t;
        good.source[41] = z, good.temp_chan[41] = -1;
        e = good.view();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_SIZE, "air path 41:", "a source out of range");
        good.source[41] = keep_s, good.temp_chan[41] = keep_c;
    }
    {
        const int32_t keep = good.target[40];
        good.target[40] = -1;
        e = good.view();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_SIZE, "air path 40:", "a target of -1");
        good.target[40] = keep;
    }
    const int32_t bad_chan[4] = {-2, kChannels, INT32_MAX, INT32_MIN};
    for (int32_t c : bad_chan) {
        int32_t keep = good.volume_chan[9];
        good.volume_chan[9] = c;
        e = good.view();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_SIZE, "air path 9:", "a volume channel out of range");
        good.volume_chan[9] = keep;
        keep = good.open_chan[9];
        good.open_chan[9] = c;
        e = good.view();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_SIZE, "air path 9:", "an open channel out of range");
        good.open_chan[9] = keep;
        keep = good.temp_chan[1];  // (path 1 is supply air)
        good.temp_chan[1] = c;
        e = good.view();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_SIZE, "air path 1:", "a temperature channel out of range");
        good.temp_chan[1] = keep;
    }
    {
        int32_t keep = good.volume_chan[9];
        good.volume_chan[9] = -1;
        e = good.view();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_SIZE, "air path 9:", "a volume channel of -1");
        good.volume_chan[9] = keep;
        keep = good.temp_chan[1];
        good.temp_chan[1] = -1;
        e = good.view();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_SIZE, "air path 1:", "supply air with temperature channel -1");
        good.temp_chan[1] = keep;
        keep = good.temp_chan[0];  // (path 0 comes from zone 0)
        good.temp_chan[0] = 2;
        e = good.view();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_SIZE, "one source", "a zone source with a temperature channel");
        good.temp_chan[0] = keep;
        keep = good.source[0];
        good.source[0] = good.target[0];
        e = good.view();
        expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "air path 0:", "a path from a zone into itself");
        good.source[0] = keep;
    }
    e = good.view();
    expect(heat_air_paths_check(&m.desc, n_sites, &s, &e), HEAT_OK, nullptr, "the good list again, after every repair");
    if (n_failed) {
        std::printf("%d checks FAILED\n", n_failed);
        return 1;
    }
    std::printf("air paths host check: all statuses as the header states them\n");
    return 0;
}
