// room_radiation_host_main.cpp — a stand-alone driver of heat_room_radiation_check (include/heat_amd.h) for the sanitizers:
// tests/test_room_radiation_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model, a series with a few long-wave channels, a sky with a few
// long-wave bits and a good room radiation — shuffled entries, a receiver without entries, one with more than a wavefront's
// worth, self-views, channel entries — and damaged ones: numbers out of range, sides above 1, factors that are not finite,
// NULL arrays, lists of no length, duplicate receivers, receivers whose input has a source already. Every call's status is
// checked against the header; the table builder and its verification run inside the check. No device, no HIP.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
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

// The backs of the surfaces s with s % 3 != 0 are the receivers, in a scrambled order; receiver r sees the backs of the
// surfaces of its zone (itself among them), receiver 1 nothing, receiver 2 more than 64 sides from anywhere, every fifth
// one a channel too; the entry list is scrambled.
struct Radiation {
    std::vector<int64_t> rc_surface, en_receiver, en_surface;
    std::vector<uint8_t> rc_side, en_side;
    std::vector<int32_t> en_chan;
    std::vector<double> en_factor, sum;
    Radiation(int64_t S, int64_t Z, int n_channels) {
        for (int64_t q = 0; q < S; q++) {
            const int64_t s = (q * 101) % S;  // (101 and S are coprime: a permutation)
            if (s % 3 != 0) rc_surface.push_back(s), rc_side.push_back(1);
        }
        const int64_t NR = (int64_t)rc_surface.size();
        std::vector<int64_t> er, es;
        std::vector<uint8_t> ed;
        std::vector<int32_t> ec;
        std::vector<double> ef;
        for (int64_t r = 0; r < NR; r++) {
            if (r == 1) continue;
            if (r == 2) {
                for (int64_t j = 0; j < 70; j++) er.push_back(r), es.push_back((j * 37) % S), ed.push_back((uint8_t)(j % 2)), ec.push_back(-1), ef.push_back(1.0 / 70.0);
                continue;
            }
            const int64_t z = rc_surface[r] % Z;
            for (int64_t s = z; s < S; s += Z * 4) er.push_back(r), es.push_back(s), ed.push_back(1), ec.push_back(-1), ef.push_back(0.1 + 0.001 * (double)s);
            er.push_back(r), es.push_back(rc_surface[r]), ed.push_back(1), ec.push_back(-1), ef.push_back(0.2);  // itself
            if (r % 5 == 0) er.push_back(r), es.push_back(-1), ed.push_back(0), ec.push_back((int32_t)(r % n_channels)), ef.push_back(0.05);
        }
        const int64_t NE = (int64_t)er.size();
        int64_t step = 1009;
        while (std::gcd(step, NE) != 1) step++;  // (coprime with NE: a permutation)
        for (int64_t i = 0; i < NE; i++) {
            const int64_t j = (i * step) % NE;
            en_receiver.push_back(er[j]), en_surface.push_back(es[j]), en_side.push_back(ed[j]), en_chan.push_back(ec[j]), en_factor.push_back(ef[j]);
        }
        sum.assign((size_t)NR, 0.0);
    }
    heat_room_radiation view() {
        heat_room_radiation v;
        std::memset(&v, 0, sizeof v);
        v.n_receivers = (int64_t)rc_surface.size();
        v.rc_surface = rc_surface.data(), v.rc_side = rc_side.data(), v.sum_irradiance = sum.data();
        v.n_entries = (int64_t)en_receiver.size();
        v.en_receiver = en_receiver.data(), v.en_surface = en_surface.data(), v.en_side = en_side.data();
        v.en_chan = en_chan.data(), v.en_factor = en_factor.data();
        return v;
    }
};

}  // namespace

int main() {
    const int64_t S = 333, Z = 7;
    const int n_steps = 3, n_sites = 2, NC = 4;
    Model m(S, Z);
    std::vector<heat_weather> weather((size_t)n_steps * n_sites, heat_weather{10.0, 0.0, 1.0});
    std::vector<double> channel((size_t)n_steps * NC, 400.0);
    // the long-wave front of every surface s % 3 == 0 comes from a channel, its back from the sky where s % 6 == 0
    std::vector<int32_t> ir_front(S, -1), ir_back(S, -1);
    std::vector<uint8_t> mode(S, 0);
    for (int64_t q = 0; q < S; q += 3) ir_front[q] = (int32_t)(q % NC);
    for (int64_t q = 0; q < S; q += 6) mode[q] = 8;
    heat_series s;
    std::memset(&s, 0, sizeof s);
    s.n_steps = n_steps, s.n_sub = 1, s.n_channels = NC;
    s.weather = weather.data(), s.channel = channel.data();
    s.ir_front_chan = ir_front.data(), s.ir_back_chan = ir_back.data();
    std::vector<heat_sky_record> record((size_t)n_steps * n_sites, heat_sky_record{0.6, 0.0, 0.8, 700.0, 100.0, 30.0, 350.0, 400.0});
    std::vector<double> normal(S, 0.5);
    heat_sky sky;
    std::memset(&sky, 0, sizeof sky);
    sky.record = record.data(), sky.mode = mode.data();
    sky.normal_x = normal.data(), sky.normal_y = normal.data(), sky.normal_z = normal.data();

    // ---- good radiation ----
    Radiation good(S, Z, NC);
    heat_room_radiation v = good.view();
    const int64_t NR = v.n_receivers, NE = v.n_entries;
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &v), HEAT_OK, nullptr, "good radiation");
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, nullptr, &v), HEAT_OK, nullptr, "good radiation without a sky");
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, nullptr), HEAT_OK, nullptr, "no radiation");
    v.sum_irradiance = nullptr;
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &v), HEAT_OK, nullptr, "no sums");
    v = good.view();
    v.n_entries = 0;
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &v), HEAT_OK, nullptr, "receivers without entries");
    {   // no channel entries: en_chan may be NULL
        Radiation plain(S, Z, NC);
        for (size_t i = 0; i < plain.en_surface.size(); i++)
            if (plain.en_surface[i] < 0) plain.en_surface[i] = 5, plain.en_chan[i] = -1;
        heat_room_radiation p = plain.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &p), HEAT_OK, nullptr, "surfaces only, with en_chan");
        p.en_chan = nullptr;
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &p), HEAT_OK, nullptr, "surfaces only, en_chan NULL");
    }

    // ---- lists of no length ----
    heat_room_radiation e;
    std::memset(&e, 0, sizeof e);
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_OK, nullptr, "empty radiation");
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, nullptr, &e), HEAT_OK, nullptr, "empty radiation without a sky");
    e = good.view();
    e.n_receivers = -1;
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "receiver", "a negative receiver count");
    e = good.view();
    e.n_entries = -5;
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "entry", "a negative entry count");
    e = good.view();
    e.n_receivers = 0;  // the entries still name receivers
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "entry 0:", "entries for receivers there are none of");

    // ---- NULLs ----
    e = good.view();
    e.rc_surface = nullptr;
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "rc_surface", "NULL rc_surface");
    e = good.view();
    e.rc_side = nullptr;
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "rc_side", "NULL rc_side");
    e = good.view();
    e.en_receiver = nullptr;
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "en_receiver", "NULL en_receiver");
    e = good.view();
    e.en_surface = nullptr;
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "en_surface", "NULL en_surface");
    e = good.view();
    e.en_side = nullptr;
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "en_side", "NULL en_side");
    e = good.view();
    e.en_factor = nullptr;
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "en_factor", "NULL en_factor");
    e = good.view();
    e.en_chan = nullptr;  // ... with channel entries in the list
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "en_chan is NULL", "NULL en_chan beside a channel entry");

    // ---- damaged receivers ----
    const int64_t last = NR - 1;
    {
        Radiation bad(S, Z, NC);
        bad.rc_side[7] = 2;
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "receiver 7:", "a receiver side above 1");
    }
    for (int64_t q : {(int64_t)-1, S, S + 100000, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()}) {
        Radiation bad(S, Z, NC);
        bad.rc_surface[last] = q;
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "receiver", "a receiver surface out of range");
    }
    {
        Radiation bad(S, Z, NC);
        bad.rc_surface[last] = bad.rc_surface[3];
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "is receiver 3 already", "the same side twice");
        bad.rc_side[last] = 0;  // the other side of the same surface is another receiver
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_OK, nullptr, "both sides of a surface");
    }
    {
        Radiation bad(S, Z, NC);
        bad.rc_surface[10] = 9, bad.rc_side[10] = 0;  // the front of surface 9 has channel 1
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "receiver 10:", "a receiver with a channel");
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "channel 1", "a receiver with a channel: its number");
        bad.rc_surface[10] = 12, bad.rc_side[10] = 1;  // the back of surface 12 has the sky's bit 3
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "mode bit 3", "a receiver with a sky bit");
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, nullptr, &e), HEAT_OK, nullptr, "... which nothing drives without the sky");
        ir_back[12] = 2;  // both: two sources before the radiation adds a third — the sky's own refusal comes first
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "surface 12:", "a receiver with a channel and a sky bit");
        ir_back[12] = -1;
    }

    // ---- damaged entries ----
    for (double f : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()}) {
        Radiation bad(S, Z, NC);
        bad.en_factor[(size_t)NE - 1] = f;
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "not finite", "a factor that is not finite");
    }
    {
        Radiation bad(S, Z, NC);
        bad.en_factor[5] = -3.5;  // any finite number is the caller's business
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_OK, nullptr, "a negative factor");
    }
    size_t surf_entry = 0, chan_entry = 0;
    while (good.en_surface[surf_entry] < 0) surf_entry++;
    while (good.en_surface[chan_entry] >= 0) chan_entry++;
    {
        Radiation bad(S, Z, NC);
        bad.en_side[surf_entry] = 255;
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "entry", "an emitter side above 1");
        bad.en_side[surf_entry] = 1, bad.en_side[chan_entry] = 77;  // not read beside a channel
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_OK, nullptr, "a side byte beside a channel entry");
    }
    {
        Radiation bad(S, Z, NC);
        bad.en_chan[surf_entry] = 0;
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, "channel 0 beside emitter", "a channel beside a surface");
    }
    for (int64_t q : {(int64_t)-2, S, S + 100000, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()}) {
        Radiation bad(S, Z, NC);
        bad.en_surface[surf_entry] = q;
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "emitter surface", "an emitter out of range");
    }
    for (int64_t r : {(int64_t)-1, NR, NR + 100000, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()}) {
        Radiation bad(S, Z, NC);
        bad.en_receiver[(size_t)NE / 2] = r;
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "receiver", "an entry's receiver out of range");
    }
    for (int32_t c : {-1, -7, NC, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()}) {
        Radiation bad(S, Z, NC);
        bad.en_chan[chan_entry] = c;
        e = bad.view();
        expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_SIZE, "channel", "a channel out of range");
    }
    // the series' own refusals come first
    s.n_sub = -1;
    e = good.view();
    expect(heat_room_radiation_check(&m.desc, n_sites, &s, &sky, &e), HEAT_E_INVALID_ARG, nullptr, "a bad series");
    s.n_sub = 1;

    if (n_failed) {
        std::printf("%d room radiation host checks FAILED\n", n_failed);
        return 1;
    }
    std::printf("room radiation host check: all statuses as the header states them (%lld receivers, %lld entries)\n", (long long)NR, (long long)NE);
    return 0;
}
