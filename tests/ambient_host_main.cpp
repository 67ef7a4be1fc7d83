// ambient_host_main.cpp — a stand-alone driver of heat_ambient_check (include/heat_amd.h) and of the ambient table builder
// (heat_amd/csrc/plan.hpp) for the sanitizers: tests/test_ambient_series_host.py compiles it together with
// heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model whose fronts are Ambient on every fourth surface and whose backs
// are Ambient on every third (so every twelfth wall is Ambient on both sides), a series with a few channels and a good
// drive — the sides in a scrambled order, gain, offset and mix on some — and damaged ones: numbers out of range, sides above
// 1, sides that are not Ambient, values that are not finite, NULL arrays, lists of no length, a side listed twice. Every
// call's status is checked against the header. The tables are also built against a device order of their own (dev_of) and
// compared element by element: the record, the peer back record of a both-sides-Ambient wall, the sentinel elsewhere; then
// damaged and refused by their verification. No device, no HIP.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

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

void expect_true(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED %s\n", what);
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
        const int64_t n_nodes = 3;
        node_offset.resize(S + 1);
        for (int64_t s = 0; s <= S; s++) node_offset[s] = n_nodes * s;
        mass.assign(n_nodes * S, 4000.0);
        uvalue.assign(n_nodes * S, 1.5);
        alpha.assign(n_nodes * S, 0.0);
        zeros.assign(S, 0.0);
        ones.assign(S, 1.0);
        kind_front.resize(S), kind_back.resize(S), zone_front.assign(S, 0), zone_back.resize(S);
        for (int64_t s = 0; s < S; s++) {
            kind_front[s] = s % 4 == 0 ? HEAT_BOUNDARY_AMBIENT : HEAT_BOUNDARY_OUTDOOR;
            kind_back[s] = s % 3 == 0 ? HEAT_BOUNDARY_AMBIENT : HEAT_BOUNDARY_SPACE;
            zone_back[s] = (int32_t)(s % Z);
        }
        zone_slot.resize(Z);
        for (int64_t z = 0; z < Z; z++) zone_slot[z] = z;
        for (int a = 0; a < 9; a++) {
            slot[a].resize(S);
            for (int64_t s = 0; s < S; s++) slot[a][s] = Z + s * (8 + n_nodes) + (a < 8 ? a : 8);
        }
        zone_volume.assign(Z, 250.0);
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

// Every Ambient side of the model, scrambled; gain on every second, offset on every third, a mix zone on every fourth.
struct Drive {
    std::vector<int64_t> surface;
    std::vector<uint8_t> side;
    std::vector<int32_t> chan, mix_zone;
    std::vector<double> gain, offset, mix, sum;
    Drive(const Model &m, int n_channels) {
        std::vector<int64_t> qs;
        std::vector<uint8_t> ds;
        for (int64_t s = 0; s < m.S; s++) {
            if (m.kind_front[s] == HEAT_BOUNDARY_AMBIENT) qs.push_back(s), ds.push_back(0);
            if (m.kind_back[s] == HEAT_BOUNDARY_AMBIENT) qs.push_back(s), ds.push_back(1);
        }
        const int64_t N = (int64_t)qs.size();
        int64_t step = 89;
        while (N % step == 0) step++;  // (89 is prime: coprime with N unless it divides it)
        for (int64_t i = 0; i < N; i++) {
            const int64_t j = (i * step) % N;
            surface.push_back(qs[j]), side.push_back(ds[j]);
            chan.push_back((int32_t)(i % n_channels));
            gain.push_back(i % 2 ? 1.0 : 0.9), offset.push_back(i % 3 ? 0.0 : -2.5);
            mix_zone.push_back(i % 4 ? -1 : (int32_t)(i % m.Z));
            mix.push_back(i % 4 ? std::numeric_limits<double>::quiet_NaN() : 0.5);  // (read only where there is a zone)
        }
        sum.assign((size_t)N, 0.0);
    }
    heat_ambient_drive view() {
        heat_ambient_drive v;
        std::memset(&v, 0, sizeof v);
        v.n_sides = (int64_t)surface.size();
        v.surface = surface.data(), v.side = side.data(), v.chan = chan.data();
        v.gain = gain.data(), v.offset = offset.data(), v.mix_zone = mix_zone.data(), v.mix = mix.data();
        v.sum_temperature = sum.data();
        return v;
    }
};

}  // namespace

int main() {
    const int64_t S = 301, Z = 7;
    const int n_steps = 3, n_sites = 2, NC = 5;
    Model m(S, Z);
    std::vector<heat_weather> weather((size_t)n_steps * n_sites, heat_weather{10.0, 0.0, 1.0});
    std::vector<double> channel((size_t)n_steps * NC, 12.0);
    heat_series s;
    std::memset(&s, 0, sizeof s);
    s.n_steps = n_steps, s.n_sub = 1, s.n_channels = NC;
    s.weather = weather.data(), s.channel = channel.data();

    // ---- good drives ----
    Drive good(m, NC);
    heat_ambient_drive v = good.view();
    const int64_t N = v.n_sides;
    expect(heat_ambient_check(&m.desc, n_sites, &s, &v), HEAT_OK, nullptr, "good drive");
    expect(heat_ambient_check(&m.desc, n_sites, &s, nullptr), HEAT_OK, nullptr, "no drive");
    v.n_sides = 0;
    expect(heat_ambient_check(&m.desc, n_sites, &s, &v), HEAT_OK, nullptr, "a drive of no side");
    v.surface = nullptr, v.side = nullptr, v.chan = nullptr;
    expect(heat_ambient_check(&m.desc, n_sites, &s, &v), HEAT_OK, nullptr, "a drive of no side and no array");
    v = good.view();
    v.gain = nullptr, v.offset = nullptr, v.sum_temperature = nullptr;
    expect(heat_ambient_check(&m.desc, n_sites, &s, &v), HEAT_OK, nullptr, "no gain, offset, sums");
    v.mix_zone = nullptr, v.mix = nullptr;
    expect(heat_ambient_check(&m.desc, n_sites, &s, &v), HEAT_OK, nullptr, "no mixing at all");
    {
        Drive plain(m, NC);
        for (auto &z : plain.mix_zone) z = -1;
        heat_ambient_drive p = plain.view();
        p.mix = nullptr;
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_OK, nullptr, "mix NULL where no side mixes");
    }

    // ---- damaged drives ----
    heat_ambient_drive e = good.view();
    e.n_sides = -2;
    expect(heat_ambient_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "ambient side", "negative count");
    const char *const name[3] = {"surface", "side", "chan"};
    for (int a = 0; a < 3; a++) {
        e = good.view();
        if (a == 0) e.surface = nullptr;
        if (a == 1) e.side = nullptr;
        if (a == 2) e.chan = nullptr;
        expect(heat_ambient_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, name[a], "a NULL array");
    }
    e = good.view();
    e.mix = nullptr;
    expect(heat_ambient_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, "ambient side 0:", "mix NULL beside a mixing side");
    {
        Drive d(m, NC);
        d.side[5] = 2;
        heat_ambient_drive p = d.view();
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_INVALID_ARG, "ambient side 5:", "a side byte above 1");
    }
    {
        Drive d(m, NC);
        d.gain[6] = std::numeric_limits<double>::infinity();
        heat_ambient_drive p = d.view();
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_INVALID_ARG, "ambient side 6:", "an infinite gain");
        d.gain[6] = 1.0, d.offset[7] = std::numeric_limits<double>::quiet_NaN();
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_INVALID_ARG, "ambient side 7:", "a NaN offset");
        d.offset[7] = 0.0, d.mix[8] = std::numeric_limits<double>::quiet_NaN();
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_INVALID_ARG, "ambient side 8:", "a NaN mix on a mixing side");
    }
    {
        Drive d(m, NC);
        d.surface[9] = S;
        heat_ambient_drive p = d.view();
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_SIZE, "ambient side 9:", "a surface past the end");
        d.surface[9] = -1;
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_SIZE, "ambient side 9:", "a negative surface");
    }
    {
        Drive d(m, NC);
        d.surface[10] = 1, d.side[10] = 0;  // the front of surface 1 faces the outdoor air
        heat_ambient_drive p = d.view();
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_SIZE, "ambient side 10:", "an Outdoor side");
        d.side[10] = 1;                     // ... and its back a zone, whose record keeps a list position in that slot
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_SIZE, "ambient side 10:", "a Space side");
    }
    {
        Drive d(m, NC);
        d.surface[11] = d.surface[3], d.side[11] = d.side[3];
        heat_ambient_drive p = d.view();
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_SIZE, "ambient side 11:", "a side listed twice");
    }
    {
        Drive d(m, NC);
        d.chan[12] = NC;
        heat_ambient_drive p = d.view();
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_SIZE, "ambient side 12:", "a channel past the end");
        d.chan[12] = -1;
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_SIZE, "ambient side 12:", "a negative channel");
        d.chan[12] = 0, d.mix_zone[13] = (int32_t)Z;
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_SIZE, "ambient side 13:", "a mix zone past the end");
        d.mix_zone[13] = -2;
        expect(heat_ambient_check(&m.desc, n_sites, &s, &p), HEAT_E_SIZE, "ambient side 13:", "a mix zone below -1");
    }
    s.n_sub = -1;
    e = good.view();
    expect(heat_ambient_check(&m.desc, n_sites, &s, &e), HEAT_E_INVALID_ARG, nullptr, "a bad series");
    s.n_sub = 1;

    // ---- the setter's checks (the same list check under its own name) ----
    const int32_t *const kind[2] = {m.kind_front.data(), m.kind_back.data()};
    std::string err;
    expect_true(heat::check_ambient_sides(S, kind, N, good.surface.data(), good.side.data(), "entry", err) == HEAT_OK, "the setter's good list");
    expect_true(heat::check_ambient_sides(S, kind, 0, nullptr, nullptr, "entry", err) == HEAT_OK, "the setter's empty list");
    expect_true(heat::check_ambient_sides(S, kind, -1, nullptr, nullptr, "entry", err) == HEAT_E_INVALID_ARG, "the setter's negative count");
    expect_true(heat::check_ambient_sides(S, kind, 2, nullptr, good.side.data(), "entry", err) == HEAT_E_INVALID_ARG && err.find("entry 0") != std::string::npos,
                "the setter's NULL surfaces");
    {
        const int64_t q[3] = {0, 12, 1};
        const uint8_t d[3] = {0, 1, 1};
        expect_true(heat::check_ambient_sides(S, kind, 3, q, d, "entry", err) == HEAT_E_SIZE && err.find("entry 2:") != std::string::npos, "the setter's Space side");
        const int64_t q2[3] = {0, 12, 0};
        const uint8_t d2[3] = {0, 1, 0};
        expect_true(heat::check_ambient_sides(S, kind, 3, q2, d2, "entry", err) == HEAT_E_SIZE && err.find("entry 2:") != std::string::npos, "the setter's duplicate");
    }

    // ---- the tables against a device order of their own ----
    std::vector<int32_t> dev_of((size_t)S);
    for (int64_t q = 0; q < S; q++) dev_of[(size_t)q] = (int32_t)((q * 37 + 11) % S);  // (37 and 301 are coprime: a permutation)
    heat::AmbientTables t;
    heat::build_ambient_tables(S, dev_of.data(), kind, N, good.surface.data(), good.side.data(), t);
    expect_true(t.rec.size() == (size_t)N && t.peer.size() == (size_t)N, "table sizes");
    int64_t n_peers = 0;
    for (int64_t i = 0; i < N && t.rec.size() == (size_t)N; i++) {
        const int64_t q = good.surface[(size_t)i];
        const bool both = good.side[(size_t)i] == 0 && q % 3 == 0;  // (a driven front: q % 4 == 0; its back is Ambient when q % 3 == 0)
        expect_true(t.rec[(size_t)i] == (uint32_t)(good.side[(size_t)i] * S + dev_of[(size_t)q]), "a record");
        expect_true(t.peer[(size_t)i] == (both ? (uint32_t)(S + dev_of[(size_t)q]) : heat::kNoAmbientPeer), "a peer");
        n_peers += both;
    }
    expect_true(n_peers == (S + 11) / 12, "every twelfth wall has a peer");
    expect_true(heat::check_ambient_tables(S, dev_of.data(), kind, N, good.surface.data(), good.side.data(), t, err) == HEAT_OK, "the tables verify");
    {
        heat::AmbientTables bad = t;
        bad.rec[4] = (uint32_t)(2 * S);
        expect_true(heat::check_ambient_tables(S, dev_of.data(), kind, N, good.surface.data(), good.side.data(), bad, err) == HEAT_E_SIZE, "a record past the end");
        bad = t;
        bad.rec[4] = bad.rec[5];
        expect_true(heat::check_ambient_tables(S, dev_of.data(), kind, N, good.surface.data(), good.side.data(), bad, err) == HEAT_E_SIZE, "a record of another side");
        bad = t;
        for (int64_t i = 0; i < N; i++)
            if (bad.peer[(size_t)i] != heat::kNoAmbientPeer) { bad.peer[(size_t)i] = heat::kNoAmbientPeer; break; }
        expect_true(heat::check_ambient_tables(S, dev_of.data(), kind, N, good.surface.data(), good.side.data(), bad, err) == HEAT_E_SIZE, "a missing peer");
        bad = t;
        for (int64_t i = 0; i < N; i++)
            if (bad.peer[(size_t)i] == heat::kNoAmbientPeer) { bad.peer[(size_t)i] = (uint32_t)S; break; }
        expect_true(heat::check_ambient_tables(S, dev_of.data(), kind, N, good.surface.data(), good.side.data(), bad, err) == HEAT_E_SIZE, "a stray peer");
        bad = t;
        bad.peer.pop_back();
        expect_true(heat::check_ambient_tables(S, dev_of.data(), kind, N, good.surface.data(), good.side.data(), bad, err) == HEAT_E_SIZE, "a short table");
        heat::AmbientTables none;
        heat::build_ambient_tables(S, dev_of.data(), kind, 0, nullptr, nullptr, none);
        expect_true(none.rec.empty() && heat::check_ambient_tables(S, dev_of.data(), kind, 0, nullptr, nullptr, none, err) == HEAT_OK, "no tables without sides");
    }

    if (n_failed) {
        std::printf("%d ambient host checks FAILED\n", n_failed);
        return 1;
    }
    std::printf("ambient host check: all statuses as the header states them (%lld sides, %lld peers)\n", (long long)N, (long long)n_peers);
    return 0;
}
