// air_networks_host_main.cpp — a stand-alone driver of heat_air_networks_check (include/heat_amd.h) for the sanitizers:
// tests/test_air_networks_host.py compiles it together with heat_amd/csrc/plan.cpp by
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// and runs it as a child process. It lays out a small model, a good term — 61 networks of 1 to 64 nodes over 400 zones, every
// width class present, chains of doorways with links to outside, sources, wind pressures and open fractions, every derived
// channel written once — and damaged ones: offsets that do not partition the nodes, zones in two networks or in none, links
// across networks, sides with two temperatures or none, constants that are negative or not finite, NULL arrays, lists of no
// length, derived channels written twice or read by a network. Every call's status is checked against the header; the table
// builder (the class sort, the per-node link lists, s_lin) and its verification run inside the check. No device, no HIP.
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

constexpr int32_t kInputs = 7;  // 0, 1 outside temperatures; 2, 3 wind pressures; 4 an open fraction; 5 a fan; 6 unread; the derived channels follow

struct Networks {
    std::vector<int32_t> net_offset, max_iter, node_zone, src_chan, zone_a, zone_b, temp_chan, wp_chan, frac_chan, out_ab, out_ba;
    std::vector<double> tol, g_min, src_gain, c, gh, p_lin, wp_gain, pressure, sum_ab, sum_ba, max_res;
    std::vector<int64_t> iters_sum, unconverged;
    // networks of 1, 2, ..., 8, 9, 16, 17, 32, 33, 64 nodes, then fives, over the zones in a scattered order
    explicit Networks(int64_t Z) {
        const int sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 32, 33, 64};
        int64_t at = 0;
        net_offset.push_back(0);
        auto zone_of = [Z](int64_t i) { return (int32_t)((i * 7) % Z); };  // (7 and Z = 400 share no factor)
        size_t k = 0;
        while (at < Z) {
            int64_t n = k < sizeof sizes / sizeof sizes[0] ? sizes[k] : 5;
            if (at + n > Z) n = Z - at;
            k++;
            for (int64_t i = 0; i < n; i++) {
                node_zone.push_back(zone_of(at + i));
                src_chan.push_back((at + i) % 6 == 0 ? 5 : -1), src_gain.push_back(0.5), pressure.push_back(0.25 * (double)i);
                if (i > 0) link(zone_of(at + i), zone_of(at + i / 2), 0.5);          // a tree of doorways
                if (i > 0 && i % 4 == 0) link(zone_of(at + i), zone_of(at + i - 1), 0.4);  // a second link of the same two zones, or a loop
                if (i % 3 == 0) link(zone_of(at + i), -1, 0.02);
            }
            at += n;
            net_offset.push_back((int32_t)at), tol.push_back(1e-7), max_iter.push_back(24), g_min.push_back(1e-9);
            iters_sum.push_back(0), unconverged.push_back(0), max_res.push_back(0.0);
        }
        int32_t next = kInputs;
        for (size_t l = 0; l < zone_a.size(); l++) {
            out_ab[l] = zone_b[l] >= 0 ? next++ : -1;
            out_ba[l] = l % 5 == 4 ? -1 : next++;
        }
    }
    void link(int32_t a, int32_t b, double coef) {
        const size_t l = zone_a.size();
        zone_a.push_back(a), zone_b.push_back(b), temp_chan.push_back(b < 0 ? (int32_t)(l % 2) : -1);
        wp_chan.push_back(b < 0 && l % 3 ? 2 + (int32_t)(l % 2) : -1), frac_chan.push_back(l % 4 == 1 ? 4 : -1);
        out_ab.push_back(-1), out_ba.push_back(-1);
        c.push_back(coef), gh.push_back(9.81 * (double)(l % 7)), p_lin.push_back(0.05 + 0.01 * (double)(l % 3)), wp_gain.push_back(0.8);
        sum_ab.push_back(0.0), sum_ba.push_back(0.0);
    }
    int32_t n_derived() const { return 2 * (int32_t)zone_a.size(); }
    heat_air_networks view() {
        heat_air_networks nw;
        std::memset(&nw, 0, sizeof nw);
        nw.n_networks = (int64_t)tol.size(), nw.n_nodes = (int64_t)node_zone.size(), nw.n_links = (int64_t)zone_a.size();
        nw.net_offset = net_offset.data(), nw.tol = tol.data(), nw.max_iter = max_iter.data(), nw.g_min = g_min.data();
        nw.node_zone = node_zone.data(), nw.src_chan = src_chan.data(), nw.src_gain = src_gain.data();
        nw.zone_a = zone_a.data(), nw.zone_b = zone_b.data(), nw.temp_chan = temp_chan.data(), nw.wp_chan = wp_chan.data();
        nw.frac_chan = frac_chan.data(), nw.out_ab = out_ab.data(), nw.out_ba = out_ba.data();
        nw.c = c.data(), nw.gh = gh.data(), nw.p_lin = p_lin.data(), nw.wp_gain = wp_gain.data();
        nw.resume = 1, nw.pressure = pressure.data(), nw.sum_ab = sum_ab.data(), nw.sum_ba = sum_ba.data();
        nw.iters_sum = iters_sum.data(), nw.unconverged = unconverged.data(), nw.max_res = max_res.data();
        return nw;
    }
};

}  // namespace

#define CHECK(nwp) heat_air_networks_check(&m.desc, &s, nullptr, nullptr, nwp)

int main() {
    const int64_t S = 90, Z = 400;
    Model m(S, Z);
    Networks good(Z);
    const int32_t n_channels = kInputs + good.n_derived();
    const int n_steps = 3;
    std::vector<heat_weather> weather((size_t)n_steps, heat_weather{10.0, 0.0, 1.0});
    std::vector<double> channel((size_t)n_steps * n_channels, 20.0);
    heat_series s;
    std::memset(&s, 0, sizeof s);
    s.n_steps = n_steps, s.n_sub = 1, s.n_channels = n_channels;
    s.weather = weather.data(), s.channel = channel.data();
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // ---- a good term ----
    heat_air_networks nw = good.view(), e;
    expect(CHECK(&nw), HEAT_OK, nullptr, "a good term");
    expect(CHECK(nullptr), HEAT_OK, nullptr, "no term");
    nw.src_chan = nullptr, nw.src_gain = nullptr, nw.wp_chan = nullptr, nw.frac_chan = nullptr, nw.out_ab = nullptr, nw.out_ba = nullptr;
    nw.gh = nullptr, nw.wp_gain = nullptr, nw.pressure = nullptr, nw.sum_ab = nullptr, nw.sum_ba = nullptr, nw.iters_sum = nullptr;
    nw.unconverged = nullptr, nw.max_res = nullptr;
    expect(CHECK(&nw), HEAT_OK, nullptr, "no optional list, state or accumulator");

    // ---- lists of no length ----
    std::memset(&e, 0, sizeof e);
    expect(CHECK(&e), HEAT_OK, nullptr, "an empty term");
    e = good.view(), e.n_networks = 0, e.n_nodes = 0, e.n_links = 0;
    expect(CHECK(&e), HEAT_OK, nullptr, "arrays of no length");
    e = good.view(), e.n_networks = -1;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "negative count", "a negative count of networks");
    e = good.view(), e.n_links = -1;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "negative count", "a negative count of links");
    e = good.view(), e.n_networks = 0;
    expect(CHECK(&e), HEAT_E_SIZE, "network 0:", "nodes without a network");

    // ---- NULLs ----
    e = good.view(), e.net_offset = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "network 0: net_offset", "NULL net_offset");
    e = good.view(), e.tol = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "network 0: tol", "NULL tol");
    e = good.view(), e.max_iter = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "network 0: max_iter", "NULL max_iter");
    e = good.view(), e.g_min = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "network 0: g_min", "NULL g_min");
    e = good.view(), e.node_zone = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "node 0: node_zone", "NULL node_zone");
    e = good.view(), e.zone_a = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "link 0: zone_a", "NULL zone_a");
    e = good.view(), e.zone_b = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "link 0: zone_b", "NULL zone_b");
    e = good.view(), e.temp_chan = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "link 0: temp_chan", "NULL temp_chan");
    e = good.view(), e.c = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "link 0: c", "NULL c");
    e = good.view(), e.p_lin = nullptr;
    expect(CHECK(&e), HEAT_E_INVALID_ARG, "link 0: p_lin", "NULL p_lin");
    expect(heat_air_networks_check(&m.desc, nullptr, nullptr, nullptr, &nw), HEAT_E_INVALID_ARG, "series", "NULL series");

    // ---- the networks' extents, the zones, the links, values, derived channels ----
    {
        Networks bad = good;
        bad.net_offset[0] = 1, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "network 0:", "offsets that do not start at 0");
        bad = good, bad.net_offset[3] = bad.net_offset[2], e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "network 2:", "a network of no node");
        bad = good, bad.net_offset[14] = bad.net_offset[13] + 65, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "network 13:", "a network of 65 nodes");
        bad = good, bad.net_offset.back() -= 1, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "network", "offsets that do not end at the nodes");
        bad = good, bad.node_zone[7] = (int32_t)Z, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "node 7:", "a zone past the end");
        bad = good, bad.node_zone[7] = -1, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "node 7:", "a negative zone");
        bad = good, bad.node_zone[300] = bad.node_zone[2], e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "node 300:", "a zone in two networks");
        bad = good, bad.src_chan[6] = n_channels, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "node 6:", "a source channel past the end");
        bad = good, bad.src_chan[6] = -2, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "node 6:", "a source channel below -1");
        bad = good, bad.src_gain[6] = nan, e = bad.view();
        expect(CHECK(&e), HEAT_E_INVALID_ARG, "node 6:", "a source gain that is not finite");
        bad = good, bad.pressure[9] = inf, e = bad.view();
        expect(CHECK(&e), HEAT_E_INVALID_ARG, "node 9:", "a pressure that is not finite on resume");
        bad = good, bad.pressure[9] = inf, e = bad.view(), e.resume = 0;
        expect(CHECK(&e), HEAT_OK, nullptr, "a pressure that is not read without resume");
        for (const int32_t v : {0, 65, -3}) {
            bad = good, bad.max_iter[4] = v, e = bad.view();
            expect(CHECK(&e), HEAT_E_INVALID_ARG, "network 4:", "max_iter outside [1, 64]");
        }
        for (const double v : {nan, inf, -inf, -1e-300}) {
            bad = good, bad.tol[5] = v, e = bad.view();
            expect(CHECK(&e), HEAT_E_INVALID_ARG, "network 5:", "a tol that is negative or not finite");
            bad = good, bad.g_min[5] = v, e = bad.view();
            expect(CHECK(&e), HEAT_E_INVALID_ARG, "network 5:", "a g_min that is not positive and finite");
            bad = good, bad.c[50] = v, e = bad.view();
            expect(CHECK(&e), HEAT_E_INVALID_ARG, "link 50:", "a c that is negative or not finite");
            bad = good, bad.gh[50] = v, e = bad.view();
            expect(CHECK(&e), HEAT_E_INVALID_ARG, "link 50:", "a gh that is negative or not finite");
            bad = good, bad.p_lin[50] = v, e = bad.view();
            expect(CHECK(&e), HEAT_E_INVALID_ARG, "link 50:", "a p_lin that is not positive and finite");
        }
        bad = good, bad.g_min[5] = 0.0, e = bad.view();
        expect(CHECK(&e), HEAT_E_INVALID_ARG, "network 5:", "a g_min of zero");
        bad = good, bad.p_lin[50] = 0.0, e = bad.view();
        expect(CHECK(&e), HEAT_E_INVALID_ARG, "link 50:", "a p_lin of zero");
        bad = good, bad.tol[5] = 0.0, bad.c[50] = 0.0, bad.gh[50] = 0.0, e = bad.view();
        expect(CHECK(&e), HEAT_OK, nullptr, "a tol, a c and a gh of zero");
        bad = good, bad.wp_gain[50] = nan, e = bad.view();
        expect(CHECK(&e), HEAT_E_INVALID_ARG, "link 50:", "a wind pressure gain that is not finite");
        // the links' zones: links 0 and 1 are the links to outside of networks 0 and 1, link 2 joins the nodes of network 1
        bad = good, bad.zone_a[1] = (int32_t)Z, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 1:", "zone_a past the end");
        bad = good, bad.zone_b[1] = -2, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 1:", "zone_b below -1");
        bad = good, bad.zone_b[1] = bad.zone_a[1], e = bad.view();
        expect(CHECK(&e), HEAT_E_INVALID_ARG, "link 1:", "zone_a equal to zone_b");
        bad = good, bad.zone_b[1] = bad.node_zone[0], e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 1:", "a link into another network");
        bad = good, bad.temp_chan[0] = -1, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 0:", "outside air without a temperature channel");
        bad = good, bad.temp_chan[2] = 0, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 2:", "a temperature channel on a link between zones");
        bad = good, bad.wp_chan[2] = 2, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 2:", "a wind pressure on a link between zones");
        bad = good, bad.temp_chan[0] = n_channels, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 0:", "a temperature channel past the end");
        bad = good, bad.frac_chan[0] = -2, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 0:", "an open-fraction channel below -1");
        bad = good, bad.out_ba[0] = n_channels, e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 0:", "a derived channel past the end");
        // network 0 is one node with one link to outside
        bad = good, bad.zone_a[0] = bad.node_zone[1], e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "network 0:", "a network with no link to outside");
        bad = good, bad.out_ba[60] = bad.out_ab[2], e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 60:", "two links with one derived channel");
        bad = good, bad.out_ab[1] = bad.out_ba[1], e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 1:", "a link whose two flows share one derived channel");
        bad = good, bad.frac_chan[2] = bad.out_ba[70], e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 2:", "an open-fraction channel that is a derived channel");
        bad = good, bad.temp_chan[0] = bad.out_ba[70], e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "link 0:", "a temperature channel that is a derived channel");
        bad = good, bad.src_chan[3] = bad.out_ba[70], e = bad.view();
        expect(CHECK(&e), HEAT_E_SIZE, "node 3:", "a source channel that is a derived channel");
    }
    // ---- beside openings and controllers ----
    {
        const int32_t oz_a[1] = {3}, oz_b[1] = {-1}, otc[1] = {0}, ofc[1] = {good.out_ba[70]}, ooc[1] = {good.out_ba[71]};
        const double oarea[1] = {0.5};
        heat_openings op;
        std::memset(&op, 0, sizeof op);
        op.n_openings = 1, op.zone_a = oz_a, op.zone_b = oz_b, op.temp_chan = otc, op.out_chan = ooc, op.area = oarea;
        e = good.view();
        expect(heat_air_networks_check(&m.desc, &s, &op, nullptr, &e), HEAT_E_SIZE, "link 71:", "a derived channel that is an opening's");
        op.out_chan = ofc, op.frac_chan = nullptr;
        Networks fewer = good;
        fewer.out_ba[70] = -1, fewer.frac_chan[2] = ofc[0], e = fewer.view();
        expect(heat_air_networks_check(&m.desc, &s, &op, nullptr, &e), HEAT_E_SIZE, "link 2:", "a network that reads an opening");
        const int32_t free_chan[1] = {6};
        op.out_chan = free_chan, op.frac_chan = ofc, e = good.view();
        expect(heat_air_networks_check(&m.desc, &s, &op, nullptr, &e), HEAT_E_SIZE, "run behind the openings", "an opening that reads a network");
        const int32_t cz[1] = {3}, cset[1] = {0}, cout[1] = {4}, cen[1] = {good.out_ba[70]};
        const double ckp[1] = {0.5}, chi[1] = {1.0};
        heat_controllers ct;
        std::memset(&ct, 0, sizeof ct);
        ct.n_controllers = 1, ct.sense_index = cz, ct.set_chan = cset, ct.out_chan = cout, ct.kp = ckp, ct.out_hi = chi;
        e = good.view();
        expect(heat_air_networks_check(&m.desc, &s, nullptr, &ct, &e), HEAT_OK, nullptr, "a network that reads a controller (frac_chan 4)");
        ct.en_chan = cen;
        expect(heat_air_networks_check(&m.desc, &s, nullptr, &ct, &e), HEAT_E_SIZE, "run behind the controllers", "a controller that reads a network");
        ct.en_chan = nullptr, ct.out_chan = cen;
        expect(heat_air_networks_check(&m.desc, &s, nullptr, &ct, &e), HEAT_E_SIZE, "link 70:", "a derived channel that is a controller's");
    }
    s.n_channels = 0;
    e = good.view();
    expect(CHECK(&e), HEAT_E_SIZE, nullptr, "a series without channels");
    s.n_channels = n_channels;
    nw = good.view();
    expect(CHECK(&nw), HEAT_OK, nullptr, "the good term again");

    if (n_failed) {
        std::printf("%d checks failed\n", n_failed);
        return 1;
    }
    std::printf("air networks host check: all statuses as the header states them\n");
    return 0;
}
