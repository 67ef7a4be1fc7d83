"""Air networks of a series on the host (include/heat_amd.h, heat_air_networks): no GPU here.

The rule in numpy (heat_amd/air_networks.py, apply) against hand-worked cases, line by line; the ABI (symbols, struct layout);
every refusal of heat_air_networks_check with its code and message — the check, its table builder and the tables'
verification also run under AddressSanitizer / UBSan as a stand-alone program (tests/air_networks_host_main.cpp) in a child
process; and the generator's cases (tests/air_networks_cases.py) through the CPU oracle alone: they are accepted, every solve
converges, the signed mass into every zone is at most tol, links reverse, both regimes and the acceleration are exercised, a
cut loop equals the loop in one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import heat_amd
from heat_amd import air_networks as an, binding, modeldict as mdl
import air_networks_cases as nc
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_air_networks_check", "heat_batch_march_series_networks")
E_INVALID_ARG, E_SIZE = -1, -4
FIELDS = ("n_networks", "n_nodes", "n_links", "net_offset", "tol", "max_iter", "g_min", "node_zone", "src_chan", "src_gain", "zone_a", "zone_b",
          "temp_chan", "wp_chan", "frac_chan", "out_ab", "out_ba", "c", "gh", "p_lin", "wp_gain", "resume", "pressure", "sum_ab", "sum_ba",
          "iters_sum", "unconverged", "max_res")
OUT_OF_SCOPE = ("power-law exponents other than 1/2", "ducts and fan curves", "wind pressure coefficients from direction", "moist-air density",
                "networks of more than 64 zones", "more than one datum per network", "any change to the march kernels or to a consumer")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_air_networks {" in header
    assert "heat_air_networks_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_networks" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("AirNetworks", "make_air_networks", "air_networks_check"))
    assert all(hasattr(heat_amd, n) for n in ("AirNetworks", "make_air_networks", "air_networks_check", "air_networks"))
    assert all(hasattr(an, n) for n in ("apply", "accumulate", "fresh", "concat", "orifice", "tall_opening", "paths"))
    flat = " ".join(header.replace("*", " ").split())
    for words in OUT_OF_SCOPE:
        assert words in flat, words                                     # what is out of scope is stated
    assert "heat_air_networks, below" in flat                           # the openings' comment points to the new term
    kernels = open(os.path.join(ROOT, "heat_amd", "csrc", "series_kernels.hip")).read()
    assert "k_series_networks" in kernels and "launch_series_networks" in kernels
    assert L.heat_amd_abi_version() == 1
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW) and "pub struct HeatAirNetworks" in rust


def test_air_networks_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = ["sizeof(heat_air_networks)", "sizeof(heat_controllers)", "sizeof(heat_openings)", "sizeof(heat_series_call)"] + [
        "offsetof(heat_air_networks, %s)" % f for f in FIELDS]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == ([C.sizeof(binding.AirNetworks), C.sizeof(binding.Controllers), C.sizeof(binding.Openings), C.sizeof(binding.SeriesCall)] +
                   [getattr(binding.AirNetworks, f).offset for f in FIELDS])
    assert [f for f, _ in binding.AirNetworks._fields_] == list(FIELDS)
    # every field is 8 bytes wide; the structs beside it are as they were
    assert got[0] == 8 * len(FIELDS) and got[4:] == [8 * i for i in range(len(FIELDS))]
    assert got[1] == 8 * 26 and got[2] == 8 * 17 and got[3] == 8 * 24


# ---- the rule in numpy: hand-worked cases ----
# channel 0 the outside temperature, 1 a wind pressure, 2 an open fraction, 3 a fan, 4 and 5 derived, 6 a bystander
ROW = np.array([5.0, 2.0, 0.5, -0.01, np.nan, np.nan, 7.0])
RHO = lambda t: 101325. * 28.97 / (8314.46261815324 * (t + 273.15))   # noqa: E731


def one_zone(**more):
    return dict(dict(net_offset=[0, 1], tol=[1e-9], max_iter=[40], g_min=[1e-12], node_zone=[0], zone_a=[0], zone_b=[-1], temp_chan=[0], c=[0.05],
                     p_lin=[0.01]), **more)


def run(nw, T=(21.0,), row=ROW, state=None):
    state = an.fresh(nw) if state is None else state
    new, rec = an.apply(np.asarray(T), row, nw, state)
    return new, rec, state


def test_one_zone_with_one_link_ends_where_the_pressure_difference_vanishes():
    """Without a source nothing flows through a single link: P ends where dp = 0, at wp_gain * row[wp_chan] + gh * (ra - rb)."""
    nw = one_zone(wp_chan=[1], wp_gain=[1.5], gh=[20.0], out_ba=[4], out_ab=[5])
    new, rec, st = run(nw)
    want = 1.5 * 2.0 + 20.0 * (RHO(21.0) - RHO(5.0))
    assert rec["converged"][0] and abs(st["pressure"][0] - want) < 1e-7 and abs(rec["link_q"][0]) < 1e-6
    assert np.array_equal(st["pressure"], rec["node_p"]) and np.isnan(ROW[4])           # the row itself is not written
    assert new[4] == rec["ba"][0] and new[5] == rec["ab"][0] and np.array_equal(np.delete(new, [4, 5]), np.delete(ROW, [4, 5]))
    # with an extract fan the link carries the fan's mass in: rho(outside) q = 0.01 kg/s
    new, rec, st = run(dict(nw, src_chan=[3]))
    assert rec["converged"][0] and rec["link_q"][0] < 0 and abs(RHO(5.0) * rec["ba"][0] - 0.01) <= 1e-9 and rec["ab"][0] == 0.0
    assert new[4] == -rec["link_q"][0] and new[5] == 0.0


def test_two_openings_at_two_heights_give_the_closed_form_of_a_stack():
    """A warm zone with two equal openings to cold outside air, H apart: the neutral plane lies between them, the cold air
    enters below and leaves above, equal and opposite in mass to tol. With equal c the mass balance rho_out c sqrt(dp_low) =
    rho_in c sqrt(dp_high) and dp_low + dp_high = g H (rho_out - rho_in) give q_low = c sqrt(g H drho / (1 + (rho_out / rho_in)^2))."""
    H, c, Ti, To = 3.0, 0.04, 24.0, 5.0
    nw = one_zone(zone_a=[0, 0], zone_b=[-1, -1], temp_chan=[0, 0], c=[c, c], gh=[an.G * 1.0, an.G * (1.0 + H)], p_lin=[1e-4, 1e-4], out_ba=[4, 5])
    new, rec, st = run(nw, T=(Ti,))
    ri, ro = RHO(Ti), RHO(To)
    q_low, q_high = rec["link_q"]
    assert rec["converged"][0] and q_low < 0 < q_high                                   # in below (b -> a), out above (a -> b)
    assert abs(ro * -q_low - ri * q_high) <= 1e-9                                        # equal and opposite in mass, to tol
    drive = an.G * H * (ro - ri)
    want_low = c * np.sqrt(drive / (1.0 + (ro / ri) ** 2))
    assert abs(-q_low - want_low) <= 1e-6 * want_low
    assert new[4] == -q_low and new[5] == 0.0


def test_the_regimes_meet_at_p_lin_and_the_law_follows_the_rule_line_by_line():
    """dp is set through the pressure of the one node: tol is huge, so the first assembly stops the solve and the flows written
    are those of the pressure given."""
    p_lin = 0.09
    s_lin = np.sqrt(p_lin)
    for ad in (np.nextafter(p_lin, 0.0), p_lin, np.nextafter(p_lin, 1.0)):
        for sign in (1.0, -1.0):
            nw = one_zone(tol=[1e9], p_lin=[p_lin], c=[0.3], gh=[0.0])
            st = dict(an.fresh(nw), pressure=np.array([sign * ad]))
            _, rec, _ = run(nw, state=st)
            assert rec["net_iters"][0] == 0 and rec["converged"][0]
            want = 0.3 * np.sqrt(ad) if ad >= p_lin else (0.3 * ad) / s_lin
            assert rec["link_q"][0] == sign * want and bool(rec["root"][0]) == (ad >= p_lin)
    # the two laws agree at p_lin to rounding: C sqrt(p) against C p / sqrt(p)
    assert abs(0.3 * np.sqrt(p_lin) - (0.3 * p_lin) / s_lin) <= 1e-16


def test_the_open_fraction_is_clamped_at_both_ends():
    for f, want in ((-0.3, 0.0), (0.0, 0.0), (0.25, 0.25), (1.0, 1.0), (1.4, 1.0)):
        row = ROW.copy()
        row[2] = f
        nw = one_zone(tol=[1e9], frac_chan=[2], c=[0.3])
        _, rec, _ = run(nw, row=row, state=dict(an.fresh(nw), pressure=np.array([4.0])))
        d0 = 4.0 - 0.0
        assert rec["link_q"][0] == (0.3 * want) * np.sqrt(d0 - 0.0 * (RHO(21.0) - RHO(5.0)))


def two_zones(swap):
    a, b = (1, 0) if swap else (0, 1)
    return dict(net_offset=[0, 2], tol=[1e-10], max_iter=[40], g_min=[1e-12], node_zone=[0, 1], zone_a=[a, 0, 1], zone_b=[b, -1, -1],
                temp_chan=[-1, 0, 0], wp_chan=[-1, 1, -1], c=[0.5, 0.03, 0.04], gh=[12.0, 5.0, 30.0], p_lin=[0.01] * 3,
                out_ab=[5 if swap else 4, -1, -1], out_ba=[4 if swap else 5, -1, -1])


def test_swapping_the_ends_of_a_link_negates_its_flow_and_swaps_its_channels_bit_for_bit():
    T = (19.0, 26.0)
    new0, rec0, st0 = run(two_zones(False), T=T)
    new1, rec1, st1 = run(two_zones(True), T=T)
    assert rec0["converged"][0] and rec0["link_q"][0] != 0.0 and rec0["net_iters"][0] == rec1["net_iters"][0]
    assert rec1["link_q"][0] == -rec0["link_q"][0] and np.array_equal(rec1["link_q"][1:], rec0["link_q"][1:])
    assert rec1["ab"][0] == rec0["ba"][0] and rec1["ba"][0] == rec0["ab"][0]
    assert np.array_equal(new0, new1) and np.array_equal(st0["pressure"], st1["pressure"])


def test_the_elimination_runs_in_the_order_written_with_entries_fifteen_orders_apart():
    """Three zones in a row, the middle doorways fifteen orders of magnitude more open than the cracks to outside: one Newton
    step of apply() against the elimination and the back-substitution written out with Python floats in the header's order. A
    pivoted or reordered elimination rounds otherwise. Zones 0 and 1 are joined by three links, the second of them given the
    other way round: an entry of A takes them in ascending link number, whichever way round each is."""
    nw = dict(net_offset=[0, 3], tol=[0.0], max_iter=[1], g_min=[1e-12], node_zone=[0, 1, 2], zone_a=[0, 1, 0, 2, 1, 0], zone_b=[1, 2, -1, -1, 0, 1],
              temp_chan=[-1, -1, 0, 0, -1, -1], c=[1e8, 3e7, 1e-8, 2e-8, 2.3e7, 5.7e6], gh=[0.0, 0.0, 3.0, 40.0, 1.0, 2.0], p_lin=[5.0] * 6)
    T = np.array([21.0, 22.0, 23.0])
    st = dict(an.fresh(nw), pressure=np.array([0.3, 0.1, -0.2]))
    P0 = st["pressure"].copy()
    _, rec, _ = run(nw, T=T, state=st)
    # the assembly by hand (every link in the linear regime: |dp| < 5)
    r = [float(RHO(t)) for t in T] + [float(RHO(5.0))]
    s_lin = float(np.sqrt(5.0))
    A = [[1e-12, 0.0, 0.0], [0.0, 1e-12, 0.0], [0.0, 0.0, 1e-12]]
    F = [0.0, 0.0, 0.0]
    for a, b, c, gh in ((0, 1, 1e8, 0.0), (1, 2, 3e7, 0.0), (0, -1, 1e-8, 3.0), (2, -1, 2e-8, 40.0), (1, 0, 2.3e7, 1.0), (0, 1, 5.7e6, 2.0)):
        ra, rb = r[a], r[b]
        dp = (float(P0[a]) - (float(P0[b]) if b >= 0 else 0.0)) - gh * (ra - rb)
        q, gq = (c * abs(dp)) / s_lin, c / s_lin
        ru = ra if dp >= 0.0 else rb
        m, gm = ru * q, ru * gq
        ms = m if dp >= 0.0 else -m
        F[a] = F[a] - ms
        A[a][a] = A[a][a] + gm
        if b >= 0:
            F[b] = F[b] + ms
            A[b][b] = A[b][b] + gm
            A[a][b] = A[a][b] - gm
            A[b][a] = A[b][a] - gm
    for kk in range(3):
        for rr in range(kk + 1, 3):
            fac = A[rr][kk] / A[kk][kk]
            for j in range(kk + 1, 3):
                A[rr][j] = A[rr][j] - fac * A[kk][j]
            F[rr] = F[rr] - fac * F[kk]
    d = [0.0, 0.0, 0.0]
    for j in (2, 1, 0):
        d[j] = F[j] / A[j][j]
        for rr in range(j):
            F[rr] = F[rr] - A[rr][j] * d[j]
    assert rec["net_iters"][0] == 1 and not rec["converged"][0]
    assert [float(v) for v in rec["node_p"]] == [float(P0[i]) + d[i] for i in range(3)]
    assert max(A[0][0], A[1][1]) / 2e-8 > 1e15


def test_a_nan_is_data_and_stops_its_network_at_once():
    row = ROW.copy()
    row[0] = np.nan
    nw = an.concat(one_zone(out_ba=[4]), dict(one_zone(out_ba=[5]), node_zone=[1], zone_a=[1], temp_chan=[6], src_chan=[3]))
    st = dict(an.fresh(nw), pressure=np.array([0.7, 0.0]))
    new, rec, st = run(nw, T=(21.0, 22.0), row=row, state=st)
    assert np.isnan(rec["link_q"][0]) and np.isnan(new[4]) and rec["net_iters"][0] == 0 and rec["converged"][0] and st["pressure"][0] == 0.7
    assert np.isfinite(rec["link_q"][1]) and rec["net_iters"][1] > 0 and rec["converged"][1] and rec["res"][0] == 0.0
    acc = an.fresh(nw)
    an.accumulate(rec, acc)
    assert np.isnan(acc["sum_ba"][0]) and np.isfinite(acc["sum_ba"][1]) and acc["unconverged"].tolist() == [0, 0] and acc["iters_sum"][0] == 0


def test_the_conveniences():
    assert an.orifice(0.5, 0.6) == 0.6 * 0.5 * np.sqrt(2.0 / 1.2)
    t = an.tall_opening(0.9, 2.0, 0.6, sill=3.0)
    assert t["c"].tolist() == [float(an.orifice(0.9, 0.6))] * 2 and t["gh"].tolist() == [an.G * 3.5, an.G * 4.5]
    nw = two_zones(False)
    nw = dict(nw, out_ba=[5, 6, -1])
    p = an.paths(nw)
    assert p["target"].tolist() == [1, 0, 0] and p["source"].tolist() == [0, 1, -1] and p["temp_chan"].tolist() == [-1, -1, 0]
    assert p["volume_chan"].tolist() == [4, 5, 6] and p["link"].tolist() == [0, 0, 1]
    both = an.concat(one_zone(), dict(two_zones(False), node_zone=[3, 4], zone_a=[3, 3, 4], zone_b=[4, -1, -1]))
    assert both["net_offset"].tolist() == [0, 1, 3] and both["node_zone"].tolist() == [0, 3, 4] and both["wp_chan"].tolist() == [-1, -1, 1, -1]
    assert both["out_ab"].tolist() == [-1, 4, -1, -1] and both["gh"].tolist() == [0.0, 12.0, 5.0, 30.0]


# ---- heat_air_networks_check: every refusal with its code and what it names ----
@pytest.fixture(scope="module")
def model():
    md, _ = mdl.clustered_massive(200, Z=8, seed=3)
    return md


def good():
    return dict(net_offset=[0, 2, 3], tol=[1e-7, 1e-7], max_iter=[24, 24], g_min=[1e-9, 1e-9], node_zone=[1, 4, 6], src_chan=[-1, 1, -1],
                zone_a=[1, 1, 4, 6], zone_b=[4, -1, -1, -1], temp_chan=[-1, 0, 0, 0], wp_chan=[-1, 2, -1, 2], frac_chan=[-1, 9, -1, 3],
                out_ab=[5, -1, -1, -1], out_ba=[6, 7, -1, 8], c=[0.5, 0.02, 0.03, 0.02], gh=[9.81, 4.0, 20.0, 9.81], p_lin=[0.1] * 4)


OPENING = dict(zone_a=[2], zone_b=[-1], temp_chan=[0], out_chan=[4], area=[0.5], cs=[9.0], c0=[0.01])
CONTROLLER = dict(sense_index=[1], set_chan=[1], out_chan=[9], kp=[0.5], out_hi=[1.0])


def check(model, nw, openings=OPENING, controllers=CONTROLLER):
    try:
        binding.air_networks_check(model, nw, openings=openings, controllers=controllers, weather=np.zeros((2, 1, 3)), n_sub=1,
                                   channel=np.zeros((2, 10)))
    except heat_amd.HeatError as e:
        return e.code, str(e)
    return 0, ""


def changed(nw, key, i, v):
    out = dict(nw)
    out[key] = list(nw[key])
    out[key][i] = v
    return out


def test_a_good_term_is_accepted_alone_and_beside_openings_and_controllers(model):
    assert check(model, good()) == (0, "")
    assert check(model, changed(good(), "frac_chan", 1, -1), openings=None, controllers=None) == (0, "")
    assert check(model, None) == (0, "") and check(model, {}) == (0, "")
    assert check(model, dict(good(), resume=an.fresh(good()))) == (0, "")


def test_every_refusal_names_its_network_node_or_link(model):
    g = good()
    resumed = lambda **kw: dict(g, resume=dict(an.fresh(g), **kw))   # noqa: E731
    for bad, code, needle in ((changed(g, "net_offset", 0, 1), E_SIZE, "network 0: net_offset starts"),
                              (dict(g, net_offset=[0, 3, 3]), E_SIZE, "network 1: 0 nodes"),
                              (dict(g, net_offset=[0, 2, 2]), E_SIZE, "network 1: 0 nodes"),
                              (dict(g, net_offset=[0, 1, 2]), E_SIZE, "network 1: net_offset ends at 2"),
                              (changed(g, "tol", 1, -1e-9), E_INVALID_ARG, "network 1: tol"),
                              (changed(g, "tol", 0, np.inf), E_INVALID_ARG, "network 0: tol"),
                              (changed(g, "g_min", 0, 0.0), E_INVALID_ARG, "network 0: g_min"),
                              (changed(g, "g_min", 1, np.nan), E_INVALID_ARG, "network 1: g_min"),
                              (changed(g, "max_iter", 1, 0), E_INVALID_ARG, "network 1: max_iter"),
                              (changed(g, "max_iter", 0, 65), E_INVALID_ARG, "network 0: max_iter"),
                              (changed(g, "node_zone", 2, 8), E_SIZE, "node 2: zone 8"),
                              (changed(g, "node_zone", 0, -1), E_SIZE, "node 0: zone -1"),
                              (changed(g, "node_zone", 2, 4), E_SIZE, "node 2: zone 4 is a node of network 0"),
                              (changed(g, "src_chan", 1, 10), E_SIZE, "node 1: source channel"),
                              (dict(g, src_gain=[1.0, np.inf, 1.0]), E_INVALID_ARG, "node 1: src_gain"),
                              (resumed(pressure=[0.0, 0.0, np.nan]), E_INVALID_ARG, "node 2: pressure"),
                              (changed(g, "zone_a", 0, 8), E_SIZE, "link 0: zone_a"),
                              (changed(g, "zone_b", 0, -2), E_SIZE, "link 0: zone_b"),
                              (changed(g, "zone_b", 0, 1), E_INVALID_ARG, "link 0: zone_a == zone_b"),
                              (changed(g, "zone_b", 0, 6), E_SIZE, "link 0: zone_a 1 is in network 0 and zone_b 6 in 1"),
                              (changed(g, "zone_a", 3, 2), E_SIZE, "link 3: zone_a 2 is in no network"),
                              (changed(g, "temp_chan", 1, -1), E_SIZE, "link 1: a link to outside without a temperature channel"),
                              (changed(g, "temp_chan", 0, 0), E_SIZE, "link 0: a link between zones with an outside channel"),
                              (changed(g, "wp_chan", 0, 2), E_SIZE, "link 0: a link between zones with an outside channel"),
                              (changed(g, "temp_chan", 2, 10), E_SIZE, "link 2: temp_chan"),
                              (changed(g, "wp_chan", 1, -2), E_SIZE, "link 1: wp_chan"),
                              (changed(g, "frac_chan", 2, 10), E_SIZE, "link 2: frac_chan"),
                              (changed(g, "out_ab", 2, 10), E_SIZE, "link 2: out_ab"),
                              (changed(g, "out_ba", 2, -2), E_SIZE, "link 2: out_ba"),
                              (changed(g, "c", 1, -0.02), E_INVALID_ARG, "link 1: c"),
                              (changed(g, "c", 1, np.nan), E_INVALID_ARG, "link 1: c"),
                              (changed(g, "gh", 2, -1.0), E_INVALID_ARG, "link 2: gh"),
                              (changed(g, "p_lin", 3, 0.0), E_INVALID_ARG, "link 3: p_lin"),
                              (changed(g, "p_lin", 3, np.inf), E_INVALID_ARG, "link 3: p_lin"),
                              (dict(g, wp_gain=[1.0, np.nan, 1.0, 1.0]), E_INVALID_ARG, "link 1: wp_gain"),
                              (changed(g, "zone_a", 3, 4), E_SIZE, "network 1: no link to outside"),
                              (changed(g, "out_ba", 1, 6), E_SIZE, "link 1: its derived channel out_ba 6 is also link 0's"),
                              (changed(g, "out_ab", 0, 6), E_SIZE, "link 0: its derived channel out_ba 6 is also link 0's"),
                              (changed(g, "out_ba", 1, 4), E_SIZE, "link 1: its derived channel out_ba 4 is also opening 0's"),
                              (changed(g, "out_ab", 0, 9), E_SIZE, "link 0: its derived channel out_ab 9 is also controller 0's"),
                              (changed(g, "frac_chan", 1, 4), E_SIZE, "link 1: its frac_chan 4 is the derived channel of opening 0"),
                              (changed(g, "frac_chan", 1, 8), E_SIZE, "link 1: its frac_chan 8 is the derived channel of link 3"),
                              (changed(g, "temp_chan", 2, 5), E_SIZE, "link 2: its temp_chan 5 is the derived channel of link 0"),
                              (changed(g, "wp_chan", 3, 7), E_SIZE, "link 3: its wp_chan 7 is the derived channel of link 1"),
                              (changed(g, "src_chan", 1, 6), E_SIZE, "node 1: its src_chan 6 is the derived channel of link 0"),
                              (changed(g, "src_chan", 1, 4), E_SIZE, "node 1: its src_chan 4 is the derived channel of opening 0")):
        got, msg = check(model, bad)
        assert got == code and needle in msg, (msg, needle)
    # the networks run behind the openings and the controllers: neither reads a network's derived channel
    got, msg = check(model, g, openings=dict(OPENING, frac_chan=[7]))
    assert got == E_SIZE and "link 1: its derived channel 7 is read by opening 0" in msg
    got, msg = check(model, g, controllers=dict(CONTROLLER, en_chan=[5]))
    assert got == E_SIZE and "link 0: its derived channel 5 is read by controller 0" in msg
    # a bad opening or controller is its own refusal; a series without channels
    got, msg = check(model, g, openings=dict(OPENING, area=[-1.0]))
    assert got == E_INVALID_ARG and "opening 0:" in msg
    got, msg = check(model, g, controllers=dict(CONTROLLER, kp=[-1.0]))
    assert got == E_INVALID_ARG and "controller 0:" in msg


def test_counts_and_null_arrays_are_refused_through_the_c_abi(model):
    L = binding.load_library()
    desc, keep = binding.make_desc(model)
    s, skeep = binding.make_series(weather=np.zeros((2, 1, 3)), n_sub=1, channel=np.zeros((2, 10)))
    g = {k: v for k, v in good().items() if k not in ("frac_chan",)}

    def raw(**fields):
        nw, nkeep = binding.make_air_networks(**g)
        for k, v in fields.items():
            setattr(nw, k, v)
        rc = L.heat_air_networks_check(C.byref(desc), C.byref(s), None, None, C.byref(nw))
        return rc, L.heat_last_error().decode()

    assert raw()[0] == 0
    for field, needle in (("net_offset", "network 0: net_offset"), ("tol", "network 0: tol"), ("max_iter", "network 0: max_iter"),
                          ("g_min", "network 0: g_min"), ("node_zone", "node 0: node_zone"), ("zone_a", "link 0: zone_a"),
                          ("zone_b", "link 0: zone_b"), ("temp_chan", "link 0: temp_chan"), ("c", "link 0: c"), ("p_lin", "link 0: p_lin")):
        rc, msg = raw(**{field: None})
        assert rc == E_INVALID_ARG and needle in msg, (field, msg)
    for field in ("src_chan", "src_gain", "wp_chan", "out_ab", "out_ba", "gh", "wp_gain") + binding.NETWORK_STATE + binding.NETWORK_STATS:   # nullable
        rc, msg = raw(**{field: None})
        assert rc == 0, (field, msg)
    for field in ("n_networks", "n_nodes", "n_links"):
        rc, msg = raw(**{field: -1})
        assert rc == E_INVALID_ARG and "negative count" in msg, msg
    rc, msg = raw(n_networks=0)
    assert rc == E_SIZE and "network 0:" in msg
    rc, msg = raw(n_networks=0, n_nodes=0, n_links=0)
    assert rc == 0, msg


def test_air_networks_check_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "air_networks_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "air networks host check: all statuses as the header states them" in out.stdout


# ---- the generator's cases: accepted, and — through the CPU oracle alone — they hold their conditions ----
COVERAGE_CASES = [("ragged_mixed", 2, True, nc.TOL), ("ragged_mixed", 5, True, nc.TOL), ("ragged_mixed", 2, False, nc.TOL),
                  ("rooms_with_windows_large", 2, False, nc.TOL), ("ragged_mixed", 2, True, 0.0), ("ragged_mixed", 5, True, 0.0)]
_LOOPS = {}


def oracle_loop(oracle, model_name, n_sub, floor, tol):
    key = (model_name, n_sub, floor, tol)
    if key not in _LOOPS:
        c = nc.case(model_name, nc.N_STEPS, n_sub, 2, nc.SEED, floor=floor, tol=tol)
        m = oracle.OracleModel(c["md"])

        def march(s, wk, za, zb):
            assert m.march(s, wk, za, zb, threads=1)[0] == 0

        state = c["st"].copy()
        _LOOPS[key] = (c, march, nc.loop_with_rules(march, c, state), state)
    return _LOOPS[key]


@pytest.mark.parametrize("model_name,n_sub,floor,tol", COVERAGE_CASES)
def test_the_generators_cases_are_accepted_and_hold_their_conditions(oracle, model_name, n_sub, floor, tol):
    c, march, out, _ = oracle_loop(oracle, model_name, n_sub, floor, tol)
    md, nw, info = c["md"], c["networks"], c["networks_info"]
    kw = dict(weather=c["w"], n_sub=n_sub, channel=c["channel"], probes=c["probes"])
    binding.air_networks_check(md, nw, openings=c["openings"], controllers=c["controllers"], **kw)
    binding.air_species_check(md, c["species"], loads=c["loads"], air=c["air"], handlers=c["handlers"], **kw)
    # what the generator promises: every zone a node, the sizes, every derived column read by one air path, windows behind controllers
    Z, sizes = int(md["n_zones"]), sorted(info["sizes"].tolist())
    assert sorted(nw["node_zone"].tolist()) == list(range(Z)) and set(nc.SIZES[Z]) <= set(sizes) and set(sizes) - set(nc.SIZES[Z]) <= {3, 5}
    # the launch geometry: on 500 zones every width class has a full wavefront of networks and, where a workgroup holds more than
    # one network, a ragged last one; 20 zones are two launches of less than a wavefront each
    shapes = nc.wave_shapes(sizes)
    if Z == 500:
        assert all(full >= 1 for _, full, _ in shapes.values()) and all(shapes[w][2] >= 1 for w in (8, 16, 32)), shapes
        assert shapes[16][0] >= 5 and shapes[32][0] >= 3 and shapes[64] == (2, 2, 0), shapes
    else:
        assert shapes == {8: (3, 0, 3), 16: (1, 0, 1), 32: (0, 0, 0), 64: (0, 0, 0)}, shapes
    written = np.concatenate([nw["out_ab"][nw["out_ab"] >= 0], nw["out_ba"][nw["out_ba"] >= 0]])
    assert sorted(written.tolist()) == info["derived"].tolist() and np.isnan(c["channel"][:, info["derived"]]).all()
    assert sorted(np.asarray(c["air"]["volume_chan"])[info["paths"]].tolist()) == info["derived"].tolist()
    assert len(info["auto"]) >= 2 and set(nw["frac_chan"][info["auto"]].tolist()) <= set(np.asarray(c["controllers"]["out_chan"])[info["windows"]].tolist())
    assert len(info["fans"]) >= 2 and float(nw["c"].max()) <= nc.C_MAX and (not floor or float(nw["p_lin"].min()) >= 0.1)
    # two links of the same two zones (the tall openings), loops, and a shuffled list
    pair = set()
    twice = 0
    for a, b in zip(nw["zone_a"].tolist(), nw["zone_b"].tolist()):
        if b >= 0:
            twice += (min(a, b), max(a, b)) in pair
            pair.add((min(a, b), max(a, b)))
    assert twice >= len(pair) // 3
    # the conditions, on the oracle loop alone
    nc.assert_coverage(nc.coverage(c, out), "%s n_sub=%d floor=%s tol=%g" % (model_name, n_sub, floor, tol), tol=tol)
    for key in ("trace", "link_q", "node_p", "path_q", "conc_rows", "control_u"):
        assert np.all(np.isfinite(out[key])), key
    # sum of signed mass into every zone at every converged step
    conv = out["converged"][:, info["plan"]["node_net"]]
    assert (np.abs(out["mass_in"][conv]) <= max(tol, 0.0)).all() and conv.any()
    # the rows hold the flows, and the air paths carry them: the path's volume is the link's flow in its direction
    q = out["link_q"]
    assert np.array_equal(out["rows"][:, nw["out_ba"][nw["out_ba"] >= 0]], np.where(q < 0, -q, 0.0)[:, nw["out_ba"] >= 0])
    assert np.array_equal(out["rows"][:, nw["out_ab"][nw["out_ab"] >= 0]], np.where(q > 0, q, 0.0)[:, nw["out_ab"] >= 0])
    # the accumulators are the sums of the returned rows
    acc = out["carry"]["networks"]
    assert np.array_equal(acc["iters_sum"], out["net_iters"].sum(axis=0)) and np.array_equal(acc["unconverged"], (~out["converged"]).sum(axis=0))
    assert np.array_equal(acc["pressure"], out["node_p"][-1])
    gap = nc.margin(c, out)
    print("%s n_sub=%d: least distance of a decision from its threshold %.3e K" % (model_name, n_sub, gap))
    if floor:
        assert gap >= nc.MARGIN, gap


def test_a_cut_loop_equals_the_loop_in_one(oracle):
    c, march, one_, s1 = oracle_loop(oracle, "ragged_mixed", 2, True, nc.TOL)
    s2 = c["st"].copy()
    first = nc.loop_with_rules(march, c, s2, steps=slice(0, 9))
    second = nc.loop_with_rules(march, c, s2, steps=slice(9, None), carry=first["carry"], step_base=0)
    assert np.array_equal(s1, s2)
    for key in ("link_q", "node_p", "net_iters", "control_u", "opening_v", "trace", "path_q"):
        assert np.array_equal(one_[key], np.concatenate([first[key], second[key]])), key
    for key in an.STATE + an.ACC:
        assert np.array_equal(one_["carry"]["networks"][key], second["carry"]["networks"][key]), key
    assert (first["carry"]["networks"]["pressure"] != 0).all()
