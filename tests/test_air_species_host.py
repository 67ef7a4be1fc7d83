"""Air species of a series on the host (include/heat_amd.h, heat_air_species / heat_air_species_check /
heat_batch_march_series_species; heat_amd/air_species.py): the entry points are declared, exported and bound; the ctypes mirror
has the header's layout; the rule in numpy (air_species.apply — the reference of tests/test_air_species_gpu.py) gives the
hand-worked single-zone cases at, one ulp below and one ulp above every threshold; every refusal the header lists comes back with
its code and names the species, the source or the vent, before any device work; the generator's cases are accepted and — run
through the CPU oracle alone — open and close paths, saturate and release vents and cross a limit. heat_air_species_check — with
the table builder and its verification — also runs under AddressSanitizer / UBSan as a stand-alone program
(tests/air_species_host_main.cpp) in a child process. No GPU needed.

Reference: the rule is this project's own (the reference has no counterpart: zone.rs, model.rs:500-597); the air properties are
the reference's (gas.rs:49,165-179)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import heat_amd
from heat_amd import air_species as asp, binding, modeldict as mdl
import air_species_cases as asc
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_air_species_check", "heat_batch_march_series_species")
E_INVALID_ARG, E_SIZE = -1, -4
FIELDS = ("n_species", "outdoor_chan", "n_sources", "src_zone", "src_species", "src_chan", "src_factor", "n_vents", "vent_zone",
          "vent_species", "vent_temp_chan", "vent_enable_chan", "vent_v_min", "vent_v_max", "vent_c_lo", "vent_c_hi", "limit_chan",
          "occ_chan", "resume", "step_base", "conc", "n_occupied", "sum_conc", "max_conc", "step_max", "n_above", "excess_above",
          "sum_volume", "sum_q", "steps_saturated")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_air_species {" in header
    assert "heat_air_species_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_species" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("AirSpecies", "make_air_species", "air_species_check"))
    assert all(hasattr(heat_amd, n) for n in ("AirSpecies", "make_air_species", "air_species_check", "air_species"))
    assert all(hasattr(asp, n) for n in ("apply", "accumulate", "fresh", "concat", "per_zone"))
    for word in ("density differences", "recirculating", "sorption", "latent heat", "deposition"):
        assert word in header, word                                     # what is out of scope is stated
    assert L.heat_amd_abi_version() == 1
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW)


def test_air_species_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = (["sizeof(heat_air_species)", "sizeof(heat_air_paths)", "sizeof(heat_air_handlers)", "sizeof(heat_series_call)", "sizeof(heat_series)",
             "sizeof(heat_zone_loads)", "sizeof(heat_comfort)"] + ["offsetof(heat_air_species, %s)" % f for f in FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    # (the structs beside it keep their sizes: the species are a struct of their own, heat_series_call is as it was)
    assert got == ([C.sizeof(binding.AirSpecies), C.sizeof(binding.AirPaths), C.sizeof(binding.AirHandlers), C.sizeof(binding.SeriesCall),
                    C.sizeof(binding.Series), C.sizeof(binding.ZoneLoads), C.sizeof(binding.Comfort)] +
                   [getattr(binding.AirSpecies, f).offset for f in FIELDS])
    assert [f for f, _ in binding.AirSpecies._fields_] == list(FIELDS)
    # every field is 8 bytes wide
    assert got[0] == 8 * len(FIELDS) and got[7:] == [8 * i for i in range(len(FIELDS))]
    assert got[1] == 8 * 14 and got[2] == 8 * 26 and got[3] == 8 * 24


# ---- the rule in numpy: hand-worked single-zone cases ----
# channel 0 the outdoor level, 1 the outdoor temperature, 2 a volume, 3 a source, 4 enable, 5 the limit, 6 occupancy
CO, TIN, VOL, H = 400.0, 5.0, 250.0, 90.0
C_LO, C_HI, V_MIN, V_MAX = 600.0, 1000.0, 0.01, 0.09


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def flow(t_in, v):
    tk = t_in + 273.15
    rho, cp = 101325. * 28.97 / (8314.46261815324 * tk), 1002.7370 + 1.2324e-2 * tk
    return (rho * v) * cp


def vent(**more):
    return dict(dict(outdoor_chan=np.array([[0]]), vent_zone=[0], vent_species=[0], vent_temp_chan=[1], vent_v_min=[V_MIN], vent_v_max=[V_MAX],
                     vent_c_lo=[C_LO], vent_c_hi=[C_HI]), **more)


def step(species, c, row=None, T=20.0, **terms):
    conc = np.array([[c]])
    row = np.array([CO, TIN, 0.03125, 2.0, 1.0, 900.0, 1.0]) if row is None else row
    a0, b0, rows = asp.apply(np.array([T]), conc, row, np.array([7.0]), np.array([2.0]), species, np.array([VOL]), H, **terms)
    return conc[0, 0], a0, b0, rows


def test_a_vent_follows_the_concentration_between_its_limits():
    c = 800.0
    new, a0, b0, rows = step(vent(), c)
    f = (c - C_LO) / (C_HI - C_LO)
    V = V_MIN + f * (V_MAX - V_MIN)
    m = flow(TIN, V)
    assert f == 0.5 and rows["vent_v"][0] == V and not rows["saturated"][0]
    assert a0[0] == 7.0 + m * TIN and b0[0] == 2.0 + m and rows["vent_q"][0] == m * (TIN - 20.0) and rows["vent_q"][0] < 0.0
    # the balance: the vent is the only inflow, it carries the outside air's level
    assert new == (VOL * c + H * (0.0 + V * CO)) / (VOL + H * V) and rows["conc"][0, 0] == c and new < c
    # f at, one ulp below and one ulp above 0 ...
    for c, want_f in ((C_LO, 0.0), (down(C_LO), 0.0), (up(C_LO), (up(C_LO) - C_LO) / (C_HI - C_LO))):
        rows = step(vent(), c)[3]
        assert rows["vent_v"][0] == V_MIN + want_f * (V_MAX - V_MIN) and not rows["saturated"][0], c
    assert step(vent(), up(C_LO))[3]["vent_v"][0] > V_MIN == step(vent(), down(C_LO))[3]["vent_v"][0]
    # ... and 1: f == 1.0 is saturated, reached exactly or clamped
    for c, sat in ((C_HI, True), (up(C_HI), True), (down(C_HI), False), (5000.0, True)):
        rows = step(vent(), c)[3]
        f = min((c - C_LO) / (C_HI - C_LO), 1.0)
        assert rows["saturated"][0] == sat and rows["vent_v"][0] == V_MIN + f * (V_MAX - V_MIN), c
    assert step(vent(), down(C_HI))[3]["vent_v"][0] < V_MIN + 1.0 * (V_MAX - V_MIN)


def test_a_disabled_vent_moves_nothing_and_is_not_saturated():
    row = np.array([CO, TIN, 0.03125, 2.0, 0.0, 900.0, 1.0])
    for enable in (0.0, -1.0, np.nan):                                   # not row[enable] > 0
        row[4] = enable
        new, a0, b0, rows = step(vent(vent_enable_chan=[4]), 5000.0, row=row)
        assert rows["vent_v"][0] == 0.0 and rows["vent_q"][0] == 0.0 and not rows["saturated"][0] and a0[0] == 7.0 and b0[0] == 2.0
        assert new == (VOL * 5000.0 + H * (0.0 + 0.0 * CO)) / (VOL + H * 0.0)
    row[4] = up(0.0)
    assert step(vent(vent_enable_chan=[4]), 5000.0, row=row)[3]["saturated"][0]
    assert step(vent(vent_enable_chan=[-1]), 5000.0, row=row)[3]["vent_v"][0] == V_MAX


def test_the_order_of_the_four_inflow_kinds_and_of_a_zones_sum():
    """Volumes seven orders of magnitude apart: F and G come out as the sums in the rule's order — flows, paths, branches, vents,
    each in the caller's order."""
    Z = 3
    T, vol = np.array([20.0, 21.0, 22.0]), np.array([VOL, 300.0, 350.0])
    row = np.array([CO, TIN, 1.0, 2.0, 1.0, 900.0, 1.0])
    v = [8.53e-05, 8.33, 0.924, 3.83e-05, 628.0, 0.369, 0.0561, 480.0]   # two flows, two paths, two supply branches, two vents
    loads = dict(flows=dict(zone=[0, 1, 0], volume_chan=[2, 2, 2], temp_chan=[1, 1, 1], volume_gain=[v[0], 0.5, v[1]]))
    air = dict(target=[0, 0, 2], source=[1, -1, 0], temp_chan=[-1, 1, -1], volume_chan=[2, 2, 2], volume_gain=[v[2], v[3], 1.0])
    handlers = dict(outdoor_chan=[1], br_unit=[0, 0, 0], br_zone=[0, 0, 0], br_volume_chan=[2, 2, 2], br_volume_gain=[v[4], 5.0, v[5]], br_kind=[1, 2, 3])
    species = dict(outdoor_chan=asp.per_zone([0], Z), src_zone=[0, 0, 1], src_species=[0, 0, 0], src_chan=[3, 3, 3], src_factor=[1e-7, 9e6, 1.0],
                   vent_zone=[0, 0], vent_species=[0, 0], vent_temp_chan=[1, 1], vent_v_min=[v[6], v[7]], vent_v_max=[v[6], v[7]], vent_c_lo=[1.0, 1.0],
                   vent_c_hi=[2.0, 2.0])
    conc = np.array([[700.0, 1300.0, 50.0]])
    a0, b0, rows = asp.apply(T, conc, row, np.array([1e9, 0.0, 0.0]), np.array([1e7, 0.0, 0.0]), species, vol, H, loads=loads, air=air,
                             air_state=np.zeros(3, np.uint8), handlers=handlers)
    inflow = [(v[0] * 1.0, CO), (v[1] * 1.0, CO), (v[2] * 1.0, 1300.0), (v[3] * 1.0, CO), (v[4] * 1.0, CO), (v[5] * 1.0, CO), (v[6], CO), (v[7], CO)]
    F = G = 0.0
    for V, ci in inflow:
        F, G = F + V, G + V * ci
    S = (0.0 + 1e-7 * 2.0) + 9e6 * 2.0
    want = (vol[0] * 700.0 + H * (S + G)) / (vol[0] + H * F)
    assert conc[0, 0] == want
    # other orders of the kinds, or of a kind's members, give other sums: the volumes are chosen so that the check above tells
    # seven of these eight apart (sums of eight terms often round alike)
    others = []
    for order in ([1, 0] + list(range(2, 8)), [2, 3, 0, 1, 4, 5, 6, 7], [0, 1, 2, 3, 6, 7, 4, 5], list(range(7, -1, -1)), [4, 5, 6, 7, 0, 1, 2, 3],
                  [0, 1, 3, 2, 4, 5, 6, 7], [0, 1, 2, 3, 5, 4, 6, 7], [0, 1, 2, 3, 4, 5, 7, 6]):
        f = g = 0.0
        for i in order:
            f, g = f + inflow[i][0], g + inflow[i][0] * inflow[i][1]
        others.append((f, g))
    assert sum(1 for fg in others if fg != (F, G)) == 7, others
    # the zone's heat sum: the vents are added behind what the row held, each in the caller's order
    m0, m1 = flow(TIN, v[6]), flow(TIN, v[7])
    assert a0[0] == (1e9 + m0 * TIN) + m1 * TIN and b0[0] == (1e7 + m0) + m1
    # zone 1 has a flow and a source; zone 2 a path from zone 0, which it reads at the start of the step
    assert conc[0, 1] == (vol[1] * 1300.0 + H * ((0.0 + 1.0 * 2.0) + (0.0 + 0.5 * CO))) / (vol[1] + H * (0.0 + 0.5))
    assert conc[0, 2] == (vol[2] * 50.0 + H * (0.0 + (0.0 + 1.0 * 700.0))) / (vol[2] + H * (0.0 + 1.0))
    assert np.array_equal(rows["conc"], [[700.0, 1300.0, 50.0]])


def test_a_closed_path_contributes_nothing_and_a_source_zone_is_read_at_the_start_of_the_step():
    Z = 3
    vol = np.array([VOL, 300.0, 350.0])
    row = np.array([CO, TIN, 0.5, 2.0, 1.0, 900.0, 1.0])
    species = dict(outdoor_chan=asp.per_zone([-1], Z))
    chain = dict(target=[1, 2], source=[0, 1], volume_chan=[2, 2], open_chan=[-1, 5], sense=[1, 1], band=[0.0, 0.0], min_delta=[0.0, 0.0])
    for state, moves in ((0, False), (1, True), (2, False)):             # open = state == 1 of a controlled path
        conc = np.array([[1000.0, 0.0, 0.0]])
        asp.apply(np.zeros(Z), conc, row, None, None, species, vol, H, air=chain, air_state=np.array([0, state], np.uint8))
        b = (vol[1] * 0.0 + H * (0.0 + 0.5 * 1000.0)) / (vol[1] + H * 0.5)
        assert conc[0, 0] == (VOL * 1000.0 + H * 0.0) / (VOL + H * 0.0) and conc[0, 1] == b   # (the uncontrolled path ignores its byte)
        # zone 2 takes what zone 1 had when the step started — nothing — however much zone 1 gains in this step
        assert conc[0, 2] == 0.0
        asp.apply(np.zeros(Z), conc, row, None, None, species, vol, H, air=chain, air_state=np.array([0, state], np.uint8))
        assert (conc[0, 2] == (vol[2] * 0.0 + H * (0.0 + 0.5 * b)) / (vol[2] + H * 0.5)) == moves and (conc[0, 2] != 0.0) == moves
    # a supply path (source -1) carries the outside air's level; an extract-only branch carries nothing
    conc = np.array([[1000.0, 0.0, 0.0]])
    out = dict(outdoor_chan=asp.per_zone([0], Z))
    asp.apply(np.zeros(Z), conc, row, None, None, out, vol, H, air=dict(target=[1], source=[-1], temp_chan=[1], volume_chan=[2]),
              air_state=np.zeros(1, np.uint8), handlers=dict(outdoor_chan=[1], br_unit=[0], br_zone=[2], br_volume_chan=[2], br_kind=[2]))
    assert conc[0, 1] == (vol[1] * 0.0 + H * (0.0 + 0.5 * CO)) / (vol[1] + H * 0.5) and conc[0, 2] == 0.0


def test_nan_propagates_and_makes_every_comparison_false():
    nan = np.nan
    # a NaN concentration at a vent: f, V, m are NaN — the zone's terms with them; not saturated
    new, a0, b0, rows = step(vent(), nan)
    assert np.isnan(rows["vent_v"][0]) and np.isnan(a0[0]) and np.isnan(b0[0]) and np.isnan(new) and not rows["saturated"][0]
    # a NaN source reaches the concentration and nothing else
    row = np.array([CO, TIN, 0.03125, nan, 1.0, 900.0, 1.0])
    new, a0, b0, rows = step(vent(src_zone=[0], src_species=[0], src_chan=[3]), 800.0, row=row)
    assert np.isnan(new) and np.isfinite(a0[0]) and np.isfinite(rows["vent_v"][0])
    # the statistics: a NaN concentration is neither a maximum nor above a limit, a NaN limit is never exceeded, a NaN
    # occupancy is not occupied
    sp = dict(outdoor_chan=np.array([[-1, -1, -1]]), limit_chan=[5], occ_chan=[6, 6, -1])
    acc = asp.fresh(sp, 3)
    rows = dict(conc=np.array([[nan, 950.0, 950.0]]), vent_v=np.zeros(0), vent_q=np.zeros(0), saturated=np.zeros(0, bool))
    asp.accumulate(rows, acc, sp, np.array([0.0, 0.0, 0.0, 0.0, 0.0, 900.0, 1.0]), 7)
    assert acc["n_occupied"].tolist() == [[1, 1, 1]] and np.isnan(acc["sum_conc"][0, 0]) and acc["max_conc"][0, 0] == -np.inf
    assert acc["step_max"].tolist() == [[-1, 7, 7]] and acc["n_above"].tolist() == [[0, 1, 1]] and acc["excess_above"].tolist() == [[0.0, 50.0, 50.0]]
    asp.accumulate(rows, acc, sp, np.array([0.0, 0.0, 0.0, 0.0, 0.0, nan, nan]), 8)
    assert acc["n_occupied"].tolist() == [[1, 1, 2]] and acc["n_above"].tolist() == [[0, 1, 1]] and acc["step_max"].tolist() == [[-1, 7, 7]]
    # at, one ulp below and one ulp above the limit; the maximum keeps its first step
    acc = asp.fresh(sp, 3)
    rows["conc"] = np.array([[down(900.0), 900.0, up(900.0)]])
    asp.accumulate(rows, acc, sp, np.array([0.0, 0.0, 0.0, 0.0, 0.0, 900.0, 1.0]), 3)
    asp.accumulate(rows, acc, sp, np.array([0.0, 0.0, 0.0, 0.0, 0.0, 900.0, 1.0]), 4)
    assert acc["n_above"].tolist() == [[0, 0, 2]] and acc["step_max"].tolist() == [[3, 3, 3]] and acc["excess_above"][0, 2] == 2 * (up(900.0) - 900.0)


def test_per_zone_and_concat():
    oc = asp.per_zone([4, -1], 3)
    assert oc.dtype == np.int32 and oc.tolist() == [[4, 4, 4], [-1, -1, -1]] and oc.flags["C_CONTIGUOUS"]
    a = dict(outdoor_chan=oc, src_zone=[0], src_species=[1], src_chan=[2])
    b = dict(src_zone=[1, 2], src_species=[0, 0], src_chan=[3, 3], src_factor=[2.0, 3.0], vent_zone=[1], vent_species=[0], vent_temp_chan=[1],
             vent_v_min=[0.0], vent_v_max=[1.0], vent_c_lo=[1.0], vent_c_hi=[2.0])
    j = asp.concat(a, b)
    assert j["src_zone"].tolist() == [0, 1, 2] and j["src_factor"].tolist() == [1.0, 2.0, 3.0] and j["vent_enable_chan"].tolist() == [-1]
    assert j["outdoor_chan"] is not None and asp.n_species(j) == 2 and asp.n_sources(j) == 3 and asp.n_vents(j) == 1


# ---- refusals ----
@pytest.fixture(scope="module")
def model():
    return mdl.clustered_massive(200, Z=8, seed=3)[0]


def series(model, **more):
    return dict(dict(weather=np.zeros((2, 1, 3)), n_sub=1, channel=np.zeros((2, 7))), **more)


def good_species(model):
    Z = int(model["n_zones"])
    return dict(outdoor_chan=np.stack([np.arange(Z) % 2, np.full(Z, -1)]).astype(np.int32), conc=np.full((2, Z), 400.0),
                src_zone=np.arange(6) % Z, src_species=np.arange(6) % 2, src_chan=np.full(6, 3), src_factor=np.linspace(-1.0, 4.0, 6),
                vent_zone=[0, 3, 3, 7], vent_species=[0, 1, 0, 1], vent_temp_chan=[1, 1, 1, 1], vent_enable_chan=[-1, 4, -1, 4],
                vent_v_min=[0.0, 0.01, 0.02, 0.0], vent_v_max=[0.1, 0.01, 0.2, 0.3], vent_c_lo=[500.0, 5.0, 600.0, 6.0],
                vent_c_hi=[900.0, 9.0, 1000.0, 10.0], limit_chan=[5, -1], occ_chan=np.where(np.arange(Z) % 2, 6, -1))


def changed(g, key, i, value):
    a = np.array(g[key], dtype=np.float64 if isinstance(value, float) else None)
    a.reshape(-1)[i] = value
    return dict(g, **{key: a})


def _code(call):
    with pytest.raises(binding.HeatError) as e:
        call()
    return e.value.code, str(e.value)


def _raw(model, g, **fields):
    """heat_air_species_check with fields of the struct overwritten (a count, or None for a NULL array)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(model)
    s, skeep = binding.make_series(**series(model))
    sp, spkeep = binding.make_air_species(**g)
    for k, v in fields.items():
        setattr(sp, k, v)
    rc = L.heat_air_species_check(C.byref(desc), C.byref(s), None, None, None, C.byref(sp))
    return rc, L.heat_last_error().decode("utf-8", "replace")


def test_a_good_term_no_term_and_an_empty_term_are_accepted(model):
    g = good_species(model)
    binding.air_species_check(model, g, **series(model))
    binding.air_species_check(model, None, **series(model))
    binding.air_species_check(model, {}, **series(model))
    binding.air_species_check(model, dict(outdoor_chan=g["outdoor_chan"]), **series(model))
    # a concentration that is not finite is data
    binding.air_species_check(model, changed(changed(g, "conc", 3, np.nan), "conc", 4, np.inf), **series(model))
    # beside loads, paths and handlers, which are checked as their own checks do
    loads = dict(flows=dict(zone=[1], volume_chan=[2], temp_chan=[1]))
    air = dict(target=[1], source=[2], volume_chan=[2])
    handlers = dict(outdoor_chan=[1], br_unit=[0], br_zone=[1], br_volume_chan=[2])
    binding.air_species_check(model, g, loads=loads, air=air, handlers=handlers, **series(model))
    code, msg = _code(lambda: binding.air_species_check(model, g, loads=loads, air=air, handlers=dict(handlers, br_zone=[8]), **series(model)))
    assert code == E_SIZE and "air handler branch 0:" in msg
    code, msg = _code(lambda: binding.air_species_check(model, g, loads=loads, air=dict(air, target=[8]), **series(model)))
    assert code == E_SIZE


def test_counts_and_null_arrays_are_invalid_arguments(model):
    g = good_species(model)
    for field, needle in (("n_species", "air species"), ("n_sources", "species source"), ("n_vents", "demand vent")):
        rc, msg = _raw(model, g, **{field: -1})
        assert rc == E_INVALID_ARG and needle in msg and "negative" in msg, msg
    rc, msg = _raw(model, dict(g, vent_zone=(), vent_species=(), vent_temp_chan=(), vent_enable_chan=None, vent_v_min=(), vent_v_max=(), vent_c_lo=(),
                               vent_c_hi=()), n_species=0)
    assert rc == E_INVALID_ARG and "species source 0" in msg and "n_species 0" in msg, msg
    rc, msg = _raw(model, dict(g, src_zone=(), src_species=(), src_chan=(), src_factor=None), n_species=0)
    assert rc == E_INVALID_ARG and "demand vent 0" in msg and "n_species 0" in msg, msg
    for field in ("outdoor_chan", "conc"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "air species 0" in msg and field in msg, (field, msg)
    for field in ("src_zone", "src_species", "src_chan"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "species source 0" in msg and field in msg, (field, msg)
    for field in ("vent_zone", "vent_species", "vent_temp_chan", "vent_v_min", "vent_v_max", "vent_c_lo", "vent_c_hi"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "demand vent 0" in msg and field in msg, (field, msg)
    for field in ("src_factor", "vent_enable_chan", "limit_chan", "occ_chan") + binding.SPECIES_STATS:   # nullable
        rc, msg = _raw(model, g, **{field: None})
        assert rc == 0, (field, msg)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_values_that_are_not_finite_are_refused(model, bad):
    g = good_species(model)
    code, msg = _code(lambda: binding.air_species_check(model, changed(g, "src_factor", 4, bad), **series(model)))
    assert code == E_INVALID_ARG and "species source 4:" in msg and "src_factor" in msg, msg
    for key in ("vent_v_min", "vent_v_max", "vent_c_lo", "vent_c_hi"):
        code, msg = _code(lambda: binding.air_species_check(model, changed(g, key, 2, bad), **series(model)))
        assert code == E_INVALID_ARG and "demand vent 2:" in msg and key in msg, msg


def test_vents_with_bad_limits_are_refused(model):
    g = good_species(model)
    code, msg = _code(lambda: binding.air_species_check(model, changed(g, "vent_v_min", 0, -1e-300), **series(model)))
    assert code == E_INVALID_ARG and "demand vent 0:" in msg and "vent_v_min" in msg and "negative" in msg, msg
    code, msg = _code(lambda: binding.air_species_check(model, changed(g, "vent_v_max", 2, down(0.02)), **series(model)))
    assert code == E_INVALID_ARG and "demand vent 2:" in msg and "vent_v_max" in msg, msg
    binding.air_species_check(model, changed(g, "vent_v_max", 2, 0.02), **series(model))         # max == min: a constant vent
    for hi in (600.0, down(600.0), -5.0):
        code, msg = _code(lambda: binding.air_species_check(model, changed(g, "vent_c_hi", 2, hi), **series(model)))
        assert code == E_INVALID_ARG and "demand vent 2:" in msg and "vent_c_hi" in msg, msg
    binding.air_species_check(model, changed(g, "vent_c_hi", 2, up(600.0)), **series(model))
    binding.air_species_check(model, changed(g, "src_factor", 1, -7.0), **series(model))         # a sink is the caller's business


def test_zones_species_and_channels_out_of_range_are_size_errors(model):
    Z = int(model["n_zones"])
    g = good_species(model)
    for key, n, what in (("src_zone", Z, "zone"), ("src_species", 2, "species"), ("src_chan", 7, "channel")):
        for bad in (-1, n, n + 12345, -2 ** 31):
            code, msg = _code(lambda: binding.air_species_check(model, changed(g, key, 5, bad), **series(model)))
            assert code == E_SIZE and "species source 5:" in msg and what in msg, msg
    for key, n, what in (("vent_zone", Z, "zone"), ("vent_species", 2, "species"), ("vent_temp_chan", 7, "temperature channel")):
        for bad in (-1, n, 2 ** 31 - 1):
            code, msg = _code(lambda: binding.air_species_check(model, changed(g, key, 3, bad), **series(model)))
            assert code == E_SIZE and "demand vent 3:" in msg and what in msg, msg
    for bad in (-2, 7, -2 ** 31):
        code, msg = _code(lambda: binding.air_species_check(model, changed(g, "vent_enable_chan", 1, bad), **series(model)))
        assert code == E_SIZE and "demand vent 1:" in msg and "enable channel" in msg, msg
        code, msg = _code(lambda: binding.air_species_check(model, changed(g, "outdoor_chan", Z + 2, bad), **series(model)))
        assert code == E_SIZE and "air species 1:" in msg and "outdoor channel" in msg and "zone 2" in msg, msg
        code, msg = _code(lambda: binding.air_species_check(model, changed(g, "limit_chan", 1, bad), **series(model)))
        assert code == E_SIZE and "air species 1:" in msg and "limit channel" in msg, msg
        code, msg = _code(lambda: binding.air_species_check(model, changed(g, "occ_chan", 5, bad), **series(model)))
        assert code == E_SIZE and "air species" in msg and "occupancy channel" in msg and "zone 5" in msg, msg
    # no channels at all: every channel is out of range
    code, msg = _code(lambda: binding.air_species_check(model, g, **series(model, channel=None)))
    assert code == E_SIZE and "air species 0:" in msg, msg


def test_march_without_a_batch_is_an_invalid_argument(model):
    """What heat_batch_march_series_species can answer without a batch, and so without a device. That a bad term is refused
    BEFORE any device work needs a batch: the GPU test test_bad_species_and_sharded_batches_are_refused_by_the_march finds the
    device state untouched behind every refusal."""
    L = binding.load_library()
    s, _ = binding.make_series(**series(model))
    sp, _ = binding.make_air_species(**good_species(model))
    failed = C.c_int32(123)
    call = binding.SeriesCall(size=C.sizeof(binding.SeriesCall), s=C.pointer(s), failed_step=C.pointer(failed))
    assert L.heat_batch_march_series_species(None, C.byref(call), *([None] * 8), C.byref(sp), None, None, None) == E_INVALID_ARG
    assert failed.value == -1
    assert L.heat_batch_march_series_species(*([None] * 14)) == E_INVALID_ARG
    call.size = 8
    assert L.heat_batch_march_series_species(None, C.byref(call), *([None] * 8), C.byref(sp), None, None, None) == E_INVALID_ARG


def test_the_wrapper_reads_the_shapes(model):
    Z = int(model["n_zones"])
    sp, keep = binding.make_air_species(**good_species(model))
    assert sp.n_species == 2 and sp.n_sources == 6 and sp.n_vents == 4 and sp.resume == 0 and sp.step_base == 0
    assert keep["conc"].shape == (2, Z) and keep["n_occupied"].dtype == np.int64 and keep["sum_volume"].shape == (4,) and keep["steps_saturated"].dtype == np.int64
    sp, keep = binding.make_air_species()
    assert sp.n_species == 0 and sp.n_vents == 0 and not sp.outdoor_chan and not sp.conc and not sp.sum_conc
    conc = np.arange(2.0 * Z).reshape(2, Z)
    sp, keep = binding.make_air_species(**dict(good_species(model), conc=conc))
    assert np.array_equal(keep["conc"], conc) and keep["conc"] is not conc
    sp, keep = binding.make_air_species(**dict(good_species(model), stats=("n_above",)))
    assert not sp.sum_conc and not sp.sum_q and sp.n_above and sp.conc and "max_conc" not in keep
    resume = {k: (np.ones((2, Z)) if k not in ("sum_volume", "sum_q", "steps_saturated") else np.ones(4)) for k in binding.SPECIES_STATS}
    sp, keep = binding.make_air_species(**dict(good_species(model), resume=resume, step_base=24))
    assert sp.resume == 1 and sp.step_base == 24 and keep["step_max"].dtype == np.int64 and keep["step_max"].all()
    for bad in (dict(src_zone=np.zeros(5)), dict(vent_v_min=np.zeros(3)), dict(conc=np.zeros((2, Z + 1))), dict(stats=("sum",)),
                dict(limit_chan=np.zeros(3)), dict(occ_chan=np.zeros(Z + 1)), dict(outdoor_chan=np.zeros(Z)), dict(resume=dict(n_above=np.zeros(Z)))):
        with pytest.raises(ValueError):
            binding.make_air_species(**dict(good_species(model), **bad))


# ---- the generator's cases: accepted, and — through the CPU oracle alone — they exercise what they promise ----
COVERAGE_CASES = [("ragged_mixed", 2), ("ragged_mixed", 5), ("rooms_with_windows", 2), ("rooms_with_windows", 5), ("rooms_with_windows_large", 2),
                  ("rooms_with_windows_large", 5)]


@pytest.mark.parametrize("model_name,n_sub", COVERAGE_CASES)
def test_the_generators_cases_are_accepted_and_exercise_paths_vents_and_limits(oracle, model_name, n_sub):
    c = asc.case(model_name, asc.N_STEPS, n_sub, 2, asc.SEED)
    md, sp = c["md"], c["species"]
    kw = dict(weather=c["w"], n_sub=n_sub, channel=c["channel"], probes=c["probes"])
    binding.air_species_check(md, sp, loads=c["loads"], air=c["air"], handlers=c["handlers"], **kw)
    # what the generator promises
    Z, S, V, Q = int(md["n_zones"]), asp.n_species(sp), asp.n_vents(sp), asp.n_sources(sp)
    lanes = S * Z
    assert S == 2 and (lanes < 64 or lanes == 120 or (lanes > 256 and lanes % 64 != 0))
    per_zone = np.bincount(sp["vent_zone"], minlength=Z)
    assert per_zone.max() >= 2 and (per_zone == 0).any() and (per_zone == 1).any()               # zones with several vents
    assert {0, 1} <= set(sp["vent_species"].tolist()) and (sp["vent_enable_chan"] >= 0).any() and (sp["vent_enable_chan"] < 0).any()
    assert not np.array_equal(np.argsort(sp["vent_zone"], kind="stable"), np.arange(V))            # shuffled
    lane = sp["src_species"].astype(np.int64) * Z + sp["src_zone"]
    assert not np.array_equal(np.argsort(lane, kind="stable"), np.arange(Q)) and np.bincount(lane, minlength=lanes).min() >= 2
    assert (sp["src_factor"] < 0).any() and (sp["outdoor_chan"] < 0).any() and len(set(sp["outdoor_chan"][0].tolist())) == 2
    # a zone fed by at least three kinds of inflow
    kinds = np.stack([np.bincount(c["loads"]["flows"]["zone"], minlength=Z) > 0, np.bincount(c["air"]["target"], minlength=Z) > 0,
                      np.bincount(c["handlers"]["br_zone"][(c["handlers"]["br_kind"] & 1) != 0], minlength=Z) > 0, per_zone > 0])
    assert (kinds.sum(axis=0) >= 3).any() and kinds.all(axis=0).any()
    if lanes > 256:                                                                                # paths from another workgroup's lanes
        src, tgt = c["air"]["source"], c["air"]["target"]
        assert ((src >= 0) & (src // 256 != tgt // 256)).any()
    # the oracle loop alone
    big = md["n_surfaces"] > 8192
    m = oracle.OracleModel(md)

    def march(s, wk, za, zb):
        assert m.march(s, wk, za, zb, threads=16 if big else 1)[0] == 0

    out = asc.loop_with_rules(march, c, c["st"].copy())
    asc.assert_coverage(asc.coverage(c, out), "%s n_sub=%d, %d sources, %d vents" % (model_name, n_sub, Q, V))
    for key in ("trace",) + asp.ROWS:
        assert np.all(np.isfinite(out[key])), key
    # the accumulators are the sums of the returned rows
    acc = out["carry"]["species"]
    assert np.array_equal(acc["steps_saturated"], out["saturated"].sum(axis=0))
    for key, rows in (("sum_volume", out["vent_v"]), ("sum_q", out["vent_q"])):
        total = np.zeros(rows.shape[1])
        for r in rows:
            total = total + r
        assert np.array_equal(acc[key], total), key
    occ = sp["occ_chan"]
    occupied = (occ[None, :] < 0) | (c["channel"][:, np.maximum(occ, 0)] > 0)
    assert np.array_equal(acc["n_occupied"], np.broadcast_to(occupied.sum(axis=0), (S, Z)))
    rows = np.where(occupied[:, None, :], out["conc_rows"], -np.inf)
    assert np.array_equal(acc["max_conc"], rows.max(axis=0)) and np.array_equal(acc["step_max"], rows.argmax(axis=0))
    limit = c["channel"][:, sp["limit_chan"][0]][:, None]
    assert np.array_equal(acc["n_above"][0], (occupied & (out["conc_rows"][:, 0, :] > limit)).sum(axis=0)) and not acc["n_above"][1].any()
    assert (acc["conc"] != sp["conc"]).all() and np.array_equal(out["conc_rows"][0], sp["conc"])


def test_air_species_check_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "air_species_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "air species host check: all statuses as the header states them" in out.stdout
