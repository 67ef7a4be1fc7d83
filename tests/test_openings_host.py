"""Openings of a series on the host (include/heat_amd.h, heat_openings / heat_openings_check / heat_batch_march_series_openings;
heat_amd/openings.py): the entry points are declared, exported and bound; the ctypes mirror has the header's layout and the
structs beside it keep theirs; the rule in numpy (openings.apply — the reference of tests/test_openings_gpu.py) gives the
hand-worked single-opening cases at, one ulp below and one ulp above both ends of the open fraction, at y = 0, with a and b
swapped and with a NaN temperature; each convenience reproduces its published formula at one worked point; every refusal the
header lists comes back with its code and names the opening, before any device work; the generator's cases are accepted and — run
through the CPU oracle alone — their flows respond, their controlled paths open and close and no controller decision of the cases
used against the oracle on the GPU comes within 1e-6 K of its threshold. heat_openings_check — with the table builder and its
verification — also runs under AddressSanitizer / UBSan as a stand-alone program (tests/openings_host_main.cpp) in a child
process. No GPU needed.

Reference: the rule is this project's own (the reference has no counterpart: model.rs:546,592-593 take the volumes as given)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import heat_amd
from heat_amd import binding, modeldict as mdl, openings as opn
import helpers
import openings_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_openings_check", "heat_batch_march_series_openings")
E_INVALID_ARG, E_SIZE = -1, -4
FIELDS = ("n_openings", "zone_a", "zone_b", "temp_chan", "wind_chan", "frac_chan", "out_chan", "area", "cw", "cs", "ca", "c0", "resume",
          "step_base", "sum_v", "max_v", "step_max")
OUT_OF_SCOPE = ("a pressure network or mass balance across several openings",
                "two-way flow with a neutral plane resolved over the opening height", "wind pressure coefficients from direction",
                "density of moist air", "the opening's own effect on convection coefficients")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_openings {" in header
    assert "heat_openings_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_openings" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("Openings", "make_openings", "openings_check"))
    assert all(hasattr(heat_amd, n) for n in ("Openings", "make_openings", "openings_check", "openings"))
    assert all(hasattr(opn, n) for n in ("apply", "accumulate", "fresh", "concat", "wind_and_stack", "single_sided", "doorway"))
    flat = " ".join(header.replace("*", " ").split())
    for words in OUT_OF_SCOPE:
        assert words in flat, words                                     # what is out of scope is stated
    assert "model.rs:546,592-593" in header
    assert L.heat_amd_abi_version() == 1
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW) and "pub struct HeatOpenings" in rust


def test_openings_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = (["sizeof(heat_openings)", "sizeof(heat_air_paths)", "sizeof(heat_series_call)", "sizeof(heat_air_species)", "sizeof(heat_series)",
             "sizeof(heat_zone_loads)", "sizeof(heat_air_handlers)"] + ["offsetof(heat_openings, %s)" % f for f in FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == ([C.sizeof(binding.Openings), C.sizeof(binding.AirPaths), C.sizeof(binding.SeriesCall), C.sizeof(binding.AirSpecies),
                    C.sizeof(binding.Series), C.sizeof(binding.ZoneLoads), C.sizeof(binding.AirHandlers)] +
                   [getattr(binding.Openings, f).offset for f in FIELDS])
    assert [f for f, _ in binding.Openings._fields_] == list(FIELDS)
    # every field is 8 bytes wide
    assert got[0] == 8 * len(FIELDS) and got[7:] == [8 * i for i in range(len(FIELDS))]
    # the structs beside it are as they were: the openings are no field of any of them
    assert got[1] == 8 * 14 and got[2] == 8 * 24 and got[3] == 8 * 30


# ---- the rule in numpy: hand-worked single-opening cases ----
# two zones; channel 0 the outside temperature, 1 the wind speed, 2 the open fraction, 3 the derived channel, 4 a bystander
TA, TB, TOUT, WIND = 24.0, 19.5, 7.25, 3.5
AREA, CW, CS, CA, C0 = 0.75, 0.0625, 9.5, 0.004, 0.01


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def one(frac=0.5, T=(TA, TB), **more):
    op = dict(dict(zone_a=[0], zone_b=[-1], temp_chan=[0], wind_chan=[1], frac_chan=[2], out_chan=[3], area=[AREA], cw=[CW], cs=[CS], ca=[CA],
                   c0=[C0]), **more)
    row = np.array([TOUT, WIND, frac, -77.0, 5.5])
    out, V = opn.apply(np.array(T), row, op)
    assert row.tolist()[:2] + row.tolist()[3:] == [TOUT, WIND, -77.0, 5.5]            # the caller's row is not written
    assert np.array_equal(out[3], V[0], equal_nan=True) and np.array_equal(np.delete(out, 3), np.delete(row, 3), equal_nan=True)
    return float(V[0])


def by_hand(ta, tb, u, f, area=AREA, cw=CW, cs=CS, ca=CA, c0=C0):
    d = ta - tb
    ad = abs(d)
    tk = (ta + tb) * 0.5 + 273.15
    y = ((cw * (u * u) + cs * (ad / tk)) + ca * ad) + c0
    return (area * f) * float(np.sqrt(y))


def test_an_opening_to_outside_follows_the_rule_line_by_line():
    assert one() == by_hand(TA, TOUT, WIND, 0.5) > 0.0
    # between zones: no channel is read for the other side's temperature
    assert one(zone_b=[1], temp_chan=[-1]) == by_hand(TA, TB, WIND, 0.5) != one()
    # no wind channel: u = 0; no open-fraction channel: fully open; absent coefficients are 0
    assert one(wind_chan=[-1]) == by_hand(TA, TOUT, 0.0, 0.5) and one(wind_chan=None) == one(wind_chan=[-1])
    assert one(frac_chan=[-1]) == by_hand(TA, TOUT, WIND, 1.0) and one(frac_chan=None) == one(frac_chan=[-1])
    assert one(cs=None, ca=None) == by_hand(TA, TOUT, WIND, 0.5, cs=0.0, ca=0.0)
    # the order of the sum under the root: ((w + st) + sa) + c0 — terms fifteen orders of magnitude apart tell the orders apart
    big = dict(cw=[1e15 / (WIND * WIND)], cs=[1.0], ca=[3.0], c0=[0.03])
    w, st, sa = big["cw"][0] * (WIND * WIND), 1.0 * (abs(TA - TOUT) / ((TA + TOUT) * 0.5 + 273.15)), 3.0 * abs(TA - TOUT)
    assert one(frac=1.0, **big) == AREA * float(np.sqrt(((w + st) + sa) + 0.03))
    assert ((w + st) + sa) + 0.03 != w + ((st + sa) + 0.03)


def test_the_open_fraction_is_clamped_at_and_one_ulp_either_side_of_zero_and_one():
    full = by_hand(TA, TOUT, WIND, 1.0)
    tiny = up(0.0)                                                          # the smallest subnormal: one ulp above 0
    for f, want in ((0.0, 0.0), (down(0.0), 0.0), (-3.0, 0.0), (tiny, by_hand(TA, TOUT, WIND, tiny)),
                    (1.0, full), (up(1.0), full), (7.0, full), (down(1.0), by_hand(TA, TOUT, WIND, down(1.0)))):
        assert one(frac=f) == want, f
    assert one(frac=down(1.0)) < full and one(frac=-0.0) == 0.0
    assert one(frac=1e-3) == by_hand(TA, TOUT, WIND, 1e-3) > 0.0
    # a NaN fraction makes both comparisons false: it stays, and V is NaN
    assert np.isnan(one(frac=np.nan))


def test_y_at_zero_with_every_coefficient_zero_gives_exactly_zero():
    zero = dict(cw=[0.0], cs=[0.0], ca=[0.0], c0=[0.0])
    v = one(frac=1.0, **zero)
    assert v == 0.0 and not np.signbit(v)
    assert one(frac=1.0, cw=None, cs=None, ca=None, c0=None) == 0.0
    # no temperature difference and no wind: only c0 is left, and with c0 = 0 nothing
    assert one(frac=1.0, T=(TOUT, TB), wind_chan=[-1], c0=[0.0]) == 0.0
    assert one(frac=1.0, T=(TOUT, TB), wind_chan=[-1]) == AREA * float(np.sqrt(C0))
    # an area of zero
    assert one(area=[0.0]) == 0.0


def test_swapping_a_and_b_gives_the_same_bits():
    rng = np.random.default_rng(5)
    T = rng.uniform(-20.0, 45.0, 40)
    a, b = rng.integers(0, 40, 300), rng.integers(0, 40, 300)
    keep = a != b
    a, b = a[keep], b[keep]
    n = len(a)
    op = dict(zone_a=a, zone_b=b, out_chan=np.arange(n), area=rng.uniform(0.0, 2.0, n), cs=rng.uniform(0.0, 30.0, n), ca=rng.uniform(0.0, 0.01, n),
              c0=rng.uniform(0.0, 0.02, n))
    row = np.zeros(n)
    v1 = opn.apply(T, row, op)[1]
    v2 = opn.apply(T, row, dict(op, zone_a=b, zone_b=a))[1]
    assert np.array_equal(v1, v2) and (v1 > 0.0).all() and len(set(v1.tolist())) > n // 2


def test_a_nan_temperature_gives_a_nan_flow_and_nothing_else_changes():
    op = dict(zone_a=[0, 1, 2], zone_b=[1, 2, -1], temp_chan=[-1, -1, 0], out_chan=[3, 5, 6], area=[1.0, 1.0, 1.0], cs=[9.0, 9.0, 9.0], c0=[0.01] * 3)
    row = np.array([TOUT, WIND, 0.5, -1.0, 5.5, -1.0, -1.0])
    good, vg = opn.apply(np.array([20.0, 22.0, 25.0]), row, op)
    out, v = opn.apply(np.array([np.nan, 22.0, 25.0]), row, op)
    assert np.isnan(v[0]) and np.isnan(out[3]) and np.array_equal(v[1:], vg[1:]) and np.array_equal(np.delete(out, 3), np.delete(good, 3))
    # the accumulators: a NaN V is no maximum; its sum is NaN and the others' are not
    acc = opn.fresh(op)
    opn.accumulate(v, acc, 4)
    opn.accumulate(vg, acc, 5)
    assert np.isnan(acc["sum_v"][0]) and np.array_equal(acc["sum_v"][1:], (0.0 + vg[1:]) + vg[1:])
    assert acc["max_v"][0] == vg[0] and acc["step_max"].tolist() == [5, 4, 4]    # a maximum keeps its first step
    # a NaN outside temperature reaches the openings that read it and no other
    row[0] = np.nan
    out, v = opn.apply(np.array([20.0, 22.0, 25.0]), row, op)
    assert np.isnan(v[2]) and np.array_equal(v[:2], vg[:2])


def test_fresh_accumulate_and_concat():
    op = opn.concat(dict(zone_a=[0], zone_b=[-1], temp_chan=[0], area=[1.0], cw=[0.5]), dict(zone_a=[1, 2], zone_b=[2, 0], area=[0.5, 0.25], cs=[3.0, 4.0]))
    assert op["zone_a"].tolist() == [0, 1, 2] and op["temp_chan"].tolist() == [0, -1, -1] and op["wind_chan"].tolist() == [-1] * 3
    assert op["cw"].tolist() == [0.5, 0.0, 0.0] and op["cs"].tolist() == [0.0, 3.0, 4.0] and op["c0"].tolist() == [0.0] * 3
    assert "out_chan" not in op and op["zone_a"].dtype == np.int32 and opn.n_openings(op) == 3 and opn.n_openings({}) == 0
    acc = opn.fresh(op)
    assert acc["sum_v"].tolist() == [0.0] * 3 and (acc["max_v"] == -np.inf).all() and acc["step_max"].tolist() == [-1] * 3
    opn.accumulate(np.array([0.0, 2.0, 1.0]), acc, 10)
    opn.accumulate(np.array([0.0, 1.0, up(1.0)]), acc, 11)
    assert acc["sum_v"].tolist() == [0.0, 3.0, 1.0 + up(1.0)] and acc["max_v"].tolist() == [0.0, 2.0, up(1.0)] and acc["step_max"].tolist() == [10, 10, 11]
    out, v = opn.apply(np.zeros(3), np.zeros(2), {})
    assert out.tolist() == [0.0, 0.0] and v.shape == (0,)


def test_each_convenience_reproduces_its_published_formula_at_a_worked_point():
    g = 9.81
    # EnergyPlus, wind and stack with open area: Qw = Cw A F u, Qs = Cd A F sqrt(2 g dH |Tz - To| / T), Q = sqrt(Qw^2 + Qs^2)
    A, cd, cwo, dh, F, u, tz, to = 1.2, 0.6, 0.55, 0.9, 0.8, 2.5, 26.0, 14.0
    t = (tz + to) * 0.5 + 273.15
    qw, qs = cwo * A * F * u, cd * A * F * np.sqrt(2.0 * g * dh * abs(tz - to) / t)
    k = opn.wind_and_stack(A, cd, cwo, dh)
    assert set(k) == {"area", "cw", "cs"} and k["cw"] == cwo * cwo and k["cs"] == cd * cd * 2.0 * g * dh and k["area"] == A
    v = opn.apply(np.array([tz]), np.array([to, u, F, 0.0]), dict(zone_a=[0], zone_b=[-1], temp_chan=[0], wind_chan=[1], frac_chan=[2], out_chan=[3], **k))[1][0]
    assert v == pytest.approx(np.sqrt(qw * qw + qs * qs), rel=1e-14)
    # de Gids and Phaff: Q = A / 2 sqrt(0.001 u^2 + 0.0035 H |dT| + 0.01)
    H = 1.3
    k = opn.single_sided(A, H)
    assert set(k) == {"area", "cw", "ca", "c0"} and k["area"] == A / 2.0 and k["cw"] == 0.001 and k["ca"] == 0.0035 * H and k["c0"] == 0.01
    v = opn.apply(np.array([tz]), np.array([to, u, 1.0, 0.0]), dict(zone_a=[0], zone_b=[-1], temp_chan=[0], wind_chan=[1], out_chan=[3], **k))[1][0]
    assert v == pytest.approx(A / 2.0 * np.sqrt(0.001 * u * u + 0.0035 * H * abs(tz - to) + 0.01), rel=1e-14)
    assert 0.05 < v < 0.2                                                # (1.2 m2, 2.5 m/s, 12 K: about 0.15 m3/s)
    # Brown and Solvason: Q = Cd W H / 3 sqrt(g H |dT| / T)
    W, Hd, cdd, t1, t2 = 0.9, 2.05, 0.65, 23.0, 20.5
    k = opn.doorway(W, Hd, cdd)
    assert set(k) == {"area", "cs"} and k["area"] == cdd * W * Hd / 3.0 and k["cs"] == g * Hd
    v = opn.apply(np.array([t1, t2]), np.zeros(1), dict(zone_a=[0], zone_b=[1], out_chan=[0], **k))[1][0]
    assert v == pytest.approx(cdd * W * Hd / 3.0 * np.sqrt(g * Hd * abs(t1 - t2) / ((t1 + t2) * 0.5 + 273.15)), rel=1e-14)
    assert 0.1 < v < 0.25                                                # (a door, 2.5 K: about 0.17 m3/s each way)
    # arrays broadcast
    k = opn.doorway([0.8, 0.9], 2.0, 0.6)
    assert k["area"].shape == (2,) and k["cs"].shape == (2,)


# ---- refusals ----
@pytest.fixture(scope="module")
def model():
    return mdl.clustered_massive(200, Z=8, seed=3)[0]


N_CHANNELS = 12


def series(**more):
    return dict(dict(weather=np.zeros((2, 1, 3)), n_sub=1, channel=np.zeros((2, N_CHANNELS))), **more)


def good_openings():
    """Five openings in 8 zones: three to outside, two between zones; channels 0-1 outside temperatures, 2 wind, 3 open fraction,
    4-8 derived."""
    return dict(zone_a=[0, 3, 7, 2, 5], zone_b=[-1, -1, 4, -1, 6], temp_chan=[0, 1, -1, 0, -1], wind_chan=[2, -1, -1, 2, 2], frac_chan=[3, 3, -1, -1, 3],
                out_chan=[6, 4, 8, 5, 7], area=[0.5, 0.0, 1.0, 0.25, 2.0], cw=[0.3, 0.0, 0.0, 0.001, 0.1], cs=[5.0, 4.0, 20.0, 0.0, 0.0],
                ca=[0.0, 0.0, 0.0, 0.004, 0.0], c0=[0.0, 0.01, 0.0, 0.01, 0.02])


def changed(g, key, i, value):
    a = np.array(g[key], dtype=np.float64 if isinstance(value, float) else None)
    a[i] = value
    return dict(g, **{key: a})


def _code(call):
    with pytest.raises(binding.HeatError) as e:
        call()
    return e.value.code, str(e.value)


def _raw(model, g, **fields):
    """heat_openings_check with fields of the struct overwritten (a count, or None for a NULL array)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(model)
    s, skeep = binding.make_series(**series())
    op, okeep = binding.make_openings(**g)
    for k, v in fields.items():
        setattr(op, k, v)
    rc = L.heat_openings_check(C.byref(desc), C.byref(s), C.byref(op))
    return rc, L.heat_last_error().decode("utf-8", "replace")


def test_a_good_term_no_term_and_an_empty_term_are_accepted(model):
    g = good_openings()
    binding.openings_check(model, g, **series())
    binding.openings_check(model, None, **series())
    binding.openings_check(model, {}, **series())
    binding.openings_check(model, {k: v for k, v in g.items() if k not in ("wind_chan", "frac_chan", "cw", "cs", "ca", "c0")}, **series())
    binding.openings_check(model, dict(g, stats=()), **series())
    inner = dict(zone_a=[0, 1], zone_b=[1, 2], out_chan=[4, 5], area=[1.0, 1.0])       # no opening to outside: no temp_chan at all
    binding.openings_check(model, inner, **series())
    with pytest.raises(ValueError):
        binding.make_openings(**dict(g, stats=("sum_q",)))
    with pytest.raises(ValueError):
        binding.make_openings(**dict(g, area=[1.0]))


def test_counts_and_null_arrays_are_invalid_arguments(model):
    g = good_openings()
    rc, msg = _raw(model, g, n_openings=-1)
    assert rc == E_INVALID_ARG and "opening" in msg and "negative" in msg, msg
    for field in ("zone_a", "zone_b", "out_chan", "area"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "opening 0:" in msg and field in msg, (field, msg)
    for field in ("wind_chan", "frac_chan", "cw", "cs", "ca", "c0") + binding.OPENING_STATS:   # nullable
        rc, msg = _raw(model, g, **{field: None})
        assert rc == 0, (field, msg)
    rc, msg = _raw(model, g, n_openings=0, zone_a=None, zone_b=None, out_chan=None, area=None)
    assert rc == 0, msg
    # temp_chan is nullable only when no opening leads outside
    rc, msg = _raw(model, g, temp_chan=None)
    assert rc == E_SIZE and "opening 0:" in msg and "temp_chan is NULL" in msg, msg


@pytest.mark.parametrize("key", ["area", "cw", "cs", "ca", "c0"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, -1e-9])
def test_an_area_or_coefficient_that_is_negative_or_not_finite_is_refused(model, key, bad):
    code, msg = _code(lambda: binding.openings_check(model, changed(good_openings(), key, 3, bad), **series()))
    assert code == E_INVALID_ARG and "opening 3:" in msg and key in msg, msg


def test_every_other_refusal_names_its_opening(model):
    g = good_openings()
    for bad, code, needle in ((changed(g, "zone_b", 2, 7), E_INVALID_ARG, "opening 2:"),              # zone_a == zone_b
                              (changed(g, "zone_a", 1, 8), E_SIZE, "opening 1:"),
                              (changed(g, "zone_a", 1, -1), E_SIZE, "opening 1:"),
                              (changed(g, "zone_b", 4, 8), E_SIZE, "opening 4:"),
                              (changed(g, "zone_b", 4, -2), E_SIZE, "opening 4:"),
                              (changed(g, "out_chan", 3, N_CHANNELS), E_SIZE, "opening 3:"),
                              (changed(g, "out_chan", 3, -1), E_SIZE, "opening 3:"),
                              (changed(g, "temp_chan", 0, N_CHANNELS), E_SIZE, "opening 0:"),
                              (changed(g, "temp_chan", 3, -1), E_SIZE, "opening 3:"),                 # outside without a temperature
                              (changed(g, "temp_chan", 2, 0), E_SIZE, "opening 2:"),                  # zone to zone with one
                              (changed(g, "wind_chan", 4, N_CHANNELS), E_SIZE, "opening 4:"),
                              (changed(g, "wind_chan", 4, -2), E_SIZE, "opening 4:"),
                              (changed(g, "frac_chan", 1, N_CHANNELS), E_SIZE, "opening 1:"),
                              (changed(g, "frac_chan", 1, -2), E_SIZE, "opening 1:"),
                              (changed(g, "out_chan", 4, 6), E_SIZE, "opening 4:"),                   # opening 0 writes channel 6 too
                              (changed(g, "temp_chan", 1, 8), E_SIZE, "opening 1:"),                  # opening 2's derived channel
                              (changed(g, "wind_chan", 0, 5), E_SIZE, "opening 0:"),                  # opening 3's
                              (changed(g, "frac_chan", 4, 7), E_SIZE, "opening 4:")):                 # its own
        got, msg = _code(lambda: binding.openings_check(model, bad, **series()))
        assert got == code and needle in msg, (msg, needle)
    # a series without channels; a NULL series is the binding's to refuse
    got, msg = _code(lambda: binding.openings_check(model, g, **series(channel=np.zeros((2, 0)))))
    assert got == E_SIZE and "opening 0:" in msg


# ---- the generator's cases: accepted, and — through the CPU oracle alone — they exercise what they promise ----
COVERAGE_CASES = oc.ORACLE_CASES + [("rooms_with_windows", 5)]


@pytest.mark.parametrize("floor", [True, False], ids=["c0_floor", "c0_zero"])
@pytest.mark.parametrize("model_name,n_sub", COVERAGE_CASES)
def test_the_generators_cases_are_accepted_respond_and_keep_their_margin(oracle, model_name, n_sub, floor):
    c = oc.case(model_name, oc.N_STEPS, n_sub, 2, oc.SEED, floor=floor)
    md, op, info = c["md"], c["openings"], c["openings_info"]
    kw = dict(weather=c["w"], n_sub=n_sub, channel=c["channel"], probes=c["probes"])
    binding.openings_check(md, op, **kw)
    binding.air_species_check(md, c["species"], loads=c["loads"], air=c["air"], handlers=c["handlers"], **kw)
    # what the generator promises: every opening feeds a consumer, every kind of consumer reads a derived channel
    Z, n = int(md["n_zones"]), opn.n_openings(op)
    assert n == Z + Z // 2 and sorted(op["out_chan"].tolist()) == info["derived"].tolist() and np.isnan(c["channel"][:, info["derived"]]).all()
    assert not np.array_equal(np.argsort(op["zone_a"], kind="stable"), np.arange(n))                  # shuffled
    air, flows = c["air"], c["loads"]["flows"]
    derived = set(info["derived"].tolist())
    assert set(air["volume_chan"][info["vents"]].tolist()) | set(air["volume_chan"][info["pairs"]].tolist()) == derived
    assert (air["open_chan"][info["vents"]] >= 0).all() and (air["open_chan"][info["pairs"]] < 0).all()
    assert len(derived & set(flows["volume_chan"].tolist())) == (Z + 1) // 2
    pair_chan = air["volume_chan"][info["pairs"]]
    assert np.array_equal(pair_chan[:Z // 2], pair_chan[Z // 2:])                                      # a doorway is ONE opening
    assert (op["zone_b"] < 0).sum() == Z and (op["wind_chan"] < 0).any() and (op["frac_chan"] < 0).any() and (op["frac_chan"] >= 0).any()
    assert ((op["c0"] >= 0.01).all() and floor) or ((op["c0"] == 0.0).sum() >= n // 3 and not floor)
    # the oracle loop alone
    m = oracle.OracleModel(md)

    def march(s, wk, za, zb):
        assert m.march(s, wk, za, zb, threads=1)[0] == 0

    out = oc.loop_with_rules(march, c, c["st"].copy())
    oc.assert_coverage(oc.coverage(c, out), "%s n_sub=%d, %d openings" % (model_name, n_sub, n))
    for key in ("trace", "opening_v", "path_q", "conc_rows"):
        assert np.all(np.isfinite(out[key])), key
    assert (out["opening_v"] >= 0.0).all() and np.isfinite(out["rows"][:, info["derived"]]).all()
    # the doorways respond to the temperatures alone (the odd ones have no open-fraction channel, and no door has wind)
    doors = info["doors"][op["frac_chan"][info["doors"]] < 0]
    assert len(doors) and (out["opening_v"][:, doors].max(axis=0) > out["opening_v"][:, doors].min(axis=0)).all()
    # what moved is what the paths let through: a closed window carries nothing, whatever its opening would
    states = out["states"][:, info["vents"]]
    assert (out["path_q"][:, info["vents"]][states == 0] == 0.0).all() and (out["opening_v"] > 0.0).mean() > 0.5
    # the accumulators are the sums of the returned rows
    acc = out["carry"]["openings"]
    total = np.zeros(n)
    for r in out["opening_v"]:
        total = total + r
    assert np.array_equal(acc["sum_v"], total) and np.array_equal(acc["max_v"], out["opening_v"].max(axis=0))
    assert np.array_equal(acc["step_max"], out["opening_v"].argmax(axis=0))
    # the margin condition of the cases used against the oracle on the GPU
    gap = oc.margin(c, out)
    print("%s n_sub=%d %s: least distance of a controller decision from its threshold %.3e K" % (model_name, n_sub, "floor" if floor else "zero", gap))
    if floor and (model_name, n_sub) in oc.ORACLE_CASES:
        assert gap >= oc.MARGIN, gap


def test_a_cut_loop_equals_the_loop_in_one(oracle):
    c = oc.case("ragged_mixed", oc.N_STEPS, 2, 2, oc.SEED)
    m = oracle.OracleModel(c["md"])

    def march(s, wk, za, zb):
        assert m.march(s, wk, za, zb, threads=1)[0] == 0

    s1 = c["st"].copy()
    one_ = oc.loop_with_rules(march, c, s1)
    s2 = c["st"].copy()
    first = oc.loop_with_rules(march, c, s2, steps=slice(0, 9))
    second = oc.loop_with_rules(march, c, s2, steps=slice(9, None), carry=first["carry"], step_base=0)
    assert np.array_equal(s1, s2) and np.array_equal(one_["opening_v"], np.concatenate([first["opening_v"], second["opening_v"]]))
    for key in opn.ACC:
        assert np.array_equal(one_["carry"]["openings"][key], second["carry"]["openings"][key]), key
    assert (one_["carry"]["openings"]["step_max"] >= 9).any() and (one_["carry"]["openings"]["step_max"] < 9).any()


def test_openings_check_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "openings_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "openings host check: all statuses as the header states them" in out.stdout
