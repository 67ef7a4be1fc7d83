"""Air handlers of a series on the host (include/heat_amd.h, heat_air_handlers / heat_air_handlers_check /
heat_batch_march_series_handlers; heat_amd/air_handlers.py): the entry points are declared, exported and bound; the ctypes mirror
has the header's layout; the rule in numpy (air_handlers.apply — the reference of tests/test_air_handlers_gpu.py) gives the
hand-worked single-unit cases at, one ulp below and one ulp above every threshold; every refusal the header lists comes back with
its code and names the unit or the branch, before any device work; the generator's cases are accepted and — run through the CPU
oracle alone — exercise the bypass and both coils. heat_air_handlers_check — with the table builder and its verification — also
runs under AddressSanitizer / UBSan as a stand-alone program (tests/air_handlers_host_main.cpp) in a child process. No GPU needed.

Reference: the rule is this project's own (the reference has no plant: heating_cooling.rs is a todo!(), model.rs:522-544 knows
scheduled flows only); the air properties are the reference's (gas.rs:49,165-179)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import heat_amd
from heat_amd import air_handlers as ah, binding, modeldict as mdl
import air_handlers_cases as ahc
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_air_handlers_check", "heat_batch_march_series_handlers")
E_INVALID_ARG, E_SIZE = -1, -4
N_STEPS = 4
FIELDS = ("n_units", "outdoor_chan", "eff_chan", "eff_gain", "bypass_chan", "bypass_band", "bypass_min_delta", "heat_chan", "cool_chan",
          "heat_cap", "cool_cap", "n_branches", "br_unit", "br_zone", "br_volume_chan", "br_volume_gain", "br_kind", "bypass",
          "sum_recovered", "sum_heating", "sum_cooling", "steps_bypass", "switches", "steps_heat_saturated", "steps_cool_saturated",
          "sum_branch_q")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_air_handlers {" in header
    assert "heat_air_handlers_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_handlers" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("AirHandlers", "make_air_handlers", "air_handlers_check"))
    assert all(hasattr(heat_amd, n) for n in ("AirHandlers", "make_air_handlers", "air_handlers_check", "air_handlers"))
    assert all(hasattr(ah, n) for n in ("apply", "accumulate", "concat", "balanced"))
    for word in ("frost protection", "fan heat", "latent recovery", "variable-volume", "follows the coil outlet"):
        assert word in header, word                                     # what is out of scope is stated
    assert L.heat_amd_abi_version() == 1
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW)


def test_air_handlers_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = (["sizeof(heat_air_handlers)", "sizeof(heat_air_paths)", "sizeof(heat_comfort)", "sizeof(heat_series_call)", "sizeof(heat_series)",
             "sizeof(heat_zone_loads)"] + ["offsetof(heat_air_handlers, %s)" % f for f in FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    # (the structs beside it keep their sizes: the air handlers are a struct of their own, heat_series_call is as it was)
    assert got == ([C.sizeof(binding.AirHandlers), C.sizeof(binding.AirPaths), C.sizeof(binding.Comfort), C.sizeof(binding.SeriesCall),
                    C.sizeof(binding.Series), C.sizeof(binding.ZoneLoads)] + [getattr(binding.AirHandlers, f).offset for f in FIELDS])
    assert [f for f, _ in binding.AirHandlers._fields_] == list(FIELDS)
    assert got[0] == 8 * len(FIELDS) and got[1] == 8 * 14 and got[3] == 8 * 24


# ---- the rule in numpy: hand-worked single-unit cases ----
# channel 0 the volume (a power of two: V * T / V is T exactly), 1 the outdoor air, 2 the bypass setpoint, 3 / 4 the minimum /
# maximum supply temperature, 5 the effectiveness
VOLUME, TO, SET = 0.03125, 10.0, 24.0


def props(tr):
    tk = tr + 273.15
    return 101325. * 28.97 / (8314.46261815324 * tk), 1002.7370 + 1.2324e-2 * tk


def flow(tr, v=VOLUME):
    rho, cp = props(tr)
    return (rho * v) * cp


def unit(**more):
    """One unit that extracts from zone 0 and supplies zone 1."""
    return dict(dict(outdoor_chan=np.array([1]), br_unit=np.array([0, 0]), br_zone=np.array([0, 1]), br_volume_chan=np.array([0, 0]),
                     br_kind=np.array([2, 1])), **{k: np.array([v]) for k, v in more.items()})


def step(h, te, state=0, to=TO, setpoint=SET, t_min=-100.0, t_max=100.0, eta=1.0, t1=20.0):
    bypass = np.array([state], np.uint8)
    row = np.array([VOLUME, to, setpoint, t_min, t_max, eta])
    a0, b0, rows = ah.apply(np.array([te, t1]), row, np.array([7.0, 3.0]), np.array([2.0, 1.0]), h, bypass)
    return int(bypass[0]), a0, b0, rows


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def test_a_recovering_unit_supplies_between_outdoor_and_extract_air():
    h = unit(eff_gain=0.75)
    state, a0, b0, rows = step(h, 22.0)
    te = (VOLUME * 22.0) / VOLUME                                       # one extract branch: st / sv
    r = 0.75 * (te - TO)
    tr = TO + r
    m = flow(tr)
    assert 30.0 < m < 40.0                                              # 1/32 m3/s of air: about 38 W/K
    assert rows["extract_t"][0] == te and rows["supply_t"][0] == tr == 19.0 and rows["recovered"][0] == m * r and rows["coil_q"][0] == 0.0
    assert a0[1] == 3.0 + m * tr and b0[1] == 1.0 + m and a0[0] == 7.0 and b0[0] == 2.0          # only inflows appear in the balance
    assert rows["branch_q"][1] == m * (tr - 20.0) and rows["branch_q"][0] == 0.0                # the extract branch: 0.0
    assert state == 0 and not rows["heat_active"][0] and not rows["cool_active"][0]
    # no terms given: zeros; nullable gains and kinds: 1 and 3
    a0, b0, rows = ah.apply(np.array([22.0, 20.0]), np.array([VOLUME, TO]), None, None,
                            dict(outdoor_chan=[1], br_unit=[0, 0], br_zone=[0, 1], br_volume_chan=[0, 0]), np.zeros(1, np.uint8))
    te = (VOLUME * 22.0 + VOLUME * 20.0) / (VOLUME + VOLUME)
    tr = TO + 1.0 * (te - TO)
    assert rows["extract_t"][0] == te and a0[0] == flow(tr) * tr and b0[1] == flow(tr)
    # eta clamped at 0 and at 1; the channel multiplies the gain
    for gain, eta, want in ((-0.5, 1.0, 0.0), (2.0, 0.25, 0.5), (2.0, 0.75, 1.0), (0.5, -1.0, 0.0), (1.0, up(1.0), 1.0), (1.0, down(1.0), down(1.0))):
        rows = step(unit(eff_gain=gain, eff_chan=5), 22.0, eta=eta)[3]
        assert rows["supply_t"][0] == TO + want * (22.0 - TO), (gain, eta)
    # sv == 0: nothing to recover from, Te = To; the supply is outdoor air
    for h in (dict(unit(eff_gain=0.75), br_kind=np.array([1, 1])), dict(unit(eff_gain=0.75), br_volume_gain=np.array([0.0, 1.0]))):
        rows = step(h, 22.0)[3]
        assert rows["extract_t"][0] == TO and rows["supply_t"][0] == TO and rows["recovered"][0] == 0.0


def test_the_callers_order_in_st_m_and_a_zones_sum():
    gains = np.array([1e-3, 1.0, 3e3])
    h = dict(outdoor_chan=[1], eff_gain=[0.5], br_unit=[0, 0, 0], br_zone=[0, 1, 2], br_volume_chan=[0, 0, 0], br_volume_gain=gains, br_kind=[3, 3, 3])
    T = np.array([21.3, 24.7, 18.9])
    a0, b0, rows = ah.apply(T, np.array([VOLUME, TO]), None, None, h, np.zeros(1, np.uint8))
    v = gains * VOLUME
    st = ((0.0 + v[0] * T[0]) + v[1] * T[1]) + v[2] * T[2]
    sv = ((0.0 + v[0]) + v[1]) + v[2]
    te = st / sv
    tr = TO + 0.5 * (te - TO)
    m = [flow(tr, x) for x in v]
    M = ((0.0 + m[0]) + m[1]) + m[2]
    assert rows["extract_t"][0] == te and rows["recovered"][0] == M * (0.5 * (te - TO))
    backwards = dict(h, br_zone=[2, 1, 0], br_volume_gain=gains[::-1])
    other = ah.apply(T, np.array([VOLUME, TO]), None, None, backwards, np.zeros(1, np.uint8))[2]
    assert other["extract_t"][0] == (((0.0 + v[2] * T[2]) + v[1] * T[1]) + v[0] * T[0]) / (((0.0 + v[2]) + v[1]) + v[0])
    # a zone supplied by three units, in the caller's order: ((a + x0) + x1) + x2
    three = dict(outdoor_chan=[1, 1, 1], eff_gain=[0.0, 0.5, 1.0], br_unit=[2, 0, 1, 0, 1, 2], br_zone=[1, 1, 1, 0, 0, 0], br_volume_chan=[0] * 6,
                 br_volume_gain=[3e3, 1e-3, 1.0, 1.0, 1.0, 1.0], br_kind=[1, 1, 1, 2, 2, 2])
    a0, b0, rows = ah.apply(np.array([22.0, 20.0]), np.array([VOLUME, TO]), np.array([0.0, 0.1]), np.array([0.0, 0.1]), three, np.zeros(3, np.uint8))
    ts = [TO + e * (22.0 - TO) for e in (0.0, 0.5, 1.0)]
    m = [flow(ts[2], 3e3 * VOLUME), flow(ts[0], 1e-3 * VOLUME), flow(ts[1])]
    assert b0[1] == ((0.1 + m[0]) + m[1]) + m[2] and a0[1] == ((0.1 + m[0] * ts[2]) + m[1] * ts[0]) + m[2] * ts[1]
    assert np.array_equal(rows["branch_q"][:3], [m[0] * (ts[2] - 20.0), m[1] * (ts[0] - 20.0), m[2] * (ts[1] - 20.0)])


def test_the_bypass_opens_and_closes_at_just_below_and_just_above_its_limits():
    h = unit(eff_gain=0.75, bypass_chan=2, bypass_band=1.0, bypass_min_delta=0.5)   # d = 0.5
    limit = SET + 0.5                                                   # opens when Te - 24 > 0.5 and Te - To > 0.5
    for te, want in ((limit, 0), (down(limit), 0), (up(limit), 1)):
        state, a0, b0, rows = step(h, te)
        assert state == want and rows["supply_t"][0] == (TO if want else TO + 0.75 * (te - TO)), te
        assert rows["recovered"][0] == (0.0 if want else flow(rows["supply_t"][0]) * (0.75 * (te - TO)))
    # ... on g: the extract air must be warmer than the outdoor air by more than min_delta
    te = 26.0
    for to, want in ((te - 0.5, 0), (up(te - 0.5), 0), (down(te - 0.5), 1)):
        assert step(h, te, to=to)[0] == want, to
    # closes when Te - 24 < -0.5 ...
    limit = SET - 0.5
    for te, want in ((limit, 1), (up(limit), 1), (down(limit), 0)):
        assert step(h, te, state=1)[0] == want, te
    # ... or when the outdoor air is no colder: g <= 0, at exactly 0 too; min_delta is an opening condition only
    assert step(h, SET, state=1, to=SET - 0.25)[0] == 1
    for to, want in ((SET, 0), (up(SET), 0), (down(SET), 1)):
        assert step(h, SET, state=1, to=to)[0] == want, to
    assert step(h, 30.0, state=1, to=31.0)[0] == 0                      # e > d, but the opening condition fails on g and g <= 0 closes
    # inside the dead band the state stays; a band and a min_delta of 0: strict inequalities still
    assert step(h, SET + 0.25, state=1)[0] == 1 and step(h, SET + 0.25, state=0)[0] == 0
    sharp = unit(bypass_chan=2, bypass_band=0.0, bypass_min_delta=0.0)
    assert step(sharp, SET)[0] == 0 and step(sharp, up(SET))[0] == 1
    assert step(sharp, 26.0, to=26.0)[0] == 0 and step(sharp, 26.0, to=down(26.0))[0] == 1
    # a unit without a controller recovers whatever its byte says, and leaves the byte
    state, _, _, rows = step(unit(eff_gain=0.75), 30.0, state=1)
    assert state == 1 and rows["supply_t"][0] == TO + 0.75 * (30.0 - TO)


def test_a_nan_keeps_the_bypass_state():
    h = unit(eff_gain=0.75, bypass_chan=2, bypass_band=1.0, bypass_min_delta=0.5)
    for state in (0, 1):
        assert step(h, 30.0, state=state, setpoint=np.nan)[0] == state    # would open
        assert step(h, 15.0, state=state, setpoint=np.nan)[0] == state    # would close on e < -d; the outdoor air is still colder
        assert step(h, 15.0, state=state, to=18.0, setpoint=np.nan)[0] == 0   # g <= 0 is no NaN: it closes whatever the setpoint
        got, a0, b0, rows = step(h, 30.0, state=state, to=np.nan)         # a NaN outdoor temperature: g is NaN
        assert got == state and np.isnan(rows["supply_t"][0]) and np.isnan(a0[1])
        got, _, _, rows = step(h, np.nan, state=state)                    # a NaN zone: e and g are NaN
        assert got == state and np.isnan(rows["extract_t"][0])


def test_the_coils_at_their_thresholds_and_capacities():
    te, eta = 22.0, 0.75
    tr = TO + eta * (te - TO)                                           # 19.0
    m = flow(tr)
    # Tr equal to the minimum supply: no heating; one ulp above it: heating
    for t_min, active in ((tr, False), (down(tr), False), (up(tr), True)):
        rows = step(unit(eff_gain=eta, heat_chan=3), te, t_min=t_min)[3]
        assert bool(rows["heat_active"][0]) == active and rows["supply_t"][0] == (t_min if active else tr)
        assert rows["coil_q"][0] == (m * (t_min - tr) if active else 0.0)
    for t_max, active in ((tr, False), (up(tr), False), (down(tr), True)):
        rows = step(unit(eff_gain=eta, cool_chan=4), te, t_max=t_max)[3]
        assert bool(rows["cool_active"][0]) == active and rows["supply_t"][0] == (t_max if active else tr)
        assert rows["coil_q"][0] == (0.0 - m * (tr - t_max) if active else 0.0)
    # need == cap: not saturated; nextafter(need): saturated — the capacity one ulp below the need
    need = m * (21.0 - tr)
    for cap, sat in ((need, False), (up(need), False), (down(need), True), (np.inf, False), (0.0, True)):
        rows = step(unit(eff_gain=eta, heat_chan=3, heat_cap=cap), te, t_min=21.0)[3]
        assert bool(rows["heat_saturated"][0]) == sat and rows["heat_active"][0], cap
        assert rows["coil_q"][0] == (cap if sat else need) and rows["supply_t"][0] == (tr + cap / m if sat else 21.0)
    need = m * (tr - 17.0)
    for cap, sat in ((need, False), (up(need), False), (down(need), True), (np.inf, False), (0.0, True)):
        rows = step(unit(eff_gain=eta, cool_chan=4, cool_cap=cap), te, t_max=17.0)[3]
        assert bool(rows["cool_saturated"][0]) == sat and rows["cool_active"][0], cap
        assert rows["coil_q"][0] == (0.0 - cap if sat else 0.0 - need) and rows["supply_t"][0] == (tr - cap / m if sat else 17.0)
    # heating takes precedence where both coils would act (a minimum above the maximum)
    rows = step(unit(eff_gain=eta, heat_chan=3, cool_chan=4), te, t_min=25.0, t_max=15.0)[3]
    assert rows["heat_active"][0] and not rows["cool_active"][0] and rows["supply_t"][0] == 25.0 and rows["coil_q"][0] == m * (25.0 - tr)
    # the zone receives the air at the coil's outlet; the mass flow is the exchanger's
    state, a0, b0, rows = step(unit(eff_gain=eta, heat_chan=3), te, t_min=21.0)
    assert a0[1] == 3.0 + m * 21.0 and b0[1] == 1.0 + m and rows["branch_q"][1] == m * (21.0 - 20.0)
    # the accumulators of a step
    acc = ah.fresh(unit())
    ah.accumulate(rows, acc)
    ah.accumulate(step(unit(eff_gain=eta, cool_chan=4, cool_cap=5.0, bypass_chan=2), 30.0, t_max=0.0, setpoint=20.0)[3], acc)
    assert acc["sum_heating"][0] == m * (21.0 - tr) and acc["sum_cooling"][0] == -5.0 and acc["steps_cool_saturated"][0] == 1
    assert acc["steps_bypass"][0] == 1 and acc["switches"][0] == 1 and acc["steps_heat_saturated"][0] == 0
    assert acc["sum_recovered"][0] == m * (eta * (te - TO)) + 0.0 and acc["sum_branch_q"][0] == 0.0 and acc["sum_branch_q"][1] != 0.0


def test_concat_and_balanced_build_what_apply_takes():
    a = ah.balanced([3, 4], 0, 1, eff_gain=0.8, bypass_chan=2, bypass_band=0.5, heat_chan=3, heat_cap=900.0)
    b = ah.balanced(5, [0], 1, volume_gain=2.0)
    assert a["br_zone"].tolist() == [3, 4] and a["br_kind"].tolist() == [3, 3] and a["br_unit"].tolist() == [0, 0] and a["heat_cap"].tolist() == [900.0]
    both = ah.concat(a, b)
    assert both["br_unit"].tolist() == [0, 0, 1] and both["br_volume_gain"].tolist() == [1.0, 1.0, 2.0] and both["bypass_chan"].tolist() == [2, -1]
    assert both["eff_gain"].tolist() == [0.8, 1.0] and np.isinf(both["cool_cap"]).all() and both["heat_cap"].tolist() == [900.0, np.inf]
    assert ah.n_units(both) == 2 and ah.n_branches(both) == 3 and ah.n_units({}) == 0
    T, row = np.linspace(18.0, 26.0, 6), np.array([VOLUME, TO, SET, 21.0])
    one = ah.apply(T, row, None, None, both, np.zeros(2, np.uint8))
    parts = [ah.apply(T, row, None, None, p, np.zeros(1, np.uint8)) for p in (a, b)]
    assert np.array_equal(one[2]["supply_t"], np.concatenate([p[2]["supply_t"] for p in parts]))
    assert np.array_equal(one[0], parts[0][0] + parts[1][0])
    binding.air_handlers_check(mdl.ragged_mixed(200, Z=6, seed=5)[0], both, weather=np.zeros((N_STEPS, 2, 3)), n_sub=2, channel=np.zeros((N_STEPS, 4)))


# ---- heat_air_handlers_check ----
@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


def series(md, **more):
    return dict(dict(weather=np.zeros((N_STEPS, 2, 3)), n_sub=2, channel=np.zeros((N_STEPS, 7))), **more)


def good_handlers(md):
    """Four units, twelve branches into the six zones: channels 0-1 volumes, 2 outdoor, 3 effectiveness, 4 a bypass setpoint,
    5 / 6 the supply limits. Units 0 and 2 bypass."""
    Z = int(md["n_zones"])
    j = np.arange(12)
    return dict(outdoor_chan=np.full(4, 2, np.int32), eff_chan=np.array([3, -1, 3, -1], np.int32), eff_gain=np.array([0.8, 0.7, 0.6, 0.5]),
                bypass_chan=np.array([4, -1, 4, -1], np.int32), bypass_band=np.full(4, 0.5), bypass_min_delta=np.full(4, 0.2),
                heat_chan=np.array([5, 5, -1, -1], np.int32), cool_chan=np.array([6, -1, 6, -1], np.int32),
                heat_cap=np.array([500.0, np.inf, 0.0, 1.0]), cool_cap=np.array([np.inf, 300.0, 200.0, 0.0]),
                br_unit=(j % 4).astype(np.int32), br_zone=(j % Z).astype(np.int32), br_volume_chan=(j % 2).astype(np.int32),
                br_volume_gain=np.linspace(0.5, 1.5, 12), br_kind=(1 + j % 3).astype(np.uint8))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def _raw(md, handlers, series_args=None, **fields):
    """heat_air_handlers_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**(series_args or series(md)))
    h, hkeep = binding.make_air_handlers(**handlers)
    for name, v in fields.items():
        setattr(h, name, v)
    rc = L.heat_air_handlers_check(C.byref(desc), C.byref(s), C.byref(h))
    return rc, L.heat_last_error().decode()


def changed(handlers, key, i, value):
    a = np.array(handlers[key])
    a[i] = value
    return dict(handlers, **{key: a})


def test_good_empty_and_absent_handlers_are_accepted(model):
    g = good_handlers(model)
    binding.air_handlers_check(model, g, **series(model))
    binding.air_handlers_check(model, None, **series(model))                                 # h == NULL
    binding.air_handlers_check(model, {}, **series(model))                                   # no unit
    binding.air_handlers_check(model, dict(outdoor_chan=[2, 2]), **series(model))            # units without branches
    for field in ("eff_chan", "eff_gain", "heat_chan", "cool_chan", "heat_cap", "cool_cap", "br_volume_gain", "br_kind", "bypass",
                  "sum_recovered", "sum_heating", "sum_cooling", "steps_bypass", "switches", "steps_heat_saturated", "steps_cool_saturated",
                  "sum_branch_q"):                                                           # nullable
        assert _raw(model, g, **{field: None})[0] == 0, field
    assert _raw(model, g, bypass_chan=None, bypass_band=None, bypass_min_delta=None)[0] == 0
    binding.air_handlers_check(model, dict(g, bypass=np.arange(4) % 2, sum_recovered=np.arange(4.0), switches=np.arange(4),
                                           sum_branch_q=np.arange(12.0)), **series(model))
    # band and min_delta are read only where the unit bypasses
    binding.air_handlers_check(model, changed(changed(g, "bypass_band", 1, -1.0), "bypass_min_delta", 3, np.nan), **series(model))


def test_negative_counts_null_arrays_and_branches_without_units_are_invalid_arguments(model):
    g = good_handlers(model)
    rc, msg = _raw(model, g, n_units=-1)
    assert rc == E_INVALID_ARG and "air handler u" in msg and "n_units -1" in msg, msg
    rc, msg = _raw(model, g, n_branches=-1)
    assert rc == E_INVALID_ARG and "air handler branch j" in msg and "n_branches -1" in msg, msg
    rc, msg = _raw(model, g, n_units=0)
    assert rc == E_INVALID_ARG and "air handler branch 0" in msg and "n_units 0" in msg, msg
    rc, msg = _raw(model, g, outdoor_chan=None)
    assert rc == E_INVALID_ARG and "air handler 0" in msg and "outdoor_chan" in msg, msg
    for field in ("br_unit", "br_zone", "br_volume_chan"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "air handler branch 0" in msg and field in msg, (field, msg)
    for field in ("bypass_band", "bypass_min_delta"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "air handler 0:" in msg and field in msg, (field, msg)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, -0.5])
def test_values_that_are_negative_or_not_finite_are_refused(model, bad):
    g = good_handlers(model)
    for key in ("bypass_band", "bypass_min_delta"):
        code, msg = _code(lambda: binding.air_handlers_check(model, changed(g, key, 2, bad), **series(model)))     # unit 2 bypasses
        assert code == E_INVALID_ARG and "air handler 2:" in msg and key in msg, msg
    for key, i, name in (("eff_gain", 1, "air handler 1:"), ("br_volume_gain", 7, "air handler branch 7:")):
        if not np.isfinite(bad):
            code, msg = _code(lambda: binding.air_handlers_check(model, changed(g, key, i, bad), **series(model)))
            assert code == E_INVALID_ARG and name in msg and key in msg, msg
        else:
            binding.air_handlers_check(model, changed(g, key, i, bad), **series(model))      # a negative gain is the caller's business
    for key in ("heat_cap", "cool_cap"):
        if bad == np.inf:
            binding.air_handlers_check(model, changed(g, key, 3, bad), **series(model))      # +inf: unlimited
        else:
            code, msg = _code(lambda: binding.air_handlers_check(model, changed(g, key, 3, bad), **series(model)))
            assert code == E_INVALID_ARG and "air handler 3:" in msg and key in msg, msg


def test_a_kind_outside_one_to_three_and_a_bypass_byte_above_one_are_refused(model):
    g = good_handlers(model)
    for bad in (0, 4, 255):
        code, msg = _code(lambda: binding.air_handlers_check(model, changed(g, "br_kind", 6, bad), **series(model)))
        assert code == E_INVALID_ARG and "air handler branch 6:" in msg and "br_kind" in msg, msg
    for bad in (2, 255):
        state = np.zeros(4, np.uint8)
        state[3] = bad
        code, msg = _code(lambda: binding.air_handlers_check(model, dict(g, bypass=state), **series(model)))
        assert code == E_INVALID_ARG and "air handler 3:" in msg and "bypass" in msg, msg


def test_units_zones_and_channels_out_of_range_are_size_errors(model):
    Z = int(model["n_zones"])
    g = good_handlers(model)
    for key, n, what in (("br_unit", 4, "unit"), ("br_zone", Z, "zone"), ("br_volume_chan", 7, "volume channel")):
        for bad in (-1, n, n + 12345, -2 ** 31):
            code, msg = _code(lambda: binding.air_handlers_check(model, changed(g, key, 5, bad), **series(model)))
            assert code == E_SIZE and "air handler branch 5:" in msg and what in msg, msg
    for bad in (-1, 7, 2 ** 31 - 1):
        code, msg = _code(lambda: binding.air_handlers_check(model, changed(g, "outdoor_chan", 1, bad), **series(model)))
        assert code == E_SIZE and "air handler 1:" in msg and "outdoor channel" in msg, msg
    for key in ("eff_chan", "bypass_chan", "heat_chan", "cool_chan"):
        for bad in (-2, 7, -2 ** 31):
            code, msg = _code(lambda: binding.air_handlers_check(model, changed(g, key, 2, bad), **series(model)))
            assert code == E_SIZE and "air handler 2:" in msg and "channel" in msg, msg
        binding.air_handlers_check(model, changed(g, key, 2, -1), **series(model))           # -1: none
    # no channels at all: every outdoor channel is out of range
    code, msg = _code(lambda: binding.air_handlers_check(model, g, **series(model, channel=None)))
    assert code == E_SIZE and "air handler 0:" in msg, msg


def test_march_without_a_batch_is_an_invalid_argument(model):
    """What heat_batch_march_series_handlers can answer without a batch, and so without a device. That bad handlers are refused
    BEFORE any device work needs a batch: the GPU test test_bad_handlers_and_sharded_batches_are_refused_by_the_march finds the
    device state untouched behind every refusal."""
    L = binding.load_library()
    s, _ = binding.make_series(**series(model))
    h, _ = binding.make_air_handlers(**good_handlers(model))
    failed = C.c_int32(123)
    call = binding.SeriesCall(size=C.sizeof(binding.SeriesCall), s=C.pointer(s), failed_step=C.pointer(failed))
    assert L.heat_batch_march_series_handlers(None, C.byref(call), None, None, None, C.byref(h), None, None, None, None) == E_INVALID_ARG
    assert failed.value == -1
    assert L.heat_batch_march_series_handlers(*([None] * 10)) == E_INVALID_ARG
    call.size = 8
    assert L.heat_batch_march_series_handlers(None, C.byref(call), None, None, None, C.byref(h), None, None, None, None) == E_INVALID_ARG


def test_the_wrapper_reads_the_shapes(model):
    h, keep = binding.make_air_handlers(**good_handlers(model))
    assert h.n_units == 4 and h.n_branches == 12 and keep["br_kind"].dtype == np.uint8 and keep["bypass"].dtype == np.uint8
    assert keep["switches"].dtype == np.int64 and keep["sum_branch_q"].shape == (12,) and not keep["bypass"].any() and not keep["sum_heating"].any()
    h, keep = binding.make_air_handlers()
    assert h.n_units == 0 and h.n_branches == 0 and not h.outdoor_chan and not h.bypass and not h.sum_recovered
    resume = np.arange(4.0)
    h, keep = binding.make_air_handlers(**dict(good_handlers(model), sum_recovered=resume))
    assert np.array_equal(keep["sum_recovered"], resume) and keep["sum_recovered"] is not resume
    h, keep = binding.make_air_handlers(**dict(good_handlers(model), stats=("switches",)))
    assert not h.sum_recovered and not h.steps_bypass and not h.sum_branch_q and h.switches and h.bypass and "sum_heating" not in keep
    for bad in (dict(br_zone=np.zeros(11)), dict(eff_gain=np.zeros(3)), dict(bypass=np.zeros(5)), dict(stats=("sum",)),
                dict(stats=(), sum_cooling=np.zeros(4)), dict(sum_branch_q=np.zeros(4))):
        with pytest.raises(ValueError):
            binding.make_air_handlers(**dict(good_handlers(model), **bad))


# ---- the generator's cases: accepted, and — through the CPU oracle alone — they exercise the bypass and the coils ----
COVERAGE_CASES = [("ragged_mixed", 2), ("rooms_with_windows", 2), ("rooms_with_windows", 5), ("rooms_with_windows_large", 5),
                  ("partitioned_buildings_large", 2)]


@pytest.mark.parametrize("model_name,n_sub", COVERAGE_CASES)
def test_the_generators_cases_are_accepted_and_their_controllers_move(oracle, model_name, n_sub):
    c = ahc.case(model_name, ahc.N_STEPS, n_sub, 2, ahc.SEED)
    md, h, info = c["md"], c["handlers"], c["info"]
    kw = dict(weather=c["w"], n_sub=n_sub, channel=c["channel"], probes=c["probes"])
    binding.air_handlers_check(md, h, **kw)
    binding.air_paths_check(md, c["air"], **kw)
    binding.zone_loads_check(md, c["loads"], **kw)
    # what the generator promises
    U, B, Z = ah.n_units(h), ah.n_branches(h), int(md["n_zones"])
    assert U == ahc.N_UNITS.get(Z, U) and (U < 64 or (U > 256 and U % 64 != 0))
    per_unit = np.bincount(h["br_unit"], minlength=U)
    assert per_unit[ahc.HUB] == ahc.HUB_BRANCHES + 1 and per_unit.min() >= 1 and {1, 2, 3} <= set(h["br_kind"].tolist())
    rest = np.delete(per_unit, [ahc.HUB, ahc.SUPPLY_ONLY, ahc.PLAIN])
    assert rest.max() <= 6
    assert set(h["br_kind"][h["br_unit"] == ahc.EXTRACT_ONLY].tolist()) == {2} and set(h["br_kind"][h["br_unit"] == ahc.SUPPLY_ONLY].tolist()) == {1}
    supplies = (h["br_kind"] & 1) != 0
    assert len(set(h["br_unit"][supplies & (h["br_zone"] == ahc.SHARED_ZONE)].tolist())) >= 3
    for key, share in (("bypass_chan", 0.6), ("heat_chan", 0.6), ("cool_chan", 0.5)):
        assert abs(float((h[key] >= 0).mean()) - share) <= 0.25, key
    caps = np.concatenate([h["heat_cap"], h["cool_cap"]])
    assert 0.2 <= float(np.isinf(caps).mean()) <= 0.6
    assert np.isnan(c["channel"][info["nan_steps"], h["bypass_chan"][ahc.NAN_UNIT]]).all() and len(info["nan_steps"]) == 4
    assert not np.array_equal(np.argsort(h["br_unit"], kind="stable"), np.arange(B))            # shuffled
    if U > 256:                                                                                  # branches into the other workgroup's zones
        assert ((h["br_unit"] < 256) & (h["br_zone"] >= 256)).any() and ((h["br_unit"] >= 256) & (h["br_zone"] < 256)).any()
    # the oracle loop alone
    big = md["n_surfaces"] > 8192
    m = oracle.OracleModel(md)

    def march(s, wk, za, zb):
        assert m.march(s, wk, za, zb, threads=16 if big else 1)[0] == 0

    out = ahc.loop_with_rules(march, c, c["st"].copy())
    ahc.assert_coverage(ahc.coverage(h, out), "%s n_sub=%d, %d units, %d branches" % (model_name, n_sub, U, B))
    for key in ("trace",) + ah.ROWS:
        assert np.all(np.isfinite(out[key])), key
    # the accumulators are the sums of the returned rows
    acc = out["carry"]["handlers"]
    assert np.array_equal(acc["steps_bypass"], out["bypass"].sum(axis=0)) and np.array_equal(acc["bypass"], out["bypass"][-1].astype(np.uint8))
    assert np.array_equal(acc["switches"], (np.diff(np.concatenate([np.zeros((1, U), bool), out["bypass"]]).astype(np.int8), axis=0) != 0).sum(axis=0))
    assert np.array_equal(acc["steps_heat_saturated"], out["heat_saturated"].sum(axis=0))
    assert np.array_equal(acc["steps_cool_saturated"], out["cool_saturated"].sum(axis=0))
    q = out["coil_q"]
    for key, rows in (("sum_recovered", out["recovered"]), ("sum_heating", np.where(q > 0, q, 0.0)), ("sum_cooling", np.where(q < 0, q, 0.0)),
                      ("sum_branch_q", out["branch_q"])):
        total = np.zeros(rows.shape[1])
        for r in rows:
            total = total + r
        assert np.array_equal(acc[key], total), key
    assert not out["branch_q"][:, ~supplies].any() and not acc["switches"][h["bypass_chan"] < 0].any()
    assert (out["heat_active"] & out["cool_active"]).sum() == 0


def test_air_handlers_check_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "air_handlers_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "air handlers host check: all statuses as the header states them" in out.stdout
