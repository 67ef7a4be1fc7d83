"""Comfort of a series on the host (include/heat_amd.h, heat_comfort / heat_comfort_check / heat_batch_march_series_comfort;
heat_amd/comfort.py): the entry points are declared, exported and bound; the ctypes mirror has the header's layout and
heat_series_call keeps its size; the rule in numpy (comfort.operative, control_temperatures, accumulate — the reference of
tests/test_comfort_gpu.py) gives the hand-worked cases; every refusal the header lists comes back with its code and names the
sensor or the entry, before any device work; the case builder of the GPU tests takes every branch of the rule on a synthetic
march that moves zone and face temperatures, its control sensors change what thermostats, air paths and blinds decide, and
its oracle loop keeps every decision away from a tie. heat_comfort_check also runs under AddressSanitizer / UBSan as a
stand-alone program (tests/comfort_host_main.cpp) in a child process. No GPU needed.

Reference: the rule is this project's own (the reference has no comfort model)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from heat_amd import air_paths, binding, comfort as cf, modeldict as mdl
import comfort_cases as cc
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_comfort_check", "heat_batch_march_series_comfort")
E_INVALID_ARG, E_SIZE = -1, -4
N_STEPS = 4
FIELDS = ("n_sensors", "zone", "air_weight", "control", "n_entries", "en_sensor", "en_surface", "en_side", "en_weight", "occ_chan", "lo_chan",
          "hi_chan", "resume", "step_base", "n_occupied", "sum_operative", "min_operative", "step_min", "max_operative", "step_max", "n_below",
          "deg_below", "n_above", "deg_above", "max_above", "step_max_above")
MARGIN = 1e-6      # as the blinds tests: how far a comparison of the oracle loop must be from a tie for its outcome to be compared exactly


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_comfort {" in header
    assert "heat_comfort_check" in binding.HOST_ONLY_SYMBOLS and "heat_batch_march_series_comfort" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("Comfort", "make_comfort", "comfort_check"))
    assert all(hasattr(cf, n) for n in ("operative", "control_temperatures", "accumulate", "by_area"))
    assert L.heat_amd_abi_version() == 1
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW) and "pub struct HeatComfort" in rust
    # the positional entry points and the one-struct call stay as they are: the term rides beside them
    assert binding.HeatBatch._SERIES_ENTRY[-1][0] == "heat_batch_march_series_blinds" and "comfort" not in binding.HeatBatch._SERIES_ORDER
    assert "comfort" not in [f for f, _ in binding.SeriesCall._fields_]
    # the header says who keeps the air temperature
    assert "ideal loads and the ambient drive's mix keep the air temperature" in header


def test_comfort_layout_matches_the_header_and_the_series_call_keeps_its_size(tmp_path):
    src = tmp_path / "sz.c"
    args = ["sizeof(heat_comfort)", "sizeof(heat_series_call)", "sizeof(heat_blinds)", "sizeof(heat_air_paths)"] + ["offsetof(heat_comfort, %s)" % f for f in FIELDS]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == ([C.sizeof(binding.Comfort), C.sizeof(binding.SeriesCall), C.sizeof(binding.Blinds), C.sizeof(binding.AirPaths)] +
                   [getattr(binding.Comfort, f).offset for f in FIELDS])
    assert [f for f, _ in binding.Comfort._fields_] == list(FIELDS)
    assert got[0] == 8 * len(FIELDS) and got[1] == 8 * 24          # (heat_series_call: 24 fields of 8 bytes, as before this term)


# ---- the rule in numpy: hand-worked cases ----
def test_a_sensor_of_three_faces():
    s = dict(zone=[1], air_weight=[0.25], en_sensor=[0, 0, 0], en_surface=[0, 1, 2], en_side=[0, 1, 0], en_weight=[0.5, 0.3, 0.2])
    face, Tz = np.array([18.0, 21.5, 30.1]), np.array([99.0, 24.0])
    r, top = cf.operative(face, Tz, s)
    want = ((0.0 + 0.5 * 18.0) + 0.3 * 21.5) + 0.2 * 30.1
    assert r[0] == want and top[0] == 0.25 * 24.0 + (1.0 - 0.25) * want
    # the order is the caller's: the same faces in another order round differently somewhere (a sum of three is not associative)
    w, t = np.ones(3), np.array([1e16, -1e16, 1.0])
    a = cf.operative(t, Tz, dict(s, en_weight=w))[0][0]
    b = cf.operative(t[::-1], Tz, dict(s, en_weight=w))[0][0]
    assert a == ((0.0 + 1e16) + -1e16) + 1.0 == 1.0 and b == ((0.0 + 1.0) + -1e16) + 1e16 == 0.0
    # entries listed in any order are summed per sensor in the caller's order
    two = dict(zone=[0, 1], en_sensor=[1, 0, 1, 0], en_surface=[0, 1, 2, 3], en_side=[0, 0, 0, 0], en_weight=[0.5, 0.25, 0.5, 0.75])
    r, top = cf.operative(np.array([20.0, 10.0, 30.0, 40.0]), np.array([22.0, 26.0]), two)
    assert r[0] == (0.0 + 0.25 * 10.0) + 0.75 * 40.0 and r[1] == (0.0 + 0.5 * 20.0) + 0.5 * 30.0
    assert top[0] == 0.5 * 22.0 + 0.5 * r[0] and top[1] == 0.5 * 26.0 + 0.5 * r[1]                       # (air_weight NULL: 0.5)


def test_an_empty_sensor_the_air_weights_a_face_twice_and_a_face_of_another_zone():
    md, st = mdl.ragged_mixed(60, Z=4, seed=3)
    empty = dict(zone=[2], air_weight=[0.4])
    r, top = cf.operative(np.zeros(0), np.array([1.0, 2.0, 25.0, 4.0]), empty)
    assert r[0] == 0.0 and top[0] == 0.4 * 25.0 + (1.0 - 0.4) * 0.0 and len(cf.face_slots(md, empty)) == 0
    s = dict(zone=[0, 0, 0], en_sensor=[0, 1, 2], en_surface=[5, 5, 5], en_side=[0, 0, 0], en_weight=[1.0, 1.0, 1.0])
    for a, want in ((0.0, 19.0), (1.0, 23.0), (None, 0.5 * 23.0 + 0.5 * 19.0)):
        r, top = cf.operative(np.full(3, 19.0), np.array([23.0]), dict(s, air_weight=None if a is None else [a] * 3))
        assert np.all(r == 19.0) and np.all(top == want), (a, top)
    twice = dict(zone=[0], en_sensor=[0, 0], en_surface=[7, 7], en_side=[1, 1], en_weight=[0.5, 0.5])
    slots = cf.face_slots(md, twice)
    assert slots[0] == slots[1] == md["first_node_slot"][7] + np.diff(md["node_offset"])[7] - 1
    state = st.copy()
    state[slots[0]] = 17.3
    assert cf.operative(state[slots], state[md["zone_slot"]], twice)[0][0] == (0.0 + 0.5 * 17.3) + 0.5 * 17.3
    # a face of another zone: the rule does not ask which zone a face looks at
    q = int(np.flatnonzero((md["back_zone"] != 0) & (md["front_zone"] != 0))[0])
    other = dict(zone=[0], en_sensor=[0], en_surface=[q], en_side=[0], en_weight=[1.0])
    state[cf.face_slots(md, other)] = 31.0
    assert cf.face_slots(md, other)[0] == md["first_node_slot"][q] and cf.operative(state[cf.face_slots(md, other)], state[md["zone_slot"]], other)[0][0] == 31.0


def test_the_control_temperature_is_the_control_sensors_operative_temperature():
    s = dict(zone=[2, 0, 2], control=[0, 1, 1])
    Tz, top = np.array([20.0, 21.0, 22.0, 23.0]), np.array([30.0, 31.0, 32.0])
    assert list(cf.control_temperatures(Tz, top, s)) == [31.0, 21.0, 32.0, 23.0]
    assert list(cf.control_temperatures(Tz, top, dict(s, control=None))) == list(Tz) and list(cf.control_temperatures(Tz, np.zeros(0), {})) == list(Tz)
    assert cf.control_temperatures(Tz, top, s) is not Tz


def test_unoccupied_steps_count_nothing_and_extrema_keep_their_first_occurrence():
    s = dict(zone=[0, 0], occ_chan=[0, -1], lo_chan=[1, 1], hi_chan=[2, 2])
    acc = cf.fresh(2)
    assert acc["min_operative"][0] == np.inf and acc["max_operative"][0] == -np.inf and acc["max_above"][0] == -np.inf and acc["step_min"][0] == -1
    rows = [[1.0, 20.0, 24.0], [0.0, 20.0, 24.0], [-1.0, 20.0, 24.0], [np.nan, 20.0, 24.0], [2.0, 20.0, 24.0], [1.0, 20.0, 24.0], [1.0, 20.0, 24.0]]
    tops = [22.0, 19.0, 26.0, 18.0, 19.5, 19.5, 22.0]
    for k, (row, top) in enumerate(zip(rows, tops)):
        cf.accumulate(np.array([top, top]), np.array(row), s, acc, 100 + k)
    # sensor 0 is occupied at steps 0, 4, 5, 6 (0, a negative and a NaN occupancy count nothing); sensor 1 always
    assert list(acc["n_occupied"]) == [4, 7]
    assert acc["sum_operative"][0] == (((0.0 + 22.0) + 19.5) + 19.5) + 22.0
    assert (acc["min_operative"][0], acc["step_min"][0]) == (19.5, 104)                               # strict: the FIRST of two equal minima
    assert (acc["max_operative"][0], acc["step_max"][0]) == (22.0, 100)                               # ... and maxima
    assert (acc["min_operative"][1], acc["step_min"][1], acc["max_operative"][1], acc["step_max"][1]) == (18.0, 103, 26.0, 102)
    assert list(acc["n_below"]) == [2, 4] and list(acc["n_above"]) == [0, 1]
    assert acc["deg_below"][0] == (0.0 + (20.0 - 19.5)) + (20.0 - 19.5)
    assert acc["deg_below"][1] == (((0.0 + (20.0 - 19.0)) + (20.0 - 18.0)) + (20.0 - 19.5)) + (20.0 - 19.5)
    assert (acc["max_above"][0], acc["step_max_above"][0]) == (-np.inf, -1) and (acc["max_above"][1], acc["step_max_above"][1], acc["deg_above"][1]) == (2.0, 102, 2.0)


def test_max_above_with_its_step_and_limits_that_are_channels():
    s = dict(zone=[0], hi_chan=[0], lo_chan=[-1])
    acc = cf.fresh(1)
    for k, (hi, top) in enumerate(((24.0, 25.0), (25.5, 26.0), (23.0, 24.0), (23.0, 24.0), (26.0, 25.9), (20.0, 23.5))):
        occ, below, above = cf.accumulate(np.array([top]), np.array([hi]), s, acc, k)
        assert occ[0] and not below[0] and above[0] == (top > hi)
    assert acc["n_above"][0] == 5 and acc["n_below"][0] == 0 and acc["deg_below"][0] == 0.0
    assert acc["deg_above"][0] == ((((0.0 + 1.0) + 0.5) + 1.0) + 1.0) + 3.5
    assert (acc["max_above"][0], acc["step_max_above"][0]) == (3.5, 5)
    acc = cf.fresh(1)
    for k, top in enumerate((25.0, 25.0, 24.5)):                                                        # the first of two equal exceedances
        cf.accumulate(np.array([top]), np.array([24.0]), s, acc, 10 + k)
    assert (acc["max_above"][0], acc["step_max_above"][0]) == (1.0, 10)
    # only the accumulators that are there are maintained
    some = dict(n_above=np.zeros(1, np.int64), max_above=np.full(1, -np.inf))
    cf.accumulate(np.array([25.0]), np.array([24.0]), s, some, 3)
    assert set(some) == {"n_above", "max_above"} and some["n_above"][0] == 1 and some["max_above"][0] == 1.0


def test_a_nan_face_and_a_nan_limit():
    s = dict(zone=[0, 0], en_sensor=[0, 1], en_surface=[0, 1], en_side=[0, 0], en_weight=[1.0, 1.0], lo_chan=[0, 0], hi_chan=[1, 1])
    r, top = cf.operative(np.array([np.nan, 21.0]), np.array([22.0]), s)
    assert np.isnan(r[0]) and np.isnan(top[0]) and top[1] == 0.5 * 22.0 + 0.5 * 21.0
    acc = cf.fresh(2)
    occ, below, above = cf.accumulate(top, np.array([25.0, np.nan]), s, acc, 0)
    # a NaN makes every comparison false: the NaN sensor is counted as occupied and summed, but is no extremum and outside no limit
    assert list(acc["n_occupied"]) == [1, 1] and np.isnan(acc["sum_operative"][0]) and acc["min_operative"][0] == np.inf and acc["step_max"][0] == -1
    assert list(below) == [False, True] and list(above) == [False, False] and list(acc["n_above"]) == [0, 0]          # (a NaN upper limit)
    assert list(cf.control_temperatures(np.array([22.0]), top, dict(s, control=[1, 0]))) != [22.0]


def test_by_area_weights_sum_to_one_per_sensor():
    md, _ = mdl.rooms_with_windows(300, Z=20, seed=6)
    for weight in (None, np.random.default_rng(1).uniform(0.5, 1.0, 300), (np.full(300, 0.9), np.full(300, 0.6))):
        s = cf.by_area(md, air_weight=0.45, weight=weight, control=True)
        Z = int(md["n_zones"])
        assert list(s["zone"]) == list(range(Z)) and np.all(s["air_weight"] == 0.45) and np.all(s["control"] == 1)
        total = np.zeros(Z)
        np.add.at(total, s["en_sensor"], s["en_weight"])
        faced = np.bincount(s["en_sensor"], minlength=Z) > 0
        assert faced.any() and np.allclose(total[faced], 1.0, rtol=0, atol=1e-14) and np.all(total[~faced] == 0.0)
        # an entry is a side that faces the sensor's zone
        zone_of = np.where(s["en_side"] > 0, md["back_zone"][s["en_surface"]], md["front_zone"][s["en_surface"]])
        kind_of = np.where(s["en_side"] > 0, md["back_kind"][s["en_surface"]], md["front_kind"][s["en_surface"]])
        assert np.array_equal(zone_of, s["en_sensor"]) and np.all(kind_of == mdl.SPACE)
        assert len(s["en_sensor"]) == int((md["front_kind"] == mdl.SPACE).sum() + (md["back_kind"] == mdl.SPACE).sum())
        binding.comfort_check(md, s, **series(md))
    assert not cf.by_area(md)["control"].any()


def test_air_paths_sense_the_control_temperature_for_e_alone():
    air = dict(target=[0], source=[1], volume_chan=[0], open_chan=[1], sense=[1], band=[0.2], min_delta=[0.5])
    row, T = np.array([0.01, 24.0]), np.array([23.0, 20.0])
    state = np.zeros(1, np.uint8)
    a, b, q = air_paths.apply(T, row, None, None, air, state)                  # the air is below the setpoint: closed
    assert state[0] == 0 and q[0] == 0.0
    a1, b1, q1 = air_paths.apply(T, row, None, None, air, state, control_T=np.array([25.0, 99.0]))       # the room FEELS warm: open
    assert state[0] == 1 and q1[0] < 0.0
    # ... and the air that moves is air: the same powers as a path that opened sensing air at 25 degrees would not give
    state2 = np.ones(1, np.uint8)
    a2, b2, q2 = air_paths.apply(T, row, None, None, dict(air, open_chan=[-1]), state2)
    assert q1[0] == q2[0] and a1[0] == a2[0] and b1[0] == b2[0]
    # control_T=None and control_T=T are today's rule
    for ctl in (None, T):
        s3 = np.zeros(1, np.uint8)
        assert np.array_equal(air_paths.apply(T, row, None, None, air, s3, control_T=ctl)[2], q) and s3[0] == 0


# ---- heat_comfort_check ----
@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


def series(md, **more):
    return dict(dict(weather=np.zeros((N_STEPS, 2, 3)), n_sub=2, channel=np.zeros((N_STEPS, 3))), **more)


def good_comfort(md, n=40):
    rng = np.random.default_rng(4)
    i = np.arange(n)
    Z, S = int(md["n_zones"]), int(md["n_surfaces"])
    ne = 5 * n
    return dict(zone=(i % Z).astype(np.int32), air_weight=rng.uniform(0, 1, n), control=(i < Z - 1).astype(np.uint8),
                en_sensor=rng.integers(0, n, ne), en_surface=rng.integers(0, S, ne), en_side=rng.integers(0, 2, ne), en_weight=rng.uniform(-1, 1, ne),
                occ_chan=np.where(i % 2 == 0, 0, -1), lo_chan=np.where(i % 3 == 0, 1, -1), hi_chan=np.where(i % 3 == 1, 2, -1))


def check(md, comfort, **more):
    binding.comfort_check(md, comfort, **series(md, **more))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def _raw(md, comfort, **fields):
    """heat_comfort_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**series(md))
    c, ckeep = binding.make_comfort(**comfort)
    for name, v in fields.items():
        setattr(c, name, v)
    rc = L.heat_comfort_check(C.byref(desc), C.byref(s), C.byref(c))
    return rc, L.heat_last_error().decode()


def test_good_empty_and_absent_terms_are_accepted(model):
    g = good_comfort(model)
    check(model, g)
    check(model, None)
    check(model, {})
    check(model, {k: v for k, v in g.items() if k in ("zone", "en_sensor", "en_surface", "en_side", "en_weight")})
    check(model, {k: v for k, v in g.items() if not k.startswith("en_")})                    # sensors without any entry
    check(model, dict(g, stats=()))
    check(model, dict(g, stats=("min_operative", "max_above", "n_below")))                   # extrema without their steps
    check(model, dict(g, resume=cf.fresh(40), step_base=1000))


def test_counts_null_arrays_and_steps_without_their_extremum_are_invalid_arguments(model):
    g = good_comfort(model)
    rc, msg = _raw(model, g, n_sensors=-1)
    assert rc == E_INVALID_ARG and "comfort sensor" in msg and "n_sensors -1" in msg, msg
    rc, msg = _raw(model, g, n_entries=-1)
    assert rc == E_INVALID_ARG and "comfort entry" in msg and "n_entries -1" in msg, msg
    rc, msg = _raw(model, g, zone=None)
    assert rc == E_INVALID_ARG and "comfort sensor 0" in msg and "zone" in msg, msg
    for field in ("en_sensor", "en_surface", "en_side", "en_weight"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "comfort entry 0" in msg and field in msg, (field, msg)
    for step, ext in (("step_min", "min_operative"), ("step_max", "max_operative"), ("step_max_above", "max_above")):
        rc, msg = _raw(model, g, **{ext: None})
        assert rc == E_INVALID_ARG and "comfort sensor" in msg and step in msg and ext in msg, msg
        assert _raw(model, g, **{ext: None, step: None})[0] == 0
    for field in ("air_weight", "control", "occ_chan", "lo_chan", "hi_chan", "n_occupied", "sum_operative", "n_below", "deg_below", "n_above",
                  "deg_above", "step_min", "step_max", "step_max_above"):
        assert _raw(model, g, **{field: None})[0] == 0, field                                # the nullable ones
    assert _raw(model, g, n_entries=0, en_sensor=None, en_surface=None, en_side=None, en_weight=None)[0] == 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_weights_that_are_not_finite_are_refused(model, bad):
    g = good_comfort(model)
    a = g["en_weight"].copy()
    a[133] = bad
    code, msg = _code(lambda: check(model, dict(g, en_weight=a)))
    assert code == E_INVALID_ARG and "comfort entry 133:" in msg and "en_weight" in msg, msg
    a = g["air_weight"].copy()
    a[31] = bad
    code, msg = _code(lambda: check(model, dict(g, air_weight=a)))
    assert code == E_INVALID_ARG and "comfort sensor 31:" in msg and "air_weight" in msg, msg


def test_air_weights_outside_the_unit_interval_and_control_bytes_above_one_are_refused(model):
    g = good_comfort(model)
    for bad in (-1e-9, 1.0 + 1e-9, 2.0):
        a = g["air_weight"].copy()
        a[17] = bad
        code, msg = _code(lambda: check(model, dict(g, air_weight=a)))
        assert code == E_INVALID_ARG and "comfort sensor 17:" in msg and "air_weight" in msg, msg
    for fine in (0.0, 1.0):
        a = g["air_weight"].copy()
        a[17] = fine
        check(model, dict(g, air_weight=a))
    a = g["control"].copy()
    a[22] = 2
    code, msg = _code(lambda: check(model, dict(g, control=a)))
    assert code == E_INVALID_ARG and "comfort sensor 22:" in msg and "control" in msg, msg


def test_numbers_out_of_range_are_size_errors(model):
    g = good_comfort(model)
    Z, S = int(model["n_zones"]), int(model["n_surfaces"])
    for bad in (-1, Z, 2 ** 31 - 1):
        a = g["zone"].copy()
        a[39] = bad
        code, msg = _code(lambda: check(model, dict(g, zone=a)))
        assert code == E_SIZE and "comfort sensor 39:" in msg and "zone" in msg, msg
    for bad in (-2, 3, 2 ** 31 - 1):                                                         # (the series has three channels)
        for key, i in (("occ_chan", 7), ("lo_chan", 11), ("hi_chan", 0)):
            a = g[key].copy()
            a[i] = bad
            code, msg = _code(lambda: check(model, dict(g, **{key: a})))
            assert code == E_SIZE and "comfort sensor %d:" % i in msg and "channel" in msg, msg
    for bad in (-1, 40, 2 ** 31 - 1):
        a = g["en_sensor"].copy()
        a[199] = bad
        code, msg = _code(lambda: check(model, dict(g, en_sensor=a)))
        assert code == E_SIZE and "comfort entry 199:" in msg and "sensor" in msg, msg
    for bad in (-1, S, 2 ** 40):
        a = g["en_surface"].copy()
        a[0] = bad
        code, msg = _code(lambda: check(model, dict(g, en_surface=a)))
        assert code == E_SIZE and "comfort entry 0:" in msg and "surface" in msg, msg
    a = g["en_side"].copy()
    a[64] = 2
    code, msg = _code(lambda: check(model, dict(g, en_side=a)))
    assert code == E_SIZE and "comfort entry 64:" in msg and "side" in msg, msg
    a = g["control"].copy()
    a[Z + 2] = 1                                                                             # (sensors 2 and Z + 2 stand in zone 2)
    code, msg = _code(lambda: check(model, dict(g, control=a)))
    assert code == E_SIZE and "comfort sensor %d:" % (Z + 2) in msg and "already" in msg, msg
    a[2] = 0
    check(model, dict(g, control=a))                                                         # the second sensor of the zone alone


def test_march_without_a_batch_is_an_invalid_argument(model):
    L = binding.load_library()
    s, _ = binding.make_series(**series(model))
    c, _ = binding.make_comfort(**good_comfort(model))
    failed = C.c_int32(123)
    call = binding.SeriesCall(size=C.sizeof(binding.SeriesCall), s=C.pointer(s), failed_step=C.pointer(failed))
    assert L.heat_batch_march_series_comfort(None, C.byref(call), C.byref(c), None, None) == E_INVALID_ARG
    assert failed.value == -1
    call.size = 8                                                                            # a struct of another size is not read further
    assert L.heat_batch_march_series_comfort(None, C.byref(call), C.byref(c), None, None) == E_INVALID_ARG
    assert "sizeof(heat_series_call)" in L.heat_last_error().decode()


def test_the_wrapper_reads_the_shapes(model):
    c, keep = binding.make_comfort(**good_comfort(model))
    assert c.n_sensors == 40 and c.n_entries == 200 and c.resume == 0 and c.step_base == 0
    assert keep["zone"].dtype == np.int32 and keep["en_surface"].dtype == np.int64 and keep["en_side"].dtype == np.uint8 and keep["control"].dtype == np.uint8
    assert set(binding.COMFORT_STATS) <= set(keep) and keep["step_min"].dtype == np.int64 and keep["max_above"].dtype == np.float64
    assert tuple(binding.COMFORT_STATS) == tuple(cf.ACC)
    c, keep = binding.make_comfort()
    assert c.n_sensors == 0 and c.n_entries == 0 and not c.zone and not c.en_sensor
    c, keep = binding.make_comfort(**good_comfort(model), stats=("n_above",))
    assert c.n_above and not c.n_below and not c.min_operative and "sum_operative" not in keep
    given = cf.fresh(40)
    given["n_occupied"][:] = 5
    c, keep = binding.make_comfort(**good_comfort(model), resume=given, step_base=77)
    assert c.resume == 1 and c.step_base == 77 and np.array_equal(keep["n_occupied"], given["n_occupied"]) and keep["n_occupied"] is not given["n_occupied"]
    assert keep["min_operative"][0] == np.inf
    for bad in (dict(air_weight=np.ones(39)), dict(en_weight=np.zeros(3)), dict(stats=("nonsense",)), dict(resume=dict(n_occupied=np.zeros(40)))):
        with pytest.raises(ValueError):
            binding.make_comfort(**dict(good_comfort(model), **bad))


# ---- the case builder of the GPU tests ----
def synthetic(md, st):
    """A stand-in march that moves the zone AND the node temperatures, each with its own phase."""
    T0, nodes = st[md["zone_slot"]].copy(), mdl.node_slots(md)
    N0 = st[nodes].copy()

    def march(state, k, za, zb):
        state[md["zone_slot"]] = T0 + 1.5 * np.sin(0.8 * k + np.arange(len(T0)))
        state[nodes] = N0 + 2.0 * np.cos(0.37 * k + 0.01 * np.arange(len(nodes)))

    return march


@pytest.mark.parametrize("seed", [501, 502, 505])
def test_the_case_builder_takes_every_branch_and_its_control_sensors_change_the_decisions(seed):
    md, st = mdl.ragged_mixed(700, Z=28, seed=1)
    c = cc.comfort_case(md, st, np.random.default_rng(seed))
    march = synthetic(md, st)
    state = st.copy()
    march(state, -1, None, None)
    ref = cc.loop(c, state, march, md["zone_slot"])
    cov = cc.coverage(c, ref)
    # occupied and unoccupied steps; below, above and inside the band; each extremum updated more than once
    assert cov["occupied"] > 1000 and cov["unoccupied"] > 1000 and cov["below"] > 200 and cov["above"] > 200 and cov["inside"] > 100, cov
    assert cov["min_twice"] > 50 and cov["max_twice"] > 50 and cov["above_twice"] > 20, cov
    acc = ref["carry"]["comfort"]
    top, occ = ref["operative"], ref["occupied"]
    assert np.array_equal(acc["n_occupied"], occ.sum(axis=0)) and np.array_equal(acc["n_below"], ref["below"].sum(axis=0)) and np.array_equal(acc["n_above"], ref["above"].sum(axis=0))
    seen = occ.any(axis=0)
    assert np.array_equal(acc["min_operative"][seen], np.where(occ, top, np.inf).min(axis=0)[seen])
    assert np.array_equal(acc["step_min"][seen], np.where(occ, top, np.inf).argmin(axis=0)[seen])      # (argmin: the first occurrence)
    assert np.array_equal(acc["step_max"][seen], np.where(occ, top, -np.inf).argmax(axis=0)[seen]) and np.all(acc["step_min"][~seen] == -1)
    # the sensor without entries has r = 0.0, the controlled zones sense their sensor's operative temperature, the others their air
    assert np.all(ref["mrt"][:, cc.EMPTY] == 0.0) and np.all(ref["mrt"][:, cc.LONG] != 0.0)
    ctl = np.flatnonzero(c.comfort["control"] == 1)
    plain = np.setdiff1d(np.arange(md["n_zones"]), c.comfort["zone"][ctl])
    assert len(plain) and np.array_equal(ref["Tc"][:, c.comfort["zone"][ctl]], top[:, ctl])
    # the feedback arm: sensing the operative temperature, thermostats, air paths and blinds decide differently than sensing air
    state = st.copy()
    march(state, -1, None, None)
    air = cc.loop(c, state, march, md["zone_slot"], sense="air")
    assert np.array_equal(air["operative"], top) and np.array_equal(air["Tc"][:, plain], ref["Tc"][:, plain])   # (the synthetic march has no feedback)
    differ = {k: int((ref[k] != air[k]).sum()) for k in ("applied", "path_q", "position")}
    assert all(v > 0 for v in differ.values()), differ
    assert not np.array_equal(ref["carry"]["modes"], air["carry"]["modes"]) or differ["applied"] > 0
    # a cut with resume reproduces the uncut accumulators, and every other carried state
    state = st.copy()
    march(state, -1, None, None)
    first = cc.loop(c, state, march, md["zone_slot"], steps=range(0, 9))
    second = cc.loop(c, state, march, md["zone_slot"], steps=range(9, c.n_steps), carry=first["carry"])
    assert all(np.array_equal(second["carry"]["comfort"][k], acc[k]) for k in cf.ACC)
    assert np.array_equal(np.concatenate([first["operative"], second["operative"]]), top)
    assert np.array_equal(second["carry"]["modes"], ref["carry"]["modes"]) and np.array_equal(second["carry"]["air"]["state"], ref["carry"]["air"]["state"])
    # heat_comfort_check accepts the case, also with one sensor
    binding.comfort_check(md, c.comfort, weather=np.zeros((c.n_steps, 1, 3)), n_sub=1, channel=c.channel)
    one = cc.comfort_case(md, st, np.random.default_rng(seed), n_sensors=1)
    assert cf.n_sensors(one.comfort) == 1 and one.comfort["control"][0] == 1
    binding.comfort_check(md, one.comfort, weather=np.zeros((c.n_steps, 1, 3)), n_sub=1, channel=one.channel)


def test_every_decision_of_the_oracle_case_is_away_from_a_tie(oracle):
    """The case tests/test_comfort_gpu.py compares with the oracle loop: every comparison of that loop — limits, extrema,
    thermostats, vents, blinds — is further from a tie than MARGIN, so that device and oracle, 1e-9 apart, decide alike."""
    c, w, probes, a0, b0 = cc.oracle_case()
    ref, state = cc.oracle_loop(oracle, c, w, probes, a0, b0)
    print("margins of the oracle loop: %s" % ref["margin"])
    assert set(ref["margin"]) == {"limit", "extremum", "thermostat", "air", "I", "T"}
    assert all(v > MARGIN for v in ref["margin"].values()), ref["margin"]
    cov = cc.coverage(c, ref)
    assert cov["occupied"] > 0 and cov["unoccupied"] > 0 and cov["below"] > 0 and cov["above"] > 0 and cov["inside"] > 0, cov
    assert ref["applied"].any() and ref["carry"]["air"]["switches"].any() and ref["carry"]["blinds"]["switches"].any()


def test_comfort_check_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "comfort_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "comfort host check: all statuses as the header states them" in out.stdout
