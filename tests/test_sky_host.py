"""Sky of a series on the host (include/heat_amd.h, heat_sky / heat_sky_check / heat_batch_march_series_sky; heat_amd/sky.py):
the entry points are declared, exported and bound; the ctypes mirrors have the header's layout; the rule in numpy
(sky.incident — the reference of tests/test_sky_gpu.py) gives the closed forms of a roof, walls and a soffit; every refusal
the header lists comes back with its code and names the surface, before any device work; valid skies are accepted.
heat_sky_check also runs under AddressSanitizer / UBSan in a child process, like tests/test_ideal_loads_host.py. No GPU needed.

Reference: the rule is this project's own (the reference's harness reads EnergyPlus' incident irradiance from CSV,
validate_wall_heat_transfer.rs:675-705)."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from heat_amd import binding, build as hb, modeldict as mdl, sky

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_sky_check", "heat_batch_march_series_sky")
E_INVALID_ARG, E_SIZE = -1, -4
N_STEPS, N_CHANNELS = 4, 6
RECORD_FIELDS = ("sun_x", "sun_y", "sun_z", "beam", "diffuse", "ground", "ir_sky", "ir_ground")
SKY_FIELDS = ("record", "normal_x", "normal_y", "normal_z", "mode")


def _asan_runtime():
    out = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return out if os.path.isabs(out) and os.path.exists(out) else None


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_sky_record {" in header and "typedef struct heat_sky {" in header
    assert "heat_sky_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_sky" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("SkyRecord", "Sky", "make_sky", "sky_check"))
    assert sky.FIELDS == RECORD_FIELDS
    assert L.heat_amd_abi_version() == 1


def test_sky_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = (["sizeof(heat_sky_record)", "sizeof(heat_sky)", "sizeof(heat_series)", "sizeof(heat_zone_loads)", "sizeof(heat_series_report)",
             "sizeof(heat_ideal_loads)"] + ["offsetof(heat_sky_record, %s)" % f for f in RECORD_FIELDS] +
            ["offsetof(heat_sky, %s)" % f for f in SKY_FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == 64 and C.sizeof(binding.SkyRecord) == 64
    # (the structs beside them keep their sizes: the sky is a struct of its own)
    assert got == ([64, C.sizeof(binding.Sky), C.sizeof(binding.Series), C.sizeof(binding.ZoneLoads), C.sizeof(binding.Report),
                    C.sizeof(binding.IdealLoads)] + [getattr(binding.SkyRecord, f).offset for f in RECORD_FIELDS] +
                   [getattr(binding.Sky, f).offset for f in SKY_FIELDS])
    assert [getattr(binding.SkyRecord, f).offset for f in RECORD_FIELDS] == [8 * i for i in range(8)]


# ---- the rule in numpy: closed forms ----
BEAM, DIFFUSE, GROUND, IR_SKY, IR_GROUND = 800.0, 120.0, 45.0, 350.0, 420.0


def record(sun, beam=BEAM):
    return np.array([sun[0], sun[1], sun[2], beam, DIFFUSE, GROUND, IR_SKY, IR_GROUND])


def test_roof_under_a_sun_at_the_zenith():
    r = record((0.0, 0.0, 1.0))
    assert sky.incident(r, (0.0, 0.0, 1.0), "solar_front") == BEAM + DIFFUSE
    assert sky.incident(r, (0.0, 0.0, 1.0), "ir_front") == IR_SKY


def test_vertical_walls_facing_and_opposite_a_sun_at_30_degrees():
    el = math.radians(30.0)
    r = record((0.0, -math.cos(el), math.sin(el)))      # in the south, 30 degrees up
    facing = sky.incident(r, (0.0, -1.0, 0.0), "solar_front")
    assert abs(facing - (BEAM * math.cos(el) + DIFFUSE / 2 + GROUND / 2)) <= 1e-15 * facing
    assert sky.incident(r, (0.0, 1.0, 0.0), "solar_front") == DIFFUSE / 2 + GROUND / 2
    assert sky.incident(r, (0.0, -1.0, 0.0), "solar_back") == DIFFUSE / 2 + GROUND / 2   # the back of the facing wall looks north
    assert sky.incident(r, (0.0, 1.0, 0.0), "ir_front") == IR_SKY / 2 + IR_GROUND / 2


def test_soffit_and_the_back_of_a_roof():
    r = record((0.3, -0.5, math.sqrt(1 - 0.09 - 0.25)))
    for kind, want in (("solar", GROUND), ("ir", IR_GROUND)):
        soffit = sky.incident(r, (0.0, 0.0, -1.0), kind + "_front")
        assert soffit == want
        assert sky.incident(r, (0.0, 0.0, 1.0), kind + "_back") == soffit


def test_a_sun_below_the_horizon_adds_nothing_to_a_roof():
    r = record((0.6, 0.0, -0.8))
    assert r[3] > 0 and sky.incident(r, (0.0, 0.0, 1.0), "solar_front") == DIFFUSE
    assert sky.incident(record((0.0, 0.0, 1.0), beam=0.0), (0.0, 0.0, 1.0), "solar_front") == DIFFUSE   # and a night


def test_the_rule_broadcasts_and_a_nan_cosine_is_no_beam():
    rec = np.stack([record((0.0, 0.0, 1.0)), record((1.0, 0.0, 0.0))])                 # [2, 8]
    n = (np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, -1.0]))
    got = sky.incident(rec[:, None, :], n, "solar_front")                                # [2 steps, 3 surfaces]
    assert got.shape == (2, 3)
    assert np.array_equal(got, [[BEAM + DIFFUSE, DIFFUSE / 2 + GROUND / 2, GROUND], [DIFFUSE, BEAM + DIFFUSE / 2 + GROUND / 2, GROUND]])
    bad = record((np.nan, 0.0, 1.0))
    assert sky.incident(bad, (0.0, 0.0, 1.0), "solar_front") == DIFFUSE                # c is NaN: c > 0 is false
    with pytest.raises(ValueError):
        sky.incident(bad, (0.0, 0.0, 1.0), "front")


def test_sun_direction_is_a_unit_vector_that_rises_in_the_east():
    lat = math.radians(48.0)
    d = sky.sun_direction(172, np.arange(24.0), lat)
    assert d.shape == (24, 3) and np.allclose(np.linalg.norm(d, axis=1), 1.0)
    assert d[12, 2] == d[:, 2].max() and abs(d[12, 0]) < 1e-12 and d[12, 1] < 0       # noon: highest, due south
    assert abs(math.degrees(math.asin(d[12, 2])) - (90.0 - 48.0 + 23.45)) < 0.1
    assert d[8, 0] > 0 > d[16, 0] and d[0, 2] < 0                                      # morning east, evening west, midnight below


# ---- heat_sky_check ----
@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


def series(md, **more):
    S = int(md["n_surfaces"])
    chan = np.full(S, -1, np.int32)
    return dict(dict(weather=np.zeros((N_STEPS, 2, 3)), n_sub=2, channel=np.zeros((N_STEPS, N_CHANNELS)), solar_front=chan, ir_back=chan), **more)


def good_sky(md, n_sites=1):
    S = int(md["n_surfaces"])
    rng = np.random.default_rng(1)
    return dict(record=rng.random((N_STEPS, n_sites, 8)), mode=(np.arange(S) % 16).astype(np.uint8),
                normals=tuple(rng.normal(size=(3, S))))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def _raw(md, sky_args, series_args=None, **fields):
    """heat_sky_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**(series_args or series(md)))
    k, kkeep = binding.make_sky(**sky_args)
    for name, v in fields.items():
        setattr(k, name, v)
    rc = L.heat_sky_check(C.byref(desc), 1, C.byref(s), C.byref(k))
    return rc, L.heat_last_error().decode()


def test_good_empty_and_absent_skies_are_accepted(model):
    S = int(model["n_surfaces"])
    binding.sky_check(model, good_sky(model), **series(model))
    binding.sky_check(model, dict(good_sky(model), normals=None), **series(model))                 # the model's own normals
    binding.sky_check(model, good_sky(model, 3), n_sites=3, **series(model, weather=np.zeros((N_STEPS, 2, 3, 3))))
    # an all-zero mode needs nothing else; n_steps == 0 needs no records
    assert _raw(model, dict(record=None, mode=np.zeros(S, np.uint8)))[0] == 0
    assert _raw(model, dict(good_sky(model), record=None), series(model, weather=np.zeros((0, 3)), channel=None))[0] == 0
    L = binding.load_library()
    desc, keep = binding.make_desc(model)
    s, skeep = binding.make_series(**series(model))
    assert L.heat_sky_check(C.byref(desc), 1, C.byref(s), None) == 0                               # sky == NULL is no sky
    assert L.heat_sky_check(C.byref(desc), 1, None, None) == E_INVALID_ARG
    assert L.heat_sky_check(None, 1, C.byref(s), None) == E_INVALID_ARG
    # the series' own refusals come first
    code, msg = _code(lambda: binding.sky_check(model, good_sky(model), **series(model, solar_front=np.full(S, N_CHANNELS, np.int32))))
    assert code == E_SIZE and "surface 0" in msg, msg


def test_null_arrays_are_invalid_arguments(model):
    S = int(model["n_surfaces"])
    rc, msg = _raw(model, good_sky(model), mode=None)
    assert rc == E_INVALID_ARG and "mode is NULL" in msg and "surface" in msg, msg
    first = 1                                                                                       # (mode[0] == 0)
    for field in ("normal_x", "normal_y", "normal_z", "record"):
        rc, msg = _raw(model, good_sky(model), **{field: None})
        assert rc == E_INVALID_ARG and "surface %d:" % first in msg and field in msg, (field, msg)
        one = np.zeros(S, np.uint8)
        one[137] = 8
        rc, msg = _raw(model, dict(good_sky(model), mode=one), **{field: None})
        assert rc == E_INVALID_ARG and "surface 137:" in msg, (field, msg)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_normal_that_is_not_finite_is_refused_where_the_sky_is_used(model, axis, bad):
    g = good_sky(model)
    normals = [a.copy() for a in g["normals"]]
    normals[axis][53] = bad
    code, msg = _code(lambda: binding.sky_check(model, dict(g, normals=normals), **series(model)))
    assert code == E_INVALID_ARG and "surface 53:" in msg and "normal_" + "xyz"[axis] in msg, msg
    normals[axis][53] = 0.25
    normals[axis][48] = bad                                                                         # mode 48 % 16 == 0: not read
    binding.sky_check(model, dict(g, normals=normals), **series(model))


@pytest.mark.parametrize("bad", [16, 17, 128, 255])
def test_a_mode_byte_above_15_is_refused(model, bad):
    g = good_sky(model)
    mode = g["mode"].copy()
    mode[77] = bad
    code, msg = _code(lambda: binding.sky_check(model, dict(g, mode=mode), **series(model)))
    assert code == E_INVALID_ARG and "surface 77:" in msg, msg


@pytest.mark.parametrize("bit,name", enumerate(["solar_front", "solar_back", "ir_front", "ir_back"]))
def test_an_input_has_one_source(model, bit, name):
    S = int(model["n_surfaces"])
    chan = np.full(S, -1, np.int32)
    where = 16 * 5 + (1 << bit)                                                                     # mode = exactly this bit
    chan[where] = 2
    code, msg = _code(lambda: binding.sky_check(model, good_sky(model), **series(model, **{name: chan})))
    assert code == E_SIZE and "surface %d:" % where in msg and "channel 2" in msg, msg
    chan[where], chan[16 * 5] = -1, 2                                                               # mode 0 there: the channel is alone
    binding.sky_check(model, good_sky(model), **series(model, **{name: chan}))


def test_an_own_face_bit_on_a_sky_driven_side_is_refused_by_the_series(model):
    S = int(model["n_surfaces"])
    own = np.zeros(S, np.uint8)
    own[4] = 1                                                                                      # mode 4: long-wave front from the sky
    code, msg = _code(lambda: binding.sky_check(model, good_sky(model), **series(model, ir_own_face=own)))
    assert code == E_SIZE and "surface 4:" in msg, msg


def test_march_refuses_before_any_device_work(model):
    """What heat_batch_march_series_sky can answer without a batch: the same with or without a device."""
    L = binding.load_library()
    s, _ = binding.make_series(**series(model))
    k, _ = binding.make_sky(**good_sky(model))
    failed = C.c_int32(123)
    assert L.heat_batch_march_series_sky(None, C.byref(s), C.byref(k), None, None, None, None, None, None, C.byref(failed)) == E_INVALID_ARG
    assert failed.value == -1
    assert L.heat_batch_march_series_sky(None, None, None, None, None, None, None, None, None, None) == E_INVALID_ARG


def test_the_wrapper_reads_the_shapes(model):
    S = int(model["n_surfaces"])
    k, keep = binding.make_sky(**good_sky(model))
    assert keep["record"].shape == (N_STEPS, 1, 8) and keep["mode"].dtype == np.uint8 and keep["normal_z"].shape == (S,)
    k, keep = binding.make_sky(np.zeros((N_STEPS, 8)), np.zeros(S))                                 # one site: [n_steps, 8]
    assert not k.normal_x and keep["record"].shape == (N_STEPS, 8)
    for bad in (lambda: binding.make_sky(np.zeros((N_STEPS, 7)), np.zeros(S)),
                lambda: binding.sky_check(model, dict(good_sky(model), mode=np.zeros(S - 1)), **series(model)),
                lambda: binding.sky_check(model, dict(good_sky(model), record=np.zeros((N_STEPS + 1, 1, 8))), **series(model)),
                lambda: binding.sky_check(model, good_sky(model, 2), **series(model)),
                lambda: binding.sky_check(model, dict(good_sky(model), normals=(np.zeros(S), np.zeros(S), np.zeros(3))), **series(model))):
        with pytest.raises(ValueError):
            bad()


def test_sky_check_under_address_and_ub_sanitizers():
    asan = _asan_runtime()
    if asan is None:
        pytest.skip("gcc has no libasan here")
    lib = hb.build_plan_host()
    env = dict(os.environ)
    env["LD_PRELOAD"] = asan
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sky_host_worker.py"), lib], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-6000:])
    assert "sky host check" in out.stdout
