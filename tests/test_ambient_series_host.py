"""Ambient-side temperatures after creation, on the host (include/heat_amd.h: heat_batch_set_ambient, heat_ambient_drive /
heat_ambient_check / heat_batch_march_series_ambient; heat_amd/ambient.py): the entry points are declared, exported and bound;
the ctypes mirror has the header's layout; the rule in numpy (ambient.apply — the reference of
tests/test_ambient_series_gpu.py) gives the hand-worked cases; every refusal the header lists comes back with its code and
names the ambient side, before any device work; the cases of the GPU tests cover what they promise, and the oracle alone tells
a driven side from an undriven one in every one of them. heat_ambient_check and the table builder (the layout against a
device order, the peer record of a wall that is Ambient on both sides, the sentinel elsewhere) also run under
AddressSanitizer / UBSan as a stand-alone program (tests/ambient_host_main.cpp) in a child process. No GPU needed.

Reference: the rule is this project's own (the reference fixes its boundaries when the model is built)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ambient_cases as ac
from heat_amd import ambient as amb, binding, modeldict as mdl
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_batch_set_ambient", "heat_ambient_check", "heat_batch_march_series_ambient")
E_INVALID_ARG, E_SIZE = -1, -4
N_STEPS = 4
FIELDS = ("n_sides", "surface", "side", "chan", "gain", "offset", "mix_zone", "mix", "sum_temperature")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_ambient_drive {" in header
    assert "heat_ambient_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_ambient" not in binding.HOST_ONLY_SYMBOLS and "heat_batch_set_ambient" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("AmbientDrive", "make_ambient", "ambient_check"))
    assert hasattr(binding.HeatBatch, "set_ambient") and all(hasattr(amb, n) for n in ("apply", "b_factor"))
    assert L.heat_amd_abi_version() == 1 and re.search(r"#define\s+HEAT_AMD_ABI_VERSION\s+1\b", header)
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW) and "pub struct HeatAmbientDrive" in rust


def test_ambient_drive_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = ["sizeof(heat_ambient_drive)", "sizeof(heat_series)", "sizeof(heat_room_radiation)"] + ["offsetof(heat_ambient_drive, %s)" % f for f in FIELDS]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == ([C.sizeof(binding.AmbientDrive), C.sizeof(binding.Series), C.sizeof(binding.RoomRadiation)] +
                   [getattr(binding.AmbientDrive, f).offset for f in FIELDS])
    assert [f for f, _ in binding.AmbientDrive._fields_] == list(FIELDS) and got[0] == 8 * len(FIELDS)


# ---- the rule in numpy: hand-worked cases ----
def test_gain_only_and_offset_only():
    row = np.array([10.0, -4.0, 0.1])
    assert np.array_equal(amb.apply(dict(chan=[0, 1, 2, 0]), row, None), [10.0, -4.0, 0.1, 10.0])
    assert np.array_equal(amb.apply(dict(chan=[0, 1, 2], gain=[0.5, 2.0, 3.0]), row, None), [5.0, -8.0, 3.0 * 0.1])
    assert np.array_equal(amb.apply(dict(chan=[0, 1, 2], offset=[0.25, 4.0, 0.2]), row, None), [10.25, 0.0, 0.1 + 0.2])
    # gain before offset, each rounded: 3 * 0.1 = 0.30000000000000004, then + 0.2
    v = amb.apply(dict(chan=[2], gain=[3.0], offset=[0.2]), row, None)
    assert v[0] == (3.0 * 0.1) + 0.2
    # ... and not fused: (1 + 2^-30)^2 = 1 + 2^-29 + 2^-60 rounds to 1 + 2^-29 before the offset takes the 1 away
    e = 1.0 + 2.0 ** -30
    v = amb.apply(dict(chan=[0], gain=[e], offset=[-1.0]), np.array([e]), None)
    assert v[0] == 2.0 ** -29 and v[0] != 2.0 ** -29 + 2.0 ** -60
    # a NULL offset is no operation at all: -0.0 stays -0.0, where + 0.0 would give +0.0
    assert np.signbit(amb.apply(dict(chan=[0]), np.array([-0.0]), None)[0])
    assert not np.signbit(amb.apply(dict(chan=[0], offset=[0.0]), np.array([-0.0]), None)[0])


def test_mix_with_b_of_zero_a_half_and_one():
    """T_u = T_out + (1 - b) (T_zone - T_out): outside at 4, the zone at 20."""
    row, zones = np.array([4.0]), np.array([99.0, 20.0])
    b = np.array([0.0, 0.5, 1.0])
    mix = amb.b_factor(b)
    assert np.array_equal(mix, [1.0, 0.5, 0.0])
    v = amb.apply(dict(chan=[0, 0, 0], mix_zone=[1, 1, 1], mix=mix), row, zones)
    assert np.array_equal(v, [20.0, 12.0, 4.0])
    # -1: no mixing, and mix is not read there; the order of the three operations, each rounded
    v = amb.apply(dict(chan=[0, 0], mix_zone=[-1, 0], mix=[np.nan, 0.1]), np.array([0.3]), np.array([0.7]))
    d = 0.7 - 0.3
    m = 0.1 * d
    assert v[0] == 0.3 and v[1] == 0.3 + m
    # gain and offset come first: the mix sees the shifted value
    v = amb.apply(dict(chan=[0], gain=[2.0], offset=[1.0], mix_zone=[0], mix=[0.25]), np.array([3.0]), np.array([15.0]))
    assert v[0] == 7.0 + 0.25 * (15.0 - 7.0)


def test_a_nan_channel_propagates():
    row = np.array([np.nan, 5.0])
    v = amb.apply(dict(chan=[0, 1, 0], gain=[1.0, 1.0, 0.0], offset=[0.0, 1.0, 3.0], mix_zone=[-1, -1, 0], mix=[0.0, 0.0, 0.0]), row, np.array([20.0]))
    assert np.isnan(v[0]) and v[1] == 6.0 and np.isnan(v[2])
    v = amb.apply(dict(chan=[1], mix_zone=[0], mix=[0.5]), row, np.array([np.nan]))            # a NaN zone as well
    assert np.isnan(v[0])


# ---- heat_ambient_check ----
@pytest.fixture(scope="module")
def model():
    md, st = mdl.clustered_massive(120, Z=6, seed=5)
    md["back_kind"] = np.where(np.arange(120) % 3 == 0, mdl.AMBIENT, md["back_kind"]).astype(np.int32)
    return md


def series(md, **more):
    kw = dict(weather=np.zeros((N_STEPS, 2, 3)), n_sub=2, channel=np.zeros((N_STEPS, 4)))
    kw.update(more)
    return kw


def good_drive(md):
    fronts, backs = np.flatnonzero(md["front_kind"] == mdl.AMBIENT), np.flatnonzero(md["back_kind"] == mdl.AMBIENT)
    assert len(fronts) >= 8 and len(backs) >= 8 and len(np.intersect1d(fronts, backs))
    surface = np.concatenate([backs, fronts])
    side = np.concatenate([np.ones(len(backs), np.uint8), np.zeros(len(fronts), np.uint8)])
    N = len(surface)
    mix_zone = np.where(np.arange(N) % 3 == 0, np.arange(N) % 6, -1)
    return dict(surface=surface, side=side, chan=np.arange(N) % 4, gain=np.full(N, 0.9), offset=np.full(N, 1.5), mix_zone=mix_zone,
                mix=np.where(mix_zone >= 0, 0.4, np.nan))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def check(md, drive, **more):
    binding.ambient_check(md, drive, **series(md, **more))


def _raw(md, drive, **fields):
    """heat_ambient_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**series(md))
    a, akeep = binding.make_ambient(**drive)
    for name, v in fields.items():
        setattr(a, name, v)
    rc_ = L.heat_ambient_check(C.byref(desc), 1, C.byref(s), C.byref(a))
    return rc_, L.heat_last_error().decode()


def test_good_empty_and_absent_drives_and_the_null_forms_are_accepted(model):
    g = good_drive(model)
    check(model, g)
    check(model, None)
    check(model, {})
    check(model, dict(g, sum_temperature=np.arange(float(len(g["surface"])))))
    check(model, dict(g, sum_temperature=False))
    for gone in (("gain",), ("offset",), ("gain", "offset"), ("mix_zone", "mix"), ("gain", "offset", "mix_zone", "mix")):
        check(model, {k: v for k, v in g.items() if k not in gone})
    check(model, dict({k: v for k, v in g.items() if k != "mix"}, mix_zone=np.full(len(g["surface"]), -1)))   # mix NULL: nobody mixes
    binding.ambient_check(model, g, n_sites=3, **series(model, weather=np.zeros((N_STEPS, 2, 3, 3))))          # sites need nothing
    # the series' own refusals come first
    code, msg = _code(lambda: check(model, g, solar_front=np.full(int(model["n_surfaces"]), 5, np.int32)))
    assert code == E_SIZE and "surface 0" in msg, msg


def test_negative_counts_and_null_arrays_are_invalid_arguments(model):
    g = good_drive(model)
    rc_, msg = _raw(model, g, n_sides=-1)
    assert rc_ == E_INVALID_ARG and "ambient side" in msg, msg
    for field in ("surface", "side", "chan"):
        rc_, msg = _raw(model, g, **{field: None})
        assert rc_ == E_INVALID_ARG and "ambient side 0" in msg and field in msg, (field, msg)
    for field in ("gain", "offset", "mix_zone", "sum_temperature"):
        assert _raw(model, g, **{field: None})[0] == 0, field                                       # nullable
    first = int(np.flatnonzero(g["mix_zone"] >= 0)[0])
    rc_, msg = _raw(model, g, mix=None)                                                             # ... with mixing sides present
    assert rc_ == E_INVALID_ARG and "ambient side %d:" % first in msg and "mix" in msg, msg


def test_side_bytes_and_values_that_are_not_finite_are_invalid_arguments(model):
    g = good_drive(model)
    N = len(g["surface"])
    i = np.arange(N)
    code, msg = _code(lambda: check(model, dict(g, side=np.where(i == 5, 2, g["side"]))))
    assert code == E_INVALID_ARG and "ambient side 5:" in msg, msg
    for field, at, bad in (("gain", 2, np.inf), ("gain", 7, np.nan), ("offset", 4, -np.inf), ("offset", 1, np.nan), ("mix", 3, np.nan),
                           ("mix", 6, np.inf)):
        assert field != "mix" or g["mix_zone"][at] >= 0
        code, msg = _code(lambda: check(model, dict(g, **{field: np.where(i == at, bad, g[field])})))
        assert code == E_INVALID_ARG and "ambient side %d:" % at in msg and field in msg, (field, msg)


def test_numbers_out_of_range_sides_that_are_not_ambient_and_duplicates_are_size_errors(model):
    g = good_drive(model)
    S, Z, N = int(model["n_surfaces"]), int(model["n_zones"]), len(g["surface"])
    i = np.arange(N)
    for bad in (S, -1, S + 1000):
        code, msg = _code(lambda: check(model, dict(g, surface=np.where(i == 9, bad, g["surface"]))))
        assert code == E_SIZE and "ambient side 9:" in msg, msg
    space = int(np.flatnonzero(model["back_kind"] == mdl.SPACE)[0])
    outdoor = int(np.flatnonzero(model["front_kind"] == mdl.OUTDOOR)[0])
    for q, sd in ((space, 1), (outdoor, 0)):
        code, msg = _code(lambda: check(model, dict(g, surface=np.where(i == 4, q, g["surface"]), side=np.where(i == 4, sd, g["side"]))))
        assert code == E_SIZE and "ambient side 4:" in msg and "HEAT_BOUNDARY_AMBIENT" in msg, msg
    for bad in (4, -1):
        code, msg = _code(lambda: check(model, dict(g, chan=np.where(i == 8, bad, g["chan"]))))
        assert code == E_SIZE and "ambient side 8:" in msg and "channel" in msg, msg
    for bad in (Z, -2):
        code, msg = _code(lambda: check(model, dict(g, mix_zone=np.where(i == 6, bad, g["mix_zone"]), mix=np.full(N, 0.5))))
        assert code == E_SIZE and "ambient side 6:" in msg and "mix_zone" in msg, msg
    code, msg = _code(lambda: check(model, dict(g, surface=np.where(i == 11, g["surface"][2], g["surface"]),
                                                side=np.where(i == 11, g["side"][2], g["side"]))))
    assert code == E_SIZE and "ambient side 11:" in msg and "ambient side 2" in msg, msg
    # both sides of one wall are two sides, not one twice
    both = int(np.intersect1d(g["surface"][g["side"] == 0], g["surface"][g["side"] == 1])[0])
    check(model, dict(surface=[both, both], side=[0, 1], chan=[0, 1]))


def test_march_and_setter_without_a_batch_are_invalid_arguments(model):
    L = binding.load_library()
    s, keep = binding.make_series(**series(model))
    a, akeep = binding.make_ambient(**good_drive(model))
    failed = C.c_int32(7)
    assert L.heat_batch_march_series_ambient(None, C.byref(s), *(None,) * 15, C.byref(a), None, C.byref(failed)) == E_INVALID_ARG
    assert failed.value == -1
    assert L.heat_batch_set_ambient(None, 0, None, None, None) == E_INVALID_ARG


def test_the_wrapper_reads_the_shapes(model):
    g = good_drive(model)
    for field in ("side", "chan", "gain", "offset", "mix_zone", "mix", "sum_temperature"):
        with pytest.raises(ValueError) as e:
            binding.make_ambient(**dict(g, **{field: np.zeros(3)}))
        assert field in str(e.value)
    a, keep = binding.make_ambient(**g)
    assert a.n_sides == len(g["surface"]) and keep["sum_temperature"].shape == (a.n_sides,) and not keep["sum_temperature"].any()
    a, keep = binding.make_ambient()
    assert a.n_sides == 0 and not a.surface and not a.sum_temperature


# ---- the cases of the GPU tests ----
@pytest.mark.parametrize("name", sorted(ac.FAMILIES))
def test_the_cases_cover_what_they_promise_and_the_oracle_discriminates(oracle, name):
    c = ac.case(name)
    md = c.md
    assert 5 <= c.n_steps <= 7 and 2 <= c.n_sub <= 7
    assert {int(k) for k in md["front_kind"][c.conv]} == {mdl.SPACE, mdl.AMBIENT, mdl.OUTDOOR}
    fk, bk = md["front_kind"][c.surface], md["back_kind"][c.surface]
    assert np.all(np.where(c.side == 0, fk, bk) == mdl.AMBIENT)
    assert len(set(zip(c.surface.tolist(), c.side.tolist()))) == len(c.surface)
    n_ambient = int((md["front_kind"] == mdl.AMBIENT).sum() + (md["back_kind"] == mdl.AMBIENT).sum())
    assert len(c.surface) < n_ambient                                       # some Ambient sides are left alone
    assert (c.both & (c.side == 0)).sum() > 10 and (c.both & (c.side == 1)).sum() > 10
    moved = np.abs(c.set_values - c.descriptor)
    assert moved.min() >= 5.0 and moved.max() <= 15.0
    d = c.drive
    assert (d["gain"] == 1.0).any() and (d["gain"] != 1.0).any() and (d["offset"] == 0.0).any() and (d["offset"] != 0.0).any()
    mz = d["mix_zone"]
    assert ((mz >= 0) & (mz == c.own_zone)).any() and ((mz >= 0) & (mz == c.far) & (c.far != c.home)).any() and (mz < 0).any()
    assert np.all(np.isnan(d["mix"][mz < 0])) and np.all(np.isfinite(d["mix"][mz >= 0]))
    if c.cluster:
        assert ((mz >= 0) & (mz // c.cluster != c.home // c.cluster)).any()
    binding.ambient_check(md, d, weather=c.weather, n_sub=c.n_sub, **ac.series_kwargs(c))
    ref, iters, sides, walls = ac.discrimination(oracle, c)
    assert np.all(np.isfinite(ref)) and sides.all() and len(walls) > 10 and walls.all(), (int((~sides).sum()), int((~walls).sum()))
    v = amb.apply(d, c.channel[0], c.state[md["zone_slot"]])
    assert v.shape == (len(c.surface),) and np.all(np.isfinite(v))


def test_ambient_check_and_tables_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "ambient_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ambient host check: all statuses as the header states them" in out.stdout
