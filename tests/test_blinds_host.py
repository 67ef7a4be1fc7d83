"""Blinds of a series on the host (include/heat_amd.h, heat_blinds / heat_blinds_check / heat_batch_march_series_blinds;
heat_amd/blinds.py): the entry points are declared, exported and bound; the ctypes mirror has the header's layout; the rule in
numpy (blinds.incident_on and blinds.apply — the reference of tests/test_blinds_gpu.py) gives the hand-worked cases; every
refusal the header lists comes back with its code and names the blind, before any device work; the case builder of the GPU
tests takes every branch of the rule on synthetic zone temperatures. heat_blinds_check also runs under AddressSanitizer / UBSan
as a stand-alone program (tests/blinds_host_main.cpp) in a child process. No GPU needed.

Reference: the rule is this project's own (the reference has no solar geometry, let alone one that moves)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from heat_amd import binding, blinds as bl, modeldict as mdl, sky, solar_gains
import blinds_cases as bc
import shades_cases as sc
from test_shades_host import good_gains, good_shades, good_sky, series
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_blinds_check", "heat_batch_march_series_blinds")
E_INVALID_ARG, E_SIZE = -1, -4
FIELDS = ("n_blinds", "shade", "beam_closed", "diffuse_closed", "ground_closed", "pos_chan", "irr_close", "irr_open", "zone", "set_chan",
          "band", "enable_chan", "state", "steps_closed", "switches", "sum_position")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_blinds {" in header
    assert "heat_blinds_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_blinds" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("Blinds", "make_blinds", "blinds_check"))
    assert all(hasattr(bl, n) for n in ("incident_on", "apply"))
    assert L.heat_amd_abi_version() == 1
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW) and "pub struct HeatBlinds" in rust
    # the widest entry point is the last row of the binding's table, and carries every term
    symbol, carried = binding.HeatBatch._SERIES_ENTRY[-1]
    assert symbol == "heat_batch_march_series_blinds" and carried[-1] == "blinds" and set(carried) == set(binding.HeatBatch._SERIES_TERMS) | {"report", "sky"}
    assert binding.HeatBatch._SERIES_ORDER[-3:] == ("blinds", "position", "blind_incident")
    # the header states the scope
    assert "venetian" in header and "long-wave exchange or convection" in header


def test_blinds_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = ["sizeof(heat_blinds)", "sizeof(heat_shades)", "sizeof(heat_ambient_drive)"] + ["offsetof(heat_blinds, %s)" % f for f in FIELDS]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    # (the structs beside it keep their sizes: the blinds are a struct of their own)
    assert got == ([C.sizeof(binding.Blinds), C.sizeof(binding.Shades), C.sizeof(binding.AmbientDrive)] +
                   [getattr(binding.Blinds, f).offset for f in FIELDS])
    assert [f for f, _ in binding.Blinds._fields_] == list(FIELDS)
    assert got[0] == 8 * len(FIELDS) and got[1] == 8 * 27


# ---- the rule in numpy: hand-worked cases ----
SOUTH = dict(surface=[0], normal=(np.array([0.0]), np.array([-1.0]), np.array([0.0])))


def record(beam, diffuse=100.0, ground=40.0, sun=(0.0, -0.6, 0.8)):
    return np.array([[sun[0], sun[1], sun[2], beam, diffuse, ground, 350.0, 420.0]])


def one_blind(**more):
    return dict(dict(shade=[0], beam_closed=[0.1], diffuse_closed=[0.3], ground_closed=[0.5], irr_close=[300.0], irr_open=[150.0]), **more)


def step(I, blinds, state, T=(), row=(), f=0.75, shades=SOUTH):
    return bl.apply(np.array([I], dtype=np.float64), np.array(T, dtype=np.float64), np.array(row, dtype=np.float64), blinds, state,
                    np.array([f]), shades)


def test_the_irradiance_on_the_shades_plane():
    # a south wall, the sun at (0, -0.6, 0.8): c = 0.6; a wall sees half the sky and half the ground
    I = bl.incident_on(SOUTH, record(500.0), np.array([0.75]))
    assert I.shape == (1,) and I[0] == (500.0 * 0.6 * 0.75 + 100.0 * 0.5) + 40.0 * 0.5
    shaded = dict(SOUTH, diffuse_factor=[0.5], ground_factor=[0.25])
    assert bl.incident_on(shaded, record(500.0), np.array([0.75]))[0] == (500.0 * 0.6 * 0.75 + (100.0 * 0.5) * 0.5) + (40.0 * 0.5) * 0.25
    # the sun behind the plane, and a NaN sun: no beam
    assert bl.incident_on(SOUTH, record(500.0, sun=(0.0, 0.6, 0.8)), np.array([0.0]))[0] == 70.0
    assert bl.incident_on(SOUTH, record(500.0, sun=(np.nan, -0.6, 0.8)), np.array([0.0]))[0] == 70.0
    # ... it is what sky.incident gives an unblinded side in that plane, to the bit; a series of steps, shades at two sites
    rng = np.random.default_rng(3)
    n, k = 40, 9
    normal = tuple(rng.normal(size=(3, n)))
    shades = dict(surface=rng.integers(0, 12, n), normal=normal, diffuse_factor=rng.uniform(0.5, 1, n), ground_factor=rng.uniform(0.3, 1, n))
    site = rng.integers(0, 2, 12)
    rec = np.concatenate([rng.normal(size=(k, 2, 3)), rng.uniform(0, 900, (k, 2, 1)), rng.uniform(-50, 300, (k, 2, 4))], axis=2)
    f = rng.random((k, n))
    want = sky.incident(rec[:, site[shades["surface"]], :], normal, "solar_front", shade=(f, shades["diffuse_factor"], shades["ground_factor"]))
    assert np.array_equal(bl.incident_on(shades, rec, f, site), want) and np.array_equal(bl.incident_on(shades, rec[4], f[4], site), want[4])


def test_a_controlled_blind_closes_holds_and_opens():
    b, state = one_blind(), np.zeros(1, np.uint8)
    for I, want in ((299.0, 0), (300.0, 0), (301.0, 1), (200.0, 1), (150.0, 1), (149.0, 0), (200.0, 0), (1e9, 1)):
        p, f, fd, fg = step(I, b, state)
        assert state[0] == want and p[0] == float(want), (I, want)
    # closed: exactly f * beam_closed and so on; open: (f, fd, fg) to the bit
    p, f, fd, fg = step(500.0, b, state, shades=dict(SOUTH, diffuse_factor=[0.9], ground_factor=[0.7]))
    assert (p[0], f[0], fd[0], fg[0]) == (1.0, 0.75 * 0.1, 0.9 * 0.3, 0.7 * 0.5)
    p, f, fd, fg = step(10.0, b, state, f=1.0 / 3.0, shades=dict(SOUTH, diffuse_factor=[0.9], ground_factor=[0.7]))
    assert (p[0], state[0]) == (0.0, 0) and (f[0], fd[0], fg[0]) == (1.0 / 3.0, 0.9, 0.7)


def test_a_zone_gates_the_blind():
    b = one_blind(zone=[2], set_chan=[1], band=[1.0])
    row = [0.0, 24.0]                                                          # hi = 24.5, lo = 23.5
    state = np.zeros(1, np.uint8)
    for I, T, want in ((400.0, 24.5, 0), (400.0, 24.6, 1), (400.0, 24.0, 1), (200.0, 23.5, 1), (200.0, 23.4, 0), (400.0, 24.4, 0),
                       (400.0, 25.0, 1), (100.0, 25.0, 0)):
        step(I, b, state, T=[0.0, 0.0, T], row=row)
        assert state[0] == want, (I, T, want)
    # band 0: closes above the setpoint, opens below it, keeps its state on it
    b = one_blind(zone=[0], set_chan=[0], band=[0.0])
    for T, want in ((20.0, 0), (20.000001, 1), (20.0, 1), (19.999999, 0)):
        step(400.0, b, state, T=[T], row=[20.0])
        assert state[0] == want, (T, want)


def test_a_disabled_blind_opens_and_a_nan_keeps_the_state():
    b = one_blind(enable_chan=[0])
    state = np.ones(1, np.uint8)
    assert step(400.0, b, state, row=[1.0])[0][0] == 1.0
    for off in (0.0, -1.0, np.nan):                                            # (a NaN enable value disables)
        state[:] = 1
        p, f, fd, fg = step(400.0, b, state, row=[off])
        assert (p[0], state[0], f[0]) == (0.0, 0, 0.75)
    for start in (0, 1):                                                       # a NaN irradiance, a NaN zone temperature: the state stays
        state[:] = start
        assert step(np.nan, one_blind(), state)[0][0] == float(start) and state[0] == start
        gated = one_blind(zone=[0], set_chan=[0], band=[1.0])
        assert step(200.0, gated, state, T=[np.nan], row=[20.0])[0][0] == float(start) and state[0] == start
    state[:] = 0
    assert step(400.0, gated, state, T=[np.nan], row=[20.0])[0][0] == 0.0      # (not hot: it does not close either)
    state[:] = 1
    assert step(100.0, gated, state, T=[np.nan], row=[20.0])[0][0] == 0.0      # (below irr_open it opens whatever the zone holds)


def test_a_scheduled_blind_follows_its_channel():
    b = dict(shade=[0], beam_closed=[0.2], diffuse_closed=[0.0], ground_closed=[1.0], pos_chan=[1])
    state = np.array([1], np.uint8)
    for v, want in ((0.25, 0.25), (-3.0, 0.0), (7.0, 1.0), (0.0, 0.0), (1.0, 1.0)):
        p, f, fd, fg = step(1e9, b, state, row=[9.0, v])
        q = 1.0 - want
        assert p[0] == want and state[0] == 1                                  # (the state byte of a scheduled blind is left alone)
        assert (f[0], fd[0], fg[0]) == (0.75 * (q + want * 0.2), 1.0 * (q + want * 0.0), 1.0 * (q + want * 1.0))
    p, f, fd, fg = step(0.0, b, state, row=[9.0, np.nan])                      # a NaN position stays NaN and propagates
    assert np.isnan(p[0]) and np.isnan(f[0]) and np.isnan(fd[0]) and np.isnan(fg[0])


def test_open_blinds_leave_the_bits_and_unblinded_shades_get_copies():
    rng = np.random.default_rng(11)
    n = 50
    shades = dict(surface=np.zeros(n, np.int64), normal=tuple(rng.normal(size=(3, n))), diffuse_factor=rng.uniform(0.5, 1, n),
                  ground_factor=rng.uniform(0.3, 1, n))
    f = rng.random(n)
    j = rng.permutation(n)[:30]
    b = dict(shade=j, beam_closed=rng.random(30), diffuse_closed=rng.random(30), ground_closed=rng.random(30),
             irr_close=np.full(30, np.inf), irr_open=np.full(30, -np.inf))
    state = np.zeros(30, np.uint8)
    p, fe, fde, fge = bl.apply(rng.uniform(0, 1e4, n), np.zeros(0), np.zeros(0), b, state, f, shades)
    assert not p.any() and np.array_equal(fe, f) and np.array_equal(fde, shades["diffuse_factor"]) and np.array_equal(fge, shades["ground_factor"])
    state[:] = 1                                                               # all closed: the blinded shades move, the others do not
    p, fe, fde, fge = bl.apply(rng.uniform(0, 1e4, n), np.zeros(0), np.zeros(0), b, state, f, shades)
    rest = np.setdiff1d(np.arange(n), j)
    assert p.all() and np.array_equal(fe[j], f[j] * b["beam_closed"]) and np.array_equal(fe[rest], f[rest])
    assert np.array_equal(fde[j], shades["diffuse_factor"][j] * b["diffuse_closed"]) and np.array_equal(fge[rest], shades["ground_factor"][rest])
    # no blinds at all: copies
    p, fe, fde, fge = bl.apply(np.zeros(n), np.zeros(0), np.zeros(0), {}, np.zeros(0, np.uint8), f, shades)
    assert p.shape == (0,) and np.array_equal(fe, f) and fe is not f
    # the accumulators of a step
    total, closed, switches = np.zeros(3), np.zeros(3, np.int64), np.zeros(3, np.int64)
    bl.accumulate(np.array([0.25, 1.0, np.nan]), np.array([0, 1, 1], np.uint8), np.array([0, 0, 1], np.uint8), total, closed, switches)
    assert total[0] == 0.25 and total[1] == 1.0 and np.isnan(total[2]) and list(closed) == [1, 1, 0] and list(switches) == [0, 1, 0]


# ---- heat_blinds_check ----
@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


def good_blinds(md, n=45, n_shades=70):
    rng = np.random.default_rng(4)
    i = np.arange(n)
    kind = i % 4                                                               # scheduled, controlled, gated, gated with an enable channel
    return dict(shade=rng.permutation(n_shades)[:n], beam_closed=rng.random(n), diffuse_closed=rng.random(n), ground_closed=rng.random(n),
                pos_chan=np.where(kind == 0, 0, -1), irr_close=rng.uniform(200, 400, n), irr_open=rng.uniform(50, 200, n),
                zone=np.where(kind >= 2, i % int(md["n_zones"]), -1), set_chan=np.where(kind >= 2, 1, -1), band=rng.uniform(0, 1, n),
                enable_chan=np.where(kind == 3, 2, -1), state=(i % 2).astype(np.uint8))


def check(md, blinds, shades="good", **more):
    binding.blinds_check(md, blinds, good_shades(md) if shades == "good" else shades, good_sky(md), good_gains(md), **series(md, **more))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def _raw(md, blinds, shades="good", **fields):
    """heat_blinds_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**series(md))
    k, kkeep = binding.make_sky(**binding._sky_for_gains(good_sky(md), binding._model_normals(md), int(md["n_surfaces"])))
    g, gkeep = binding.make_solar_gains(**good_gains(md))
    h, hkeep = binding.make_shades(**(good_shades(md) if shades == "good" else shades or {}))
    b, bkeep = binding.make_blinds(**blinds)
    for name, v in fields.items():
        setattr(b, name, v)
    rc = L.heat_blinds_check(C.byref(desc), 1, C.byref(s), C.byref(k), C.byref(g), C.byref(h) if shades is not None else None, C.byref(b))
    return rc, L.heat_last_error().decode()


def test_good_empty_and_absent_blinds_are_accepted(model):
    g = good_blinds(model)
    check(model, g)
    check(model, None)
    check(model, {})
    check(model, {}, shades=None)
    check(model, {k: v for k, v in g.items() if k not in ("enable_chan", "state")})
    free = np.flatnonzero(g["pos_chan"] < 0)                                   # controlled blinds only, none gated: the rest is NULL
    check(model, {k: v[free] for k, v in g.items() if k in ("shade", "beam_closed", "diffuse_closed", "ground_closed", "irr_close", "irr_open")})
    timed = np.flatnonzero(g["pos_chan"] >= 0)                                 # scheduled blinds only: no thresholds
    check(model, {k: v[timed] for k, v in g.items() if k in ("shade", "beam_closed", "diffuse_closed", "ground_closed", "pos_chan")})
    # the shades' own refusals come first
    bad = good_shades(model)
    bad["width"] = bad["width"].copy()
    bad["width"][7] = -1.0
    code, msg = _code(lambda: check(model, g, shades=bad))
    assert code == E_INVALID_ARG and "shade 7:" in msg, msg


def test_counts_null_arrays_and_missing_shades_are_invalid_arguments(model):
    g = good_blinds(model)
    rc, msg = _raw(model, g, n_blinds=-1)
    assert rc == E_INVALID_ARG and "blind" in msg and "n_blinds -1" in msg, msg
    for field in ("shade", "beam_closed", "diffuse_closed", "ground_closed"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "blind 0" in msg and field in msg, (field, msg)
    for field, i in (("irr_close", 1), ("irr_open", 1), ("set_chan", 2), ("band", 2)):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "blind %d:" % i in msg and field in msg, (field, msg)
    for field in ("enable_chan", "state", "steps_closed", "switches", "sum_position"):
        assert _raw(model, g, **{field: None})[0] == 0, field                  # the nullable ones
    for shades in (None, {}):                                                  # n_blinds > 0 without shades
        rc, msg = _raw(model, g, shades=shades)
        assert rc == E_INVALID_ARG and "blind 0" in msg and "shade" in msg, msg


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, -1e-9])
def test_bad_values_are_refused(model, bad):
    g = good_blinds(model)
    for key in ("beam_closed", "diffuse_closed", "ground_closed"):
        a = g[key].copy()
        a[31] = bad
        code, msg = _code(lambda: check(model, dict(g, **{key: a})))
        assert code == E_INVALID_ARG and "blind 31:" in msg and key in msg, msg
    a = g["band"].copy()
    a[14] = bad                                                                # (blind 14 is gated by a zone)
    code, msg = _code(lambda: check(model, dict(g, band=a)))
    assert code == E_INVALID_ARG and "blind 14:" in msg and "band" in msg, msg
    a = g["band"].copy()
    a[13] = bad                                                                # (blind 13 has no zone: its band is not read)
    check(model, dict(g, band=a))
    if np.isfinite(bad):
        return
    for key in ("irr_close", "irr_open"):
        a = g[key].copy()
        a[9] = bad                                                             # (controlled)
        code, msg = _code(lambda: check(model, dict(g, **{key: a})))
        assert code == E_INVALID_ARG and "blind 9:" in msg and "not finite" in msg, msg
        a = g[key].copy()
        a[8] = bad                                                             # (scheduled: not read)
        check(model, dict(g, **{key: a}))


def test_thresholds_in_the_wrong_order_and_state_bytes_above_one_are_refused(model):
    g = good_blinds(model)
    a = g["irr_open"].copy()
    a[21] = g["irr_close"][21] + 1.0
    code, msg = _code(lambda: check(model, dict(g, irr_open=a)))
    assert code == E_INVALID_ARG and "blind 21:" in msg and "irr_open" in msg, msg
    a[21] = g["irr_close"][21]
    check(model, dict(g, irr_open=a))                                          # equal thresholds: no hysteresis, accepted
    a = g["state"].copy()
    a[44] = 2
    code, msg = _code(lambda: check(model, dict(g, state=a)))
    assert code == E_INVALID_ARG and "blind 44:" in msg and "state" in msg, msg


def test_numbers_out_of_range_are_size_errors(model):
    g = good_blinds(model)
    Z = int(model["n_zones"])
    for bad in (-1, 70, 2 ** 31 - 1):
        a = g["shade"].copy()
        a[5] = bad
        code, msg = _code(lambda: check(model, dict(g, shade=a)))
        assert code == E_SIZE and "blind 5:" in msg and "shade" in msg, msg
    a = g["shade"].copy()
    a[40] = a[3]
    code, msg = _code(lambda: check(model, dict(g, shade=a)))
    assert code == E_SIZE and "blind 40:" in msg and "already" in msg, msg
    for bad in (-2, Z, 2 ** 31 - 1):
        a = g["zone"].copy()
        a[6] = bad
        code, msg = _code(lambda: check(model, dict(g, zone=a)))
        assert code == E_SIZE and "blind 6:" in msg and "zone" in msg, msg
    for bad in (-2, 3, 2 ** 31 - 1):                                           # (the series has three channels)
        for key, i in (("pos_chan", 7), ("enable_chan", 11)):
            a = g[key].copy()
            a[i] = bad
            code, msg = _code(lambda: check(model, dict(g, **{key: a})))
            assert code == E_SIZE and "blind %d:" % i in msg and "channel" in msg, msg
    for bad in (-1, 3, 2 ** 31 - 1):
        a = g["set_chan"].copy()
        a[18] = bad                                                            # (gated)
        code, msg = _code(lambda: check(model, dict(g, set_chan=a)))
        assert code == E_SIZE and "blind 18:" in msg and "setpoint" in msg, msg
    a = g["set_chan"].copy()
    a[17] = 99                                                                 # (no zone: not read)
    check(model, dict(g, set_chan=a))


def test_march_without_a_batch_is_an_invalid_argument(model):
    L = binding.load_library()
    s, _ = binding.make_series(**series(model))
    b, _ = binding.make_blinds(**good_blinds(model))
    failed = C.c_int32(123)
    assert L.heat_batch_march_series_blinds(None, C.byref(s), *(None,) * 17, C.byref(b), None, None, C.byref(failed)) == E_INVALID_ARG
    assert failed.value == -1


def test_the_wrapper_reads_the_shapes(model):
    b, keep = binding.make_blinds(**good_blinds(model))
    assert b.n_blinds == 45 and keep["shade"].dtype == np.int32 and keep["state"].dtype == np.uint8 and keep["switches"].dtype == np.int64
    assert set(bc.ACC) <= set(keep) and not keep["sum_position"].any()
    b, keep = binding.make_blinds()
    assert b.n_blinds == 0 and not b.shade and not b.state and not b.irr_close
    b, keep = binding.make_blinds(**good_blinds(model), stats=("switches",))
    assert b.switches and not b.steps_closed and not b.sum_position and "sum_position" not in keep
    given = np.arange(45, dtype=np.int64)
    b, keep = binding.make_blinds(**good_blinds(model), switches=given)
    assert np.array_equal(keep["switches"], given) and keep["switches"] is not given       # (a copy: the march writes it)
    for bad in (dict(beam_closed=np.ones(44)), dict(zone=np.zeros(3)), dict(stats=("nonsense",)), dict(state=np.zeros(46, np.uint8))):
        with pytest.raises(ValueError):
            binding.make_blinds(**dict(good_blinds(model), **bad))
    with pytest.raises(ValueError):
        binding.make_blinds(**good_blinds(model), stats=(), switches=given)


# ---- the case builder of the GPU tests ----
@pytest.mark.parametrize("seed", [401, 402, 405])
def test_the_case_builder_takes_every_branch_of_the_rule(seed):
    """blinds_case asserts its pattern itself (97 blinds of seven kinds on 150 shades in shuffled order, a shared shade, closed
    factors of 0 and 1, positions beyond [0, 1]); here its loop with feedback runs on SYNTHETIC zone temperatures — a stand-in
    march that only moves the zones — and every branch of the rule must be taken."""
    md, st = mdl.ragged_mixed(700, Z=28, seed=1)
    rng = np.random.default_rng(seed)
    c = bc.blinds_case(md, st, rng)
    T0 = st[md["zone_slot"]].copy()

    def march(state, k):
        state[md["zone_slot"]] = T0 + 1.5 * np.sin(0.8 * k + np.arange(len(T0)))

    state = st.copy()
    march(state, -1)
    ref = bc.loop(c, state, march, md["zone_slot"])
    cov = bc.coverage(c, ref)
    assert cov["closed"] > 20 and cov["reopened"] > 20 and cov["both"] >= 5 and cov["held"] >= 5 and cov["fractional"] > 20 and cov["clamped"] > 20, cov
    assert ref["margin"]["I"] > 1e-6                                           # (the thresholds lie between the pattern's values)
    p, kind, b = ref["position"], c.kind, c.blinds
    assert set(np.unique(p[:, kind >= 2])) == {0.0, 1.0}
    for q in range(2, len(bc.KINDS)):                                          # every kind of controlled blind closes and reopens
        d = np.diff(p[:, kind == q], axis=0)
        assert (d > 0).any() and (d < 0).any(), bc.KINDS[q]
    # the room condition: a gated blind stays open above irr_close because its zone is not hot, and opens above irr_open because it is cool
    I, T = ref["incident"], np.stack([T0 + 1.5 * np.sin(0.8 * (k - 1) + np.arange(len(T0))) for k in range(c.n_steps)])
    gated = np.flatnonzero(kind >= 4)
    tz, setp, d = T[:, b["zone"][gated]], c.channel[:, b["set_chan"][gated]], b["band"][gated] / 2.0
    en = np.where(b["enable_chan"][gated] >= 0, c.channel[:, np.maximum(b["enable_chan"][gated], 0)] > 0, True)
    bright = I[:, gated] > b["irr_close"][gated]
    hot = tz > setp + d
    assert (bright & en & ~hot & (p[:, gated] == 0)).any() and (bright & en & hot).any() and np.all(p[:, gated][bright & en & hot] == 1)
    was = np.concatenate([np.zeros((1, len(gated))), p[:-1, gated]])
    assert ((was == 1) & (p[:, gated] == 0) & en & (I[:, gated] >= b["irr_open"][gated]) & (tz < setp - d)).any()
    # the enable channel: a disabled blind is open whatever the sun does
    for q, chan in ((3, b["enable_chan"][kind == 3][0]), (5, b["enable_chan"][kind == 5][0])):
        off = ~(c.channel[:, chan] > 0)
        assert off.any() and (~off).any() and not p[off][:, kind == q].any() and p[~off][:, kind == q].any()
    # the effective factors: untouched where the shade has no blind or the blind is open, exact where it is closed
    fd0, fg0 = bl.shade_factors(c.shades)
    blinded = np.zeros(sc.N_SHADES, bool)
    blinded[b["shade"]] = True
    for k, (fe, fde, fge) in enumerate(ref["eff"]):
        assert np.array_equal(fe[~blinded], c.f[k][~blinded]) and np.array_equal(fde[~blinded], fd0[~blinded])
        is_open, shut = b["shade"][p[k] == 0], p[k] == 1
        assert np.array_equal(fe[is_open], c.f[k][is_open]) and np.array_equal(fge[is_open], fg0[is_open])
        assert np.array_equal(fe[b["shade"][shut]], c.f[k][b["shade"][shut]] * b["beam_closed"][shut])
    # the blinds move what the consumers receive
    plain = sc.reference(md, c.channel, c.ref_drives, c.args, c.gains, c.shades)
    assert not np.array_equal(plain[3], ref["transmitted"]) and np.all(np.isfinite(ref["transmitted"]))
    # the accumulators are the rows' own sums, and a cut carries them
    carry = ref["carry"]
    assert np.array_equal(carry["steps_closed"], (p > 0).sum(axis=0)) and carry["switches"][kind >= 2].sum() == cov["closed"] + cov["reopened"]
    assert not carry["switches"][kind < 2].any()
    state = st.copy()
    march(state, -1)
    first = bc.loop(c, state, march, md["zone_slot"], steps=range(0, 9))
    second = bc.loop(c, state, march, md["zone_slot"], steps=range(9, c.n_steps), carry=first["carry"], ap_sum=first["ap_sum"])
    assert np.array_equal(np.concatenate([first["position"], second["position"]]), p)
    assert all(np.array_equal(second["carry"][k], carry[k]) for k in carry) and np.array_equal(second["ap_sum"], ref["ap_sum"])
    # heat_blinds_check accepts the case
    binding.blinds_check(md, c.blinds, c.shades, dict(c.args), dict(c.gains), weather=np.zeros((c.n_steps, 1, 3)), n_sub=1,
                         channel=c.channel, **{name: chan for name, (chan, _) in c.call.items()})


def test_blinds_check_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "blinds_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "blinds host check: all statuses as the header states them" in out.stdout
