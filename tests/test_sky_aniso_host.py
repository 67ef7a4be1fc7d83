"""Anisotropic sky of a series on the host (include/heat_amd.h, heat_sky_aniso / heat_sky_aniso_check / heat_series_call /
heat_batch_march_series_call; heat_amd/sky.py, solar_gains.py, blinds.py with aniso=): the entry points are declared, exported
and bound; the ctypes mirrors have the header's layout; the rule in numpy — the reference of tests/test_sky_aniso_gpu.py — gives
the hand-worked cases, written as the exact expression in the contract's order, and with zero coefficients the bits of the
isotropic rule; every refusal the header lists comes back with its code and names its item, before any device work; the case
builder of the GPU tests holds everything the rule distinguishes. heat_sky_aniso_check and the struct-size refusal also run
under AddressSanitizer / UBSan as a stand-alone program (tests/sky_aniso_host_main.cpp) in a child process. No GPU needed.

Reference: the rule is this project's own (the reference has no solar geometry)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from heat_amd import binding, blinds as bl, modeldict as mdl, sky, solar_gains
import blinds_cases as bc
import sky_aniso_cases as ac
from test_shades_host import N_STEPS, good_gains, good_shades, good_sky, series
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_sky_aniso_check", "heat_batch_march_series_call")
E_INVALID_ARG = -1
ANISO_FIELDS = ("coef", "front_band", "back_band", "aperture_band", "shade_band")
CALL_FIELDS = ("size", "s", "sky", "aniso", "shades", "gains", "l", "air", "il", "r", "radiation", "ambient", "blinds", "trace", "applied",
               "ideal_q", "transmitted", "path_q", "sunlit", "irradiance", "ambient_t", "position", "blind_incident", "failed_step")
Z0 = 0.08715574274765817


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    for struct in ("heat_sky_coef", "heat_sky_aniso", "heat_series_call"):
        assert "typedef struct %s {" % struct in header, struct
    assert "heat_sky_aniso_check" in binding.HOST_ONLY_SYMBOLS and "heat_batch_march_series_call" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("SkyCoef", "SkyAniso", "SeriesCall", "make_sky_aniso", "sky_aniso_check"))
    assert all(hasattr(sky, n) for n in ("hay_davies", "reindl", "band_reindl", "band_perez")) and sky.Z0 == Z0
    assert L.heat_amd_abi_version() == 1
    assert "0.08715574274765817" in header                                     # the literal is the contract
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW)
    assert all("pub struct %s" % s in rust for s in ("HeatSkyCoef", "HeatSkyAniso", "HeatSeriesCall"))
    # the struct entry point is beside the chain of positional ones, not a twelfth row of it
    assert all(symbol != "heat_batch_march_series_call" for symbol, _ in binding.HeatBatch._SERIES_ENTRY)
    assert len(binding.HeatBatch._SERIES_ENTRY) == 11 and "aniso" not in binding.HeatBatch._SERIES_ORDER


def test_layouts_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = (["sizeof(heat_sky_coef)", "sizeof(heat_sky_aniso)", "sizeof(heat_series_call)", "sizeof(heat_sky)", "sizeof(heat_blinds)"] +
            ["offsetof(heat_sky_coef, circ)", "offsetof(heat_sky_coef, horiz)"] + ["offsetof(heat_sky_aniso, %s)" % f for f in ANISO_FIELDS] +
            ["offsetof(heat_series_call, %s)" % f for f in CALL_FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == ([C.sizeof(binding.SkyCoef), C.sizeof(binding.SkyAniso), C.sizeof(binding.SeriesCall), C.sizeof(binding.Sky),
                    C.sizeof(binding.Blinds)] + [binding.SkyCoef.circ.offset, binding.SkyCoef.horiz.offset] +
                   [getattr(binding.SkyAniso, f).offset for f in ANISO_FIELDS] + [getattr(binding.SeriesCall, f).offset for f in CALL_FIELDS])
    assert got[0] == 16 and got[1] == 8 * len(ANISO_FIELDS) and got[2] == 8 * len(CALL_FIELDS)
    assert [f for f, _ in binding.SkyAniso._fields_] == list(ANISO_FIELDS) and [f for f, _ in binding.SeriesCall._fields_] == list(CALL_FIELDS)


# ---- the rule in numpy: hand-worked cases, each the exact expression in the contract's order ----
SOUTH = (0.0, -1.0, 0.0)
SOUTH_SHADE = dict(surface=[0], normal=(np.array([0.0]), np.array([-1.0]), np.array([0.0])))


def record(beam=500.0, diffuse=100.0, ground=40.0, sun=(0.0, -0.6, 0.8)):
    return np.array([sun[0], sun[1], sun[2], beam, diffuse, ground, 350.0, 420.0])


def test_a_south_wall_under_a_high_sun():
    # c = 0.6, fs = fg = 0.5, the sun at 0.8 above cos 85 deg: rb = 0.6 / 0.8
    circ, horiz, band = 0.3, 0.2, 0.7
    rb = 0.6 / 0.8
    bm = 500.0 * 0.6
    cs = (100.0 * circ) * rb
    sun = bm + cs
    dv = (100.0 * 0.5) * (1.0 - circ)
    hv = (100.0 * horiz) * band
    dv = dv + hv
    gv = 40.0 * 0.5
    assert sky.incident(record(), SOUTH, "solar_front", aniso=(circ, horiz, band)) == (sun + dv) + gv
    assert sky.incident(record(), (0.0, 1.0, 0.0), "solar_back", aniso=(circ, horiz, band)) == (sun + dv) + gv
    assert sky.incident(record(), SOUTH, "solar_front", shade=(0.75, 0.5, 0.25), aniso=(circ, horiz, band)) == (sun * 0.75 + dv * 0.5) + gv * 0.25
    # more than the isotropic sky gives this facade, and less on the opposite one: tens of W/m2
    iso = sky.incident(record(), SOUTH, "solar_front")
    north = sky.incident(record(), (0.0, 1.0, 0.0), "solar_front", aniso=(circ, horiz, band))
    assert (sun + dv) + gv - iso > 10.0 and sky.incident(record(), (0.0, 1.0, 0.0), "solar_front") - north > 0.0
    # an aperture: t = 0.2 c + 0.1 by Horner's rule, tau_diffuse 0.6, scale 2
    coef = np.array([0.1, 0.2, 0.0, 0.0, 0.0, 0.0])
    t = 0.2 * 0.6 + 0.1
    pbm = ((500.0 * 0.6) * t) * 2.0
    pcs = (cs * t) * 2.0
    ps = pbm + pcs
    pd = ((dv + gv) * 0.6) * 2.0
    got = solar_gains.transmitted(record(), SOUTH, coef, 0.6, 2.0, aniso=(circ, horiz, band))
    assert got[0] == ps and got[1] == pd
    got = solar_gains.transmitted(record(), SOUTH, coef, 0.6, 2.0, shade=(0.75, 0.5, 0.25), aniso=(circ, horiz, band))
    assert got[0] == ps * 0.75 and got[1] == ((dv * 0.5 + gv * 0.25) * 0.6) * 2.0
    behind = solar_gains.transmitted(record(), (0.0, 1.0, 0.0), coef, 0.6, 2.0, aniso=(circ, horiz, band))
    assert behind[0] == 0.0 and behind[1] == ((((100.0 * 0.5) * (1.0 - circ) + hv) + gv) * 0.6) * 2.0
    # a blind's I: the shaded side rule with the shade's geometric f and its constant factors
    I = bl.incident_on(SOUTH_SHADE, record()[None, :], np.array([0.75]), aniso=([circ], [horiz], [band]))
    assert I.shape == (1,) and I[0] == (sun * 0.75 + dv) + gv
    shaded = dict(SOUTH_SHADE, diffuse_factor=[0.5], ground_factor=[0.25])
    assert bl.incident_on(shaded, record()[None, :], np.array([0.75]), aniso=([circ], [horiz], [band]))[0] == (sun * 0.75 + dv * 0.5) + gv * 0.25
    # ... per site: a shade reads the pair of ITS surface's site
    two = bl.incident_on(dict(surface=[0, 1], normal=tuple(np.repeat(n, 2) for n in SOUTH_SHADE["normal"])), np.stack([record(), record()]),
                         np.array([0.75, 0.75]), site=np.array([1, 0]), aniso=([0.0, circ], [0.0, horiz], [band, band]))
    assert two[0] == (sun * 0.75 + dv) + gv and two[1] == bl.incident_on(SOUTH_SHADE, record()[None, :], np.array([0.75]))[0]
    with pytest.raises(ValueError):
        sky.incident(record(), SOUTH, "ir_front", aniso=(circ, horiz, band))


def test_a_grazing_sun_divides_by_cos_85_and_a_sun_below_the_horizon_gives_no_circumsolar():
    h = np.sqrt(1.0 - 0.05 ** 2)
    low = record(beam=0.0, ground=0.0, sun=(0.0, -h, 0.05))                   # c = h on the south wall
    assert sky.incident(low, SOUTH, "solar_front", aniso=(1.0, 0.0, 0.0)) == ((100.0 * 1.0) * (h / Z0) + (100.0 * 0.5) * 0.0) + 0.0
    assert sky.circumsolar_ratio(np.float64(h), np.float64(0.05)) == h / Z0 and sky.circumsolar_ratio(np.float64(0.3), np.float64(Z0)) == 0.3 / Z0
    assert sky.circumsolar_ratio(np.float64(0.3), np.float64(0.5)) == 0.3 / 0.5
    for sz in (0.0, -0.0, -0.6, np.nan):                                       # c > 0, but the sun is not above the horizon
        down = record(beam=0.0, ground=0.0, sun=(0.0, -0.8, sz))
        assert sky.incident(down, SOUTH, "solar_front", aniso=(0.5, 0.0, 0.3)) == (100.0 * 0.5) * 0.5
        assert solar_gains.transmitted(down, SOUTH, np.full(6, 0.1), 0.6, 2.0, aniso=(0.5, 0.0, 0.3))[0] == 0.0
    assert sky.circumsolar_ratio(np.float64(-0.2), np.float64(0.8)) == 0.0 and sky.circumsolar_ratio(np.float64(np.nan), np.float64(0.8)) == 0.0


def test_a_horizontal_face_receives_the_diffuse_radiation_it_is_given():
    """c == sun_z exactly on a face that looks straight up, so rb == 1: D (1 - F1) + D F1. Three roundings of half an ulp of
    at most ulp(D) each behind the exact 1 - F1 ... within 2 ulp of D."""
    rng = np.random.default_rng(7)
    n = 200000
    rec = np.zeros((n, 8))
    rec[:, sky.SUN_Z] = rng.uniform(Z0 * 1.0001, 1.0, n)
    rec[:, sky.SUN_X] = np.sqrt(1.0 - rec[:, sky.SUN_Z] ** 2)
    rec[:, sky.DIFFUSE] = rng.uniform(1.0, 600.0, n)
    circ = rng.uniform(0.0, 1.0, n)
    v = sky.incident(rec, (0.0, 0.0, 1.0), "solar_front", aniso=(circ, 0.0, rng.random(n)))
    D = rec[:, sky.DIFFUSE]
    worst = np.abs(v - D) / np.spacing(D)
    print("horizontal face: worst |v - D| = %.2f ulp of D" % worst.max())
    assert np.all(worst <= 2.0)


def test_zero_coefficients_give_the_bits_of_the_isotropic_rule():
    rng = np.random.default_rng(11)
    n = 120000
    normal = tuple(rng.normal(size=(3, n)))
    rec = np.concatenate([rng.normal(size=(n, 3)), rng.uniform(0, 900, (n, 1)), rng.uniform(0, 300, (n, 2)), rng.uniform(200, 450, (n, 2))], axis=1)
    rec[::7, :3] /= np.linalg.norm(rec[::7, :3], axis=1, keepdims=True)
    rec[::11, sky.BEAM] = 0.0
    zero, band = np.zeros(n), rng.uniform(0.0, 2.0, n)
    shade = (rng.random(n), rng.uniform(0.5, 1.0, n), rng.uniform(0.3, 1.0, n))
    for side in ("solar_front", "solar_back"):
        for sh in (None, shade):
            assert np.array_equal(sky.incident(rec, normal, side, shade=sh), sky.incident(rec, normal, side, shade=sh, aniso=(zero, zero, band)))
    ap = (rng.uniform(-1, 1, (n, 6)), rng.random(n), rng.uniform(1, 5, n))
    for sh in (None, shade):
        want, got = solar_gains.transmitted(rec, normal, *ap, shade=sh), solar_gains.transmitted(rec, normal, *ap, shade=sh, aniso=(zero, zero, band))
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    for factors in (dict(), dict(diffuse_factor=shade[1], ground_factor=shade[2])):
        shades = dict(surface=rng.integers(0, 50, n), normal=normal, **factors)
        site = rng.integers(0, 3, 50)
        rec3 = rec[:3 * (n // 3)].reshape(-1, 3, 8)[:40]                       # [40 steps, 3 sites, 8]
        f = rng.random((40, n))
        want = bl.incident_on(shades, rec3, f, site)
        assert np.array_equal(want, bl.incident_on(shades, rec3, f, site, aniso=(np.zeros((40, 3)), np.zeros((40, 3)), band)))
        assert want.size >= 10 ** 5
    # ... and coefficients that are not zero do move all three
    assert not np.array_equal(sky.incident(rec, normal, "solar_front"), sky.incident(rec, normal, "solar_front", aniso=(zero + 0.3, zero, band)))
    assert not np.array_equal(sky.incident(rec, normal, "solar_front"), sky.incident(rec, normal, "solar_front", aniso=(zero, zero + 0.1, band)))


def test_the_conveniences():
    rec = np.stack([record(beam=600.0), record(beam=0.0, diffuse=0.0), record(beam=5000.0), record(beam=300.0, sun=(0.0, -0.8, -0.6))])
    day = 172.0
    circ, horiz = sky.hay_davies(rec, day)
    extra = 1367.0 * (1.0 + 0.033 * np.cos(2.0 * np.pi * day / 365.0))
    assert circ[0] == 600.0 / extra and circ[1] == 0.0 and circ[2] == 1.0 and not horiz.any()
    rcirc, rhoriz = sky.reindl(rec, day)
    assert np.array_equal(rcirc, circ)
    assert rhoriz[0] == (1.0 - circ[0]) * np.sqrt((600.0 * 0.8) / (600.0 * 0.8 + 100.0)) and rhoriz[1] == 0.0 and rhoriz[2] == 0.0
    assert rhoriz[3] == 0.0                                                    # (the sun below the horizon: no beam on the horizontal)
    # on a horizontal plane Reindl's band is 0: reindl equals hay_davies
    up = (0.0, 0.0, 1.0)
    assert sky.band_reindl(up) == 0.0
    assert np.array_equal(sky.incident(rec, up, "solar_front", aniso=(rcirc, rhoriz, sky.band_reindl(up))),
                          sky.incident(rec, up, "solar_front", aniso=(circ, horiz, 0.0)))
    assert sky.band_reindl(SOUTH) == 0.5 * 0.5 ** 1.5
    assert sky.band_perez(SOUTH) == 1.0 and sky.band_perez(up) == 0.0 and sky.band_perez((0.0, 0.6, 0.8)) == np.sqrt(1.0 - 0.8 * 0.8)
    n = np.array([0.0, 0.6, 1.0, -1.0])
    assert sky.band_perez((n, n, n)).shape == (4,) and sky.band_reindl((n, n, n)).shape == (4,)


# ---- heat_sky_aniso_check ----
@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


def good_aniso(md, n_apertures=12, n_shades=70, n_sites=1):
    rng = np.random.default_rng(6)
    S = int(md["n_surfaces"])
    return dict(coef=rng.uniform(0.0, 0.6, (N_STEPS, n_sites, 2)), front_band=rng.random(S), back_band=rng.random(S),
                aperture_band=rng.random(n_apertures), shade_band=rng.random(n_shades))


def check(md, aniso, sky_args="good", gains="good", shades="good", **more):
    binding.sky_aniso_check(md, aniso, good_sky(md) if sky_args == "good" else sky_args, good_gains(md) if gains == "good" else gains,
                            good_shades(md) if shades == "good" else shades, **series(md, **more))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def test_good_empty_and_absent_anisotropic_skies_are_accepted(model):
    g = good_aniso(model)
    check(model, g)
    check(model, None)
    check(model, dict(coef=g["coef"]))                                         # no bands: zeros
    check(model, {k: g[k] for k in ("coef", "front_band", "back_band")}, gains=None, shades=None)
    check(model, dict(g, coef=np.full_like(g["coef"], np.nan)))                # the coefficients are the caller's
    # the shades' own refusals come first
    bad = good_shades(model)
    bad["width"] = bad["width"].copy()
    bad["width"][7] = -1.0
    code, msg = _code(lambda: check(model, g, shades=bad))
    assert code == E_INVALID_ARG and "shade 7:" in msg, msg


def test_what_the_coefficients_and_the_bands_need(model):
    g = good_aniso(model)
    sides = {k: g[k] for k in ("coef", "front_band", "back_band")}
    code, msg = _code(lambda: check(model, sides, sky_args=None, gains=None, shades=None))
    assert code == E_INVALID_ARG and "sky is NULL" in msg, msg
    S = int(model["n_surfaces"])
    code, msg = _code(lambda: check(model, sides, sky_args=dict(record=None, mode=np.zeros(S, np.uint8)), gains=None, shades=None))
    assert code == E_INVALID_ARG and "sky->record is NULL" in msg, msg
    code, msg = _code(lambda: check(model, dict(g, coef=None)))
    assert code == E_INVALID_ARG and "coef is NULL" in msg, msg
    code, msg = _code(lambda: check(model, {k: v for k, v in g.items() if k != "shade_band"}, gains=None, shades=None))
    assert code == E_INVALID_ARG and "aperture_band" in msg and "aperture a" in msg, msg
    code, msg = _code(lambda: check(model, {k: v for k, v in g.items() if k != "aperture_band"}, shades=None))
    assert code == E_INVALID_ARG and "shade_band" in msg and "shade j" in msg, msg
    # the wrapper reads the shapes
    for bad in (dict(coef=g["coef"][:-1]), dict(coef=np.zeros((N_STEPS, 3))), dict(front_band=np.zeros(S + 1)), dict(aperture_band=np.zeros(3)),
                dict(shade_band=np.zeros(71))):
        with pytest.raises(ValueError):
            check(model, dict(g, **bad))
    an, keep = binding.make_sky_aniso(**g)
    assert an.coef and an.front_band and an.shade_band and keep["coef"].shape == (N_STEPS, 1, 2)
    an, keep = binding.make_sky_aniso(g["coef"][:, 0, :])
    assert an.coef and not an.front_band and not an.back_band and not an.aperture_band and not an.shade_band


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, -1e-9])
def test_bad_bands_are_refused_where_a_consumer_reads_them(model, bad):
    g = good_aniso(model)

    def damaged(key, at):
        a = g[key].copy()
        a[at] = bad
        return dict(g, **{key: a})

    # good_sky's modes are surface % 4: bit 0 the front, bit 1 the back
    for key, at, who in (("front_band", 41, "surface 41:"), ("front_band", 43, "surface 43:"), ("back_band", 42, "surface 42:"),
                         ("back_band", 199, "surface 199:"), ("aperture_band", 0, "aperture 0:"), ("aperture_band", 11, "aperture 11:"),
                         ("shade_band", 69, "shade 69:")):
        code, msg = _code(lambda: check(model, damaged(key, at)))
        assert code == E_INVALID_ARG and who in msg and key in msg, msg
    for key, at in (("front_band", 40), ("front_band", 42), ("back_band", 40), ("back_band", 41)):
        check(model, damaged(key, at))                                          # (the side's solar input is not sky-driven: not read)
    check(model, dict(g, front_band=np.zeros(int(model["n_surfaces"]))))        # zero is a band


def test_the_call_struct_is_checked_before_anything_else(model):
    L = binding.load_library()
    s, _ = binding.make_series(**series(model))
    failed = C.c_int32(123)
    assert L.heat_batch_march_series_call(None, None) == E_INVALID_ARG and "series call is NULL" in L.heat_last_error().decode()
    call = binding.SeriesCall(s=C.pointer(s), failed_step=C.pointer(failed))
    for size in (0, C.sizeof(binding.SeriesCall) - 8, C.sizeof(binding.SeriesCall) + 8):
        call.size = size
        assert L.heat_batch_march_series_call(None, C.byref(call)) == E_INVALID_ARG
        assert "size %d" % size in L.heat_last_error().decode() and failed.value == 123      # (a struct of another size is not read further)
    call = binding.SeriesCall(size=C.sizeof(binding.SeriesCall), failed_step=C.pointer(failed))
    assert L.heat_batch_march_series_call(None, C.byref(call)) == E_INVALID_ARG and "s is NULL" in L.heat_last_error().decode()
    call.s = C.pointer(s)
    assert L.heat_batch_march_series_call(None, C.byref(call)) == E_INVALID_ARG and "NULL batch" in L.heat_last_error().decode()
    assert failed.value == -1


# ---- the case builder of the GPU tests ----
@pytest.mark.parametrize("seed", [471, 472, 475])
def test_the_case_builder_holds_everything_the_rule_distinguishes(seed):
    md, st = mdl.ragged_mixed(700, Z=28, seed=1)
    c = ac.aniso_case(md, st, np.random.default_rng(seed))
    T0 = st[md["zone_slot"]].copy()

    def march(state, k):
        state[md["zone_slot"]] = T0 + 1.5 * np.sin(0.8 * k + np.arange(len(T0)))

    state = st.copy()
    march(state, -1)
    ref = ac.loop(c, state, march, md["zone_slot"])
    cov = ac.coverage(c, ref)
    assert ac.covered(cov), cov
    assert cov["sun_grazing"] >= 2 and cov["decisions_moved"] >= 5 and cov["hay_davies_steps"] >= 1, cov
    bcov = bc.coverage(c, ref)
    assert bcov["closed"] > 20 and bcov["reopened"] > 20 and bcov["fractional"] > 20, bcov
    assert np.all(np.isfinite(ref["transmitted"])) and np.array_equal(ref["incident"], c.I[:, c.blinds["shade"]])
    # with every pair zero the anisotropic loop is the isotropic loop of blinds_cases, to the bit
    zero = ac.namespace_copy(c, coef=np.zeros_like(c.coef), I=c.I_iso)
    a, b = st.copy(), st.copy()
    march(a, -1), march(b, -1)
    got, want = ac.loop(zero, a, march, md["zone_slot"]), bc.loop(zero, b, march, md["zone_slot"])
    assert np.array_equal(got["position"], want["position"], equal_nan=True) and np.array_equal(got["transmitted"], want["transmitted"])
    assert np.array_equal(a, b) and not np.array_equal(ref["transmitted"], want["transmitted"]) and not np.array_equal(state, b)
    # a cut carries what the blinds carry; the rule itself has no memory
    state2 = st.copy()
    march(state2, -1)
    first = ac.loop(c, state2, march, md["zone_slot"], steps=range(0, 9))
    second = ac.loop(c, state2, march, md["zone_slot"], steps=range(9, c.n_steps), carry=first["carry"], ap_sum=first["ap_sum"])
    assert np.array_equal(np.concatenate([first["position"], second["position"]]), ref["position"], equal_nan=True)
    assert np.array_equal(second["ap_sum"], ref["ap_sum"]) and np.array_equal(state2, state)
    # heat_sky_aniso_check accepts the case
    binding.sky_aniso_check(md, ac.aniso_kwargs(c), dict(c.args), dict(c.gains), c.shades, weather=np.zeros((c.n_steps, 1, 3)), n_sub=1,
                            channel=c.channel, **{name: chan for name, (chan, _) in c.call.items()})


def test_sky_aniso_check_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "sky_aniso_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "sky aniso host check: all statuses as the header states them" in out.stdout
