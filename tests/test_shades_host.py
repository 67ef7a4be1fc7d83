"""Shades of a series on the host (include/heat_amd.h, heat_shades / heat_shades_check / heat_batch_march_series_shaded;
heat_amd/shading.py): the entry points are declared, exported and bound; the ctypes mirror has the header's layout; the rule in
numpy (shading.sunlit — the reference of tests/test_shades_gpu.py) gives the hand-worked cases; shades that shade nothing leave
the bits of sky.incident and solar_gains.transmitted alone; every refusal the header lists comes back with its code and names
the shade, horizon, surface or aperture, before any device work; the case builder of the GPU tests covers what it promises.
heat_shades_check also runs under AddressSanitizer / UBSan as a stand-alone program (tests/shades_host_main.cpp) in a child
process. No GPU needed.

Reference: the rule is this project's own (solar geometry lives in another SIMPLE crate)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from heat_amd import binding, modeldict as mdl, shading, sky, solar_gains
import shades_cases as sc
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_shades_check", "heat_batch_march_series_shaded")
E_INVALID_ARG, E_SIZE = -1, -4
N_STEPS = 4
FIELDS = ("n_shades", "sh_surface", "sh_normal_x", "sh_normal_y", "sh_normal_z", "sh_right_x", "sh_right_y", "sh_right_z", "sh_up_x",
          "sh_up_y", "sh_up_z", "sh_width", "sh_height", "overhang_depth", "overhang_gap", "fin_pos_depth", "fin_pos_gap", "fin_neg_depth",
          "fin_neg_gap", "diffuse_factor", "ground_factor", "sh_horizon", "n_horizons", "horizon_tan2", "front_shade", "back_shade",
          "aperture_shade")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_shades {" in header
    assert "heat_shades_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_shaded" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("Shades", "make_shades", "shades_check"))
    assert all(hasattr(shading, n) for n in ("sunlit", "frame_of", "horizon_tan2"))
    assert L.heat_amd_abi_version() == 1
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW)


def test_shades_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = (["sizeof(heat_shades)", "sizeof(heat_solar_gains)", "sizeof(heat_sky)", "sizeof(heat_sky_record)", "sizeof(heat_series)",
             "sizeof(heat_air_paths)"] + ["offsetof(heat_shades, %s)" % f for f in FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    # (the structs beside it keep their sizes: the shades are a struct of their own)
    assert got == ([C.sizeof(binding.Shades), C.sizeof(binding.SolarGains), C.sizeof(binding.Sky), 64, C.sizeof(binding.Series),
                    C.sizeof(binding.AirPaths)] + [getattr(binding.Shades, f).offset for f in FIELDS])
    assert [f for f, _ in binding.Shades._fields_] == list(FIELDS)
    assert got[0] == 8 * len(FIELDS)


# ---- the rule in numpy: hand-worked cases ----
SOUTH = dict(normal=(0.0, -1.0, 0.0), right=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))


def record(sun):
    return np.array([sun[0], sun[1], sun[2], 800.0, 120.0, 45.0, 350.0, 420.0])


def test_a_south_window_under_an_overhang_at_the_solstices():
    """48 degrees north, 0.6 m of overhang 0.2 m above 1.5 m of glass, solar noon: the sun stands due south at
    90 - 48 +- 23.45 degrees, the shadow's lower edge is depth x tan(elevation) below the plate."""
    lat = math.radians(48.0)
    D, G, H = 0.6, 0.2, 1.5
    for day, about in ((172, 0.25), (355, 1.0)):
        sun = sky.sun_direction(day, 12.0, lat)
        decl = math.radians(23.45) * math.sin(2.0 * math.pi * (284.0 + day) / 365.0)
        elevation = math.pi / 2 - lat + decl
        assert abs(sun[0]) < 1e-15 and sun[1] < 0 and abs(math.asin(sun[2]) - elevation) < 1e-12
        f = shading.sunlit(record(sun), width=1.2, height=H, overhang_depth=D, overhang_gap=G, **SOUTH)
        want = (H - min(max(D * math.tan(elevation) - G, 0.0), H)) / H
        assert abs(f - want) <= 1e-12 and abs(f - about) < 0.01, (day, float(f), want)
    # exactly: the shadow of a plate 0.5 m deep under a sun at 45 degrees due south falls 0.5 m: 0.25 m into the glass
    f = shading.sunlit(record((0.0, -0.5, 0.5)), width=1.0, height=1.0, overhang_depth=0.5, overhang_gap=0.25, **SOUTH)
    assert f == 0.75
    # a sun below the plate's plane (vs <= 0) is not shaded by it; a sun behind the wall lights nothing
    assert shading.sunlit(record((0.0, -0.8, -0.6)), width=1.0, height=1.0, overhang_depth=0.5, **SOUTH) == 1.0
    assert shading.sunlit(record((0.0, 0.5, 0.5)), width=1.0, height=1.0, overhang_depth=0.5, **SOUTH) == 0.0
    assert shading.sunlit(record((0.6, 0.0, 0.8)), width=1.0, height=1.0, **SOUTH) == 0.0           # c == 0 exactly
    assert shading.sunlit(record((np.nan, -0.5, 0.5)), width=1.0, height=1.0, **SOUTH) == 0.0       # a NaN: no beam
    # a very deep plate shades everything
    assert shading.sunlit(record((0.0, -0.5, 0.5)), width=1.0, height=1.0, overhang_depth=50.0, **SOUTH) == 0.0


def test_fins_shade_from_their_own_side():
    kw = dict(width=2.0, height=1.0, fin_pos_depth=0.5, fin_neg_depth=1.0, **SOUTH)
    # sun in the south-east (us > 0): the fin beside the +u (east) edge; tan of the relative azimuth is 1
    assert shading.sunlit(record((0.5, -0.5, 0.5)), **kw) == (2.0 - 0.5) / 2.0
    # sun in the south-west: the other fin, twice as deep
    assert shading.sunlit(record((-0.5, -0.5, 0.5)), **kw) == (2.0 - 1.0) / 2.0
    assert shading.sunlit(record((0.0, -0.6, 0.8)), **kw) == 1.0                                     # us == 0: neither
    assert shading.sunlit(record((0.5, -0.5, 0.5)), fin_pos_gap=0.5, **kw) == 1.0                    # the gap swallows the shadow
    assert shading.sunlit(record((0.96, -0.28, 0.0)), **kw) == (2.0 - 0.5 * (0.96 / 0.28)) / 2.0    # (W - sw) / W, sw < W
    assert shading.sunlit(record((0.999, -0.01, 0.0)), **kw) == 0.0                                  # clamped to W
    # overhang and fins multiply
    f = shading.sunlit(record((0.5, -0.5, 0.5)), overhang_depth=0.25, **kw)
    assert f == 0.75 * 0.75


def test_the_sector_rule_is_floor_of_atan2_off_the_boundaries():
    rng = np.random.default_rng(5)
    sx, sy = rng.normal(size=20000), rng.normal(size=20000)
    deg = np.degrees(np.arctan2(sy, sx)) % 360.0
    off = np.abs(deg / 22.5 - np.round(deg / 22.5)) > 1e-9
    assert off.sum() > 19000 and np.array_equal(shading.sector_of(sx, sy)[off], np.floor(deg[off] / 22.5).astype(np.int64))
    assert set(shading.sector_of(sx, sy)) == set(range(16))
    # on the boundaries: what the header says; whatever the sun holds the sector is inside the table
    assert [int(shading.sector_of(x, y)) for x, y in ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))] == \
        [0, 1, 3, 6, 7, 9, 12, 14]
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0])
    s = shading.sector_of(odd[:, None], odd[None, :])
    assert s.min() >= 0 and s.max() <= 15


def test_the_horizon_hides_a_sun_below_its_profile():
    tan2 = shading.horizon_tan2(np.where(np.arange(16) == 13, 30.0, 5.0))                            # a hill in sector 13 (SSE .. SE)
    assert abs(tan2[13] - 1.0 / 3.0) < 1e-15
    kw = dict(width=1.0, height=1.0, horizon=0, horizon_tan2=tan2[None, :], **SOUTH)
    az = math.radians(22.5 * 13.5)
    for elevation, lit in ((29.0, 0.0), (31.0, 1.0), (-5.0, 0.0)):
        e = math.radians(elevation)
        sun = (math.cos(e) * math.cos(az), math.cos(e) * math.sin(az), math.sin(e))
        assert shading.sector_of(sun[0], sun[1]) == 13 and shading.sunlit(record(sun), **kw) == lit
    e = math.radians(10.0)                                                                           # beside the hill: above 5 degrees
    az = math.radians(22.5 * 12.5)
    assert shading.sunlit(record((math.cos(e) * math.cos(az), math.cos(e) * math.sin(az), math.sin(e))), **kw) == 1.0
    assert shading.sunlit(record((0.0, -0.8, -0.6)), width=1.0, height=1.0, **SOUTH) == 1.0          # no profile: no horizon test
    assert shading.sunlit(record((0.0, -0.8, -0.6)), **kw) == 0.0
    with pytest.raises(ValueError):
        shading.horizon_tan2(np.full(16, 90.0))


def test_frame_of_gives_a_right_handed_frame():
    rng = np.random.default_rng(6)
    n = rng.normal(size=(3, 300))
    n[:2, :20] = 0.0                                                                                 # roofs and soffits
    n[2, 20:60] = 0.0                                                                                # walls
    u, v = shading.frame_of(tuple(n))
    u, v = np.array(u), np.array(v)
    unit = n / np.linalg.norm(n, axis=0)
    assert np.allclose(np.cross(v.T, unit.T), u.T, atol=1e-14) and np.allclose((u * u).sum(axis=0), 1.0) and np.all(u[2] == 0.0)
    assert np.all(v[2, 20:] > 0) and np.allclose((u * unit).sum(axis=0), 0.0, atol=1e-15)
    (ux, uy, uz), (vx, vy, vz) = shading.frame_of((0.0, -1.0, 0.0))
    assert (ux, uy, uz, vx, vy, vz) == (1.0, 0.0, 0.0, 0.0, 0.0, 1.0)                                # a south wall: east and up


def test_a_shade_that_shades_nothing_leaves_the_bits_alone():
    rng = np.random.default_rng(7)
    n = 400
    rec = np.concatenate([rng.normal(size=(n, 3)), rng.uniform(0, 900, (n, 1)), rng.uniform(-50, 300, (n, 2)), rng.uniform(250, 480, (n, 2))], axis=1)
    rec[::17, 0] = np.nan
    normal = tuple(rng.normal(size=(3, n)))
    u, v = shading.frame_of(normal)
    f = shading.sunlit(rec, normal, u, v, np.ones(n), np.ones(n))
    c = (normal[0] * rec[:, 0] + normal[1] * rec[:, 1]) + normal[2] * rec[:, 2]
    assert np.array_equal(f, np.where(c > 0, 1.0, 0.0)) and (f == 1).any() and (f == 0).any()
    one = (f, np.ones(n), np.ones(n))
    assert np.array_equal(sky.incident(rec, normal, "solar_front"), sky.incident(rec, normal, "solar_front", shade=one))
    back = shading.sunlit(rec, tuple(-a for a in normal), u, v, np.ones(n), np.ones(n))
    assert np.array_equal(sky.incident(rec, normal, "solar_back"), sky.incident(rec, normal, "solar_back", shade=(back, np.ones(n), np.ones(n))))
    coef = rng.uniform(-0.2, 0.9, (n, 6))
    plain = solar_gains.transmitted(rec, normal, coef, 0.5, 2.0)
    shaded = solar_gains.transmitted(rec, normal, coef, 0.5, 2.0, shade=one)
    assert np.array_equal(plain[0], shaded[0]) and np.array_equal(plain[1], shaded[1])
    # ... and a shade that does shade: the beam scales with f, the other two parts with their factors
    half = solar_gains.transmitted(rec, normal, coef, 0.5, 2.0, shade=(0.5 * f, np.ones(n), np.ones(n)))
    assert np.array_equal(half[0], plain[0] * 0.5) and np.array_equal(half[1], plain[1])
    with pytest.raises(ValueError):
        sky.incident(rec, normal, "ir_front", shade=one)


# ---- heat_shades_check ----
@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


def series(md, **more):
    S = int(md["n_surfaces"])
    chan = np.full(S, -1, np.int32)
    return dict(dict(weather=np.zeros((N_STEPS, 2, 3)), n_sub=2, channel=np.zeros((N_STEPS, 3)), solar_front=chan, solar_back=chan), **more)


def good_sky(md, n_sites=1):
    S = int(md["n_surfaces"])
    return dict(record=np.random.default_rng(1).random((N_STEPS, n_sites, 8)), mode=(np.arange(S) % 4).astype(np.uint8))


def good_gains(md, n_apertures=12):
    rng = np.random.default_rng(2)
    return dict(ap_surface=np.arange(n_apertures) * 16 + 3, ap_normal=tuple(rng.normal(size=(3, n_apertures))),
                ap_tau_coef=rng.uniform(-1, 1, (n_apertures, 6)), ap_tau_diffuse=rng.random(n_apertures), ap_scale=rng.uniform(1, 5, n_apertures))


def good_shades(md, n=70, n_apertures=12):
    S = int(md["n_surfaces"])
    rng = np.random.default_rng(3)
    normal = tuple(rng.normal(size=(3, n)))
    right, up = shading.frame_of(normal)
    q = np.arange(S)
    return dict(surface=rng.integers(0, S, n), normal=normal, right=right, up=up, width=rng.uniform(1, 3, n), height=rng.uniform(1, 2, n),
                overhang_depth=rng.uniform(0, 1, n), overhang_gap=rng.uniform(0, 0.3, n), fin_pos_depth=rng.uniform(0, 1, n),
                fin_pos_gap=rng.uniform(0, 0.3, n), fin_neg_depth=rng.uniform(0, 1, n), fin_neg_gap=rng.uniform(0, 0.3, n),
                diffuse_factor=rng.uniform(0.5, 1, n), ground_factor=rng.uniform(0.5, 1, n), horizon=(np.arange(n) % 5 - 1).astype(np.int32),
                horizon_tan2=rng.uniform(0, 0.3, (4, 16)), front_shade=np.where(q % 4 % 2 == 1, q % n, -1), back_shade=np.where(q % 4 >= 2, (3 * q) % n, -1),
                aperture_shade=np.where(np.arange(n_apertures) % 2 == 1, np.arange(n_apertures) * 5, -1))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def check(md, shades, sky_args="good", gains="good", **more):
    binding.shades_check(md, shades, good_sky(md) if sky_args == "good" else sky_args, good_gains(md) if gains == "good" else gains,
                         **series(md, **more))


def _raw(md, shades, sky_args="good", gains="good", **fields):
    """heat_shades_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**series(md))
    k, kkeep = binding.make_sky(**binding._sky_for_gains(good_sky(md) if sky_args == "good" else sky_args, binding._model_normals(md),
                                                         int(md["n_surfaces"])))
    g, gkeep = binding.make_solar_gains(**(good_gains(md) if gains == "good" else gains or {}))
    h, hkeep = binding.make_shades(**shades)
    for name, v in fields.items():
        setattr(h, name, v)
    rc = L.heat_shades_check(C.byref(desc), 1, C.byref(s), C.byref(k) if sky_args is not None else None,
                             C.byref(g) if gains is not None else None, C.byref(h))
    return rc, L.heat_last_error().decode()


def test_good_empty_and_absent_shades_are_accepted(model):
    check(model, good_shades(model))
    check(model, None)
    check(model, {})
    check(model, {}, None, None)                                                                    # ... which need neither sky nor gains
    g = good_shades(model)
    check(model, {k: v for k, v in g.items() if k not in ("diffuse_factor", "ground_factor", "horizon", "horizon_tan2")})
    check(model, {k: v for k, v in g.items() if not k.endswith("_shade")})                          # shades nobody refers to
    check(model, {k: v for k, v in g.items() if k != "aperture_shade"}, gains=None)
    binding.shades_check(model, g, good_sky(model, 3), good_gains(model), n_sites=3, **series(model, weather=np.zeros((N_STEPS, 2, 3, 3))))
    # the series', the sky's and the gains' own refusals come first
    S = int(model["n_surfaces"])
    code, msg = _code(lambda: check(model, g, solar_front=np.full(S, 2, np.int32)))
    assert code == E_SIZE and "surface 1" in msg, msg
    code, msg = _code(lambda: check(model, g, gains=dict(good_gains(model), ap_scale=np.full(12, np.nan))))
    assert code == E_INVALID_ARG and "aperture 0" in msg, msg


def test_negative_counts_and_null_arrays_are_invalid_arguments(model):
    g = good_shades(model)
    rc, msg = _raw(model, g, n_shades=-1)
    assert rc == E_INVALID_ARG and "shade" in msg and "n_shades -1" in msg, msg
    rc, msg = _raw(model, g, n_horizons=-3)
    assert rc == E_INVALID_ARG and "horizon" in msg and "n_horizons -3" in msg, msg
    for field in FIELDS[1:19]:
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "shade 0" in msg and field in msg, (field, msg)
    for field in ("diffuse_factor", "ground_factor", "sh_horizon", "front_shade", "back_shade", "aperture_shade"):
        assert _raw(model, g, **{field: None})[0] == 0, field                                      # the nullable ones
    rc, msg = _raw(model, g, horizon_tan2=None)
    assert rc == E_INVALID_ARG and "horizon 0" in msg, msg
    free = {k: v for k, v in g.items() if not k.endswith("_shade")}
    rc, msg = _raw(model, free, None, None)
    assert rc == E_INVALID_ARG and "shade 0" in msg and "sky is NULL" in msg, msg
    rc, msg = _raw(model, free, dict(record=None), None)
    assert rc == E_INVALID_ARG and "shade 0" in msg and "sky->record is NULL" in msg, msg
    rc, msg = _raw(model, g, gains=None)
    assert rc == E_INVALID_ARG and "aperture 0" in msg and "gains" in msg, msg


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_values_that_are_not_finite_are_refused(model, bad):
    g = good_shades(model)
    for key in ("normal", "right", "up"):
        for axis in range(3):
            vec = [np.array(a, dtype=np.float64) for a in g[key]]
            vec[axis][7] = bad
            code, msg = _code(lambda: check(model, dict(g, **{key: vec})))
            assert code == E_INVALID_ARG and "shade 7:" in msg and "sh_%s_%s" % (key, "xyz"[axis]) in msg, msg
    for key in ("width", "height") + shading.GEOMETRY + ("diffuse_factor", "ground_factor"):
        a = g[key].copy()
        a[33] = bad
        code, msg = _code(lambda: check(model, dict(g, **{key: a})))
        assert code == E_INVALID_ARG and "shade 33:" in msg and key in msg, msg
    tan2 = g["horizon_tan2"].copy()
    tan2[2, 9] = bad
    code, msg = _code(lambda: check(model, dict(g, horizon_tan2=tan2)))
    assert code == E_INVALID_ARG and "horizon 2:" in msg and "tan2[9]" in msg, msg


def test_lengths_of_the_wrong_sign_are_refused(model):
    g = good_shades(model)
    for key in ("width", "height"):
        for bad in (0.0, -1.5):
            a = g[key].copy()
            a[12] = bad
            code, msg = _code(lambda: check(model, dict(g, **{key: a})))
            assert code == E_INVALID_ARG and "shade 12:" in msg and "not positive" in msg, msg
    for key in shading.GEOMETRY:
        a = g[key].copy()
        a[69] = -1e-9
        code, msg = _code(lambda: check(model, dict(g, **{key: a})))
        assert code == E_INVALID_ARG and "shade 69:" in msg and "negative" in msg, msg
    tan2 = g["horizon_tan2"].copy()
    tan2[3, 0] = -1e-9
    code, msg = _code(lambda: check(model, dict(g, horizon_tan2=tan2)))
    assert code == E_INVALID_ARG and "horizon 3:" in msg and "negative" in msg, msg
    for key in ("diffuse_factor", "ground_factor"):                                                  # a factor is any finite number
        check(model, dict(g, **{key: -g[key]}))


def test_numbers_out_of_range_are_size_errors(model):
    S = int(model["n_surfaces"])
    g = good_shades(model)
    n = len(g["surface"])
    for bad in (-1, S, S + 12345):
        a = g["surface"].copy()
        a[4] = bad
        code, msg = _code(lambda: check(model, dict(g, surface=a)))
        assert code == E_SIZE and "shade 4:" in msg, msg
    for bad in (-2, 4, 2 ** 31 - 1):
        a = g["horizon"].copy()
        a[8] = bad
        code, msg = _code(lambda: check(model, dict(g, horizon=a)))
        assert code == E_SIZE and "shade 8:" in msg and "horizon" in msg, msg
    for bad in (-2, n, 2 ** 31 - 1):
        a = g["front_shade"].copy()
        a[41] = bad                                                                                  # (mode 1: its front is sky-driven)
        code, msg = _code(lambda: check(model, dict(g, front_shade=a)))
        assert code == E_SIZE and "surface 41:" in msg, msg
        a = g["back_shade"].copy()
        a[42] = bad
        code, msg = _code(lambda: check(model, dict(g, back_shade=a)))
        assert code == E_SIZE and "surface 42:" in msg, msg
        a = g["aperture_shade"].copy()
        a[10] = bad
        code, msg = _code(lambda: check(model, dict(g, aperture_shade=a)))
        assert code == E_SIZE and "aperture 10:" in msg, msg


def test_a_shade_needs_the_sides_sky_bit(model):
    g = good_shades(model)
    for key, q in (("front_shade", 42), ("front_shade", 40), ("back_shade", 41), ("back_shade", 40)):   # modes 2, 0, 1, 0
        a = g[key].copy()
        a[q] = 3
        code, msg = _code(lambda: check(model, dict(g, **{key: a})))
        assert code == E_SIZE and "surface %d:" % q in msg and "sky" in msg, msg
    code, msg = _code(lambda: check(model, g, sky_args=dict(good_sky(model), mode=None)))            # no mode bytes at all
    assert code == E_SIZE and "surface 1:" in msg, msg
    # a long-wave bit is not a solar bit
    sky_args = good_sky(model)
    sky_args["mode"] = (sky_args["mode"] << 2).astype(np.uint8)
    code, msg = _code(lambda: check(model, g, sky_args=sky_args))
    assert code == E_SIZE and "surface 1:" in msg, msg


def test_march_without_a_batch_is_an_invalid_argument(model):
    L = binding.load_library()
    s, _ = binding.make_series(**series(model))
    h, _ = binding.make_shades(**good_shades(model))
    failed = C.c_int32(123)
    none = (None,) * 5
    assert L.heat_batch_march_series_shaded(None, C.byref(s), None, C.byref(h), *none, *(None,) * 6, C.byref(failed)) == E_INVALID_ARG
    assert failed.value == -1


def test_the_wrapper_reads_the_shapes(model):
    h, keep = binding.make_shades(**good_shades(model))
    assert h.n_shades == 70 and h.n_horizons == 4 and keep["horizon_tan2"].shape == (4, 16) and keep["sh_horizon"].dtype == np.int32
    assert keep["front_shade"].dtype == np.int32 and keep["sh_surface"].dtype == np.int64
    h, keep = binding.make_shades()
    assert h.n_shades == 0 and h.n_horizons == 0 and not h.sh_surface and not h.horizon_tan2 and not h.front_shade
    h, keep = binding.make_shades(**{k: v for k, v in good_shades(model).items() if k not in shading.GEOMETRY})
    assert np.all(keep["overhang_depth"] == 0) and np.all(keep["fin_neg_gap"] == 0) and len(keep["fin_pos_depth"]) == 70
    for bad in (dict(width=np.ones(69)), dict(horizon_tan2=np.zeros((4, 15))), dict(normal=(np.zeros(70), np.zeros(70), np.zeros(2))),
                dict(horizon=np.zeros(3))):
        with pytest.raises(ValueError):
            binding.make_shades(**dict(good_shades(model), **bad))
    with pytest.raises(ValueError):
        check(model, dict(good_shades(model), front_shade=np.full(3, -1)))


# ---- the case builder of the GPU tests ----
@pytest.mark.parametrize("seed", [271, 272, 275])
def test_the_case_builder_covers_what_it_promises(seed):
    """shades_case asserts its pattern itself (partly sunlit pairs, the overhang's and the fins' regimes, exact zeros of us and c,
    a NaN, all 16 sectors and their boundaries, both horizon outcomes, a shared shade, a shaded back side); here it runs on the
    CPU, and its reference columns are finite where the clamps need them to be."""
    md, _ = mdl.ragged_mixed(700, Z=28, seed=1)
    rng = np.random.default_rng(seed)
    channel, call, ref, args, gains, shades = sc.shades_case(md, rng, sc.N_SUNS)
    ref_channel, ref_drives, f, p, ap_sum = sc.reference(md, channel, ref, args, gains, shades)
    assert f.shape == (sc.N_SUNS, sc.N_SHADES) and not np.isnan(ref_channel).any() and not np.isnan(p).any()
    plain = sc.reference(md, channel, ref, args, gains, {k: v for k, v in shades.items() if not k.endswith("_shade")})
    assert np.array_equal(plain[2], f) and not np.array_equal(plain[0], ref_channel) and not np.array_equal(plain[3], p)
    # shades in the consumers' own planes that shade nothing: the columns of the unshaded rule, to the bit
    clear = sc.reference(md, channel, ref, args, gains, sc.transparent_shades(md, args, gains))
    assert np.array_equal(clear[0], plain[0]) and np.array_equal(clear[3], plain[3]) and set(np.unique(clear[2])) == {0.0, 1.0}
    s, g, h = dict(args), dict(gains), dict(shades)
    binding.shades_check(md, h, s, g, weather=np.zeros((sc.N_SUNS, 1, 3)), n_sub=1, channel=channel,
                         **{name: chan for name, (chan, _) in call.items()})


def test_shades_check_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "shades_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "shades host check: all statuses as the header states them" in out.stdout
