"""Solar gains of a series on the host (include/heat_amd.h, heat_solar_gains / heat_solar_gains_check /
heat_batch_march_series_gains; heat_amd/solar_gains.py): the entry points are declared, exported and bound; the ctypes mirror
has the header's layout; the rule in numpy (solar_gains.transmitted / received — the reference of
tests/test_solar_gains_gpu.py) gives the hand-worked cases and conserves the power distribute_by_area shares out; every
refusal the header lists comes back with its code and names the aperture or the entry, before any device work; good, empty
and absent gains are accepted. heat_solar_gains_check — with the table builder and its verification — also runs under
AddressSanitizer / UBSan as a stand-alone program (tests/solar_gains_host_main.cpp) in a child process. No GPU needed.

Reference: the rule is this project's own (window-transmitted solar lives in another SIMPLE crate)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from heat_amd import binding, modeldict as mdl, sky, solar_gains
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_solar_gains_check", "heat_batch_march_series_gains")
E_INVALID_ARG, E_SIZE = -1, -4
N_STEPS = 4
FIELDS = ("n_apertures", "ap_surface", "ap_normal_x", "ap_normal_y", "ap_normal_z", "ap_tau_coef", "ap_tau_diffuse", "ap_scale",
          "ap_sum", "n_entries", "en_surface", "en_side", "en_aperture", "en_beam", "en_diffuse")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_solar_gains {" in header
    assert "heat_solar_gains_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_gains" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("SolarGains", "make_solar_gains", "solar_gains_check"))
    assert all(hasattr(solar_gains, n) for n in ("transmitted", "received", "distribute_by_area"))
    assert L.heat_amd_abi_version() == 1
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW)


def test_solar_gains_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = (["sizeof(heat_solar_gains)", "sizeof(heat_sky)", "sizeof(heat_sky_record)", "sizeof(heat_series)", "sizeof(heat_zone_loads)",
             "sizeof(heat_series_report)", "sizeof(heat_ideal_loads)"] + ["offsetof(heat_solar_gains, %s)" % f for f in FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    # (the structs beside it keep their sizes: the gains are a struct of their own)
    assert got == ([C.sizeof(binding.SolarGains), C.sizeof(binding.Sky), 64, C.sizeof(binding.Series), C.sizeof(binding.ZoneLoads),
                    C.sizeof(binding.Report), C.sizeof(binding.IdealLoads)] + [getattr(binding.SolarGains, f).offset for f in FIELDS])
    assert [f for f, _ in binding.SolarGains._fields_] == list(FIELDS)
    assert got[0] == 8 * len(FIELDS)


# ---- the rule in numpy: hand-worked cases ----
BEAM, DIFFUSE, GROUND = 800.0, 120.0, 45.0


def record(sun, beam=BEAM):
    return np.array([sun[0], sun[1], sun[2], beam, DIFFUSE, GROUND, 350.0, 420.0])


def test_a_window_facing_the_sun_at_normal_incidence():
    tau, scale = 0.75, 2.5
    el = math.radians(30.0)
    for n in ((0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)):
        pb, pd = solar_gains.transmitted(record(n), n, (tau, 0, 0, 0, 0, 0), 0.5, scale)
        assert pb == BEAM * tau * scale
        fs = 0.5 + 0.5 * n[2]
        assert pd == (DIFFUSE * fs + GROUND * (1.0 - fs)) * 0.5 * scale
    # at 60 degrees of incidence, a linear transmittance: tau(c) = 0.1 + 0.8 c
    pb, pd = solar_gains.transmitted(record((0.0, -math.cos(el), math.sin(el))), (0.0, 0.0, 1.0), (0.1, 0.8, 0, 0, 0, 0), 0.5, scale)
    c = math.sin(el)
    assert abs(pb - BEAM * c * (0.1 + 0.8 * c) * scale) <= 4 * np.spacing(pb) and pd == DIFFUSE * 0.5 * scale


def test_a_sun_behind_the_window_or_below_the_horizon_is_no_beam():
    coef = (0.7, 0.1, 0, 0, 0, 0)
    lit = solar_gains.transmitted(record((0.0, -0.6, 0.8)), (0.0, -1.0, 0.0), coef, 0.5, 2.0)
    behind = solar_gains.transmitted(record((0.0, 0.6, 0.8)), (0.0, -1.0, 0.0), coef, 0.5, 2.0)
    below = solar_gains.transmitted(record((0.6, 0.0, -0.8)), (0.0, 0.0, 1.0), coef, 0.5, 2.0)
    roof = solar_gains.transmitted(record((0.6, 0.0, 0.8)), (0.0, 0.0, 1.0), coef, 0.5, 2.0)
    assert lit[0] > 0 and behind[0] == 0.0 and behind[1] == lit[1]
    assert roof[0] > 0 and below[0] == 0.0 and below[1] == roof[1]
    nan = solar_gains.transmitted(record((np.nan, 0.0, 1.0)), (0.0, 0.0, 1.0), coef, 0.5, 2.0)
    assert nan[0] == 0.0 and nan[1] == roof[1]                     # c is NaN: c > 0 is false
    grazing = solar_gains.transmitted(record((1.0, 0.0, 0.0)), (0.0, 0.0, 1.0), coef, 0.5, 2.0)
    assert grazing[0] == 0.0                                       # c == 0 is no beam either


def test_the_polynomial_is_horner_in_the_cosine():
    rng = np.random.default_rng(3)
    n = 500
    coef = rng.uniform(-1.0, 1.0, (n, 6))
    c = rng.uniform(0.01, 1.0, n)
    pb, _ = solar_gains.transmitted(np.stack([c, np.zeros(n), np.zeros(n), np.ones(n)] + [np.zeros(n)] * 4, axis=1),
                                    (np.ones(n), np.zeros(n), np.zeros(n)), coef, np.zeros(n), np.ones(n))
    for i in range(n):                                             # beam 1, scale 1, n = x, sun = (c, 0, 0): Pb = c t(c)
        want = c[i] * np.polyval(coef[i, ::-1], c[i])
        # (6 terms, each product and sum within an ulp of values bounded by sum |coef| c^j)
        assert abs(pb[i] - want) <= 8 * np.spacing(np.abs(coef[i]).sum()), i
    # not clamped: the polynomial is the caller's
    pb, _ = solar_gains.transmitted(record((0.0, 0.0, 1.0)), (0.0, 0.0, 1.0), (-2.0, 0, 0, 0, 0, 0), 0.0, 1.0)
    assert pb == -2.0 * BEAM


def test_received_is_one_sequential_chain_per_receiver_in_the_callers_order():
    rng = np.random.default_rng(4)
    S, NA, NE = 7, 5, 400
    pb, pd = rng.uniform(0, 1e3, (3, NA)), rng.uniform(-50, 1e3, (3, NA))
    surf, side, ap = rng.integers(0, S - 1, NE), rng.integers(0, 2, NE), rng.integers(0, NA, NE)
    eb, ed = rng.uniform(0, 1, NE), rng.uniform(0, 1, NE)
    v, has = solar_gains.received(pb, pd, surf, side, ap, eb, ed, S)
    assert v.shape == (3, 2, S) and has.shape == (2, S) and not has[:, S - 1].any() and np.all(v[:, :, S - 1] == 0.0)
    want = np.zeros((3, 2, S))
    for i in range(NE):
        for k in range(3):
            x = want[k, side[i], surf[i]] + eb[i] * pb[k, ap[i]]
            want[k, side[i], surf[i]] = x + ed[i] * pd[k, ap[i]]
    assert np.array_equal(v, want)
    assert np.array_equal(has, (want != 0).any(axis=0))


# ---- conservation with distribute_by_area ----
def test_distribute_by_area_conserves_the_transmitted_power():
    md, _ = mdl.rooms_with_windows(900, Z=60, seed=6)
    S = int(md["n_surfaces"])
    windows = np.flatnonzero(np.diff(md["node_offset"]) == 4)      # the double glazing of the model
    assert len(windows) > 100
    en = solar_gains.distribute_by_area(md, windows)
    area = md["area"]
    n = len(en["en_surface"])
    # for each aperture the shares times the receivers' areas sum to 1
    total = np.zeros(len(windows))
    np.add.at(total, en["en_aperture"], en["en_beam"] * area[en["en_surface"]])
    assert np.all(np.abs(total - 1.0) <= 1e-13) and np.array_equal(en["en_beam"], en["en_diffuse"])
    # every receiver faces the zone behind its window, and every such side is a receiver
    zone = np.where(en["en_side"] == 1, md["back_zone"][en["en_surface"]], md["front_zone"][en["en_surface"]])
    kind = np.where(en["en_side"] == 1, md["back_kind"][en["en_surface"]], md["front_kind"][en["en_surface"]])
    assert np.all(kind == mdl.SPACE) and np.array_equal(zone, md["back_zone"][windows][en["en_aperture"]])
    assert n == sum(int(((md["back_kind"] == mdl.SPACE) & (md["back_zone"] == z)).sum() + ((md["front_kind"] == mdl.SPACE) & (md["front_zone"] == z)).sum())
                    for z in md["back_zone"][windows])
    rng = np.random.default_rng(8)
    n_steps = 24
    sun = sky.sun_direction(172, 24.0 * np.arange(n_steps) / n_steps, math.radians(48.0))
    rec = np.concatenate([sun, np.stack([np.where(sun[:, 2] > 0, 800.0, 0.0), 60.0 + 140.0 * np.maximum(sun[:, 2], 0), np.full(n_steps, 40.0),
                                         np.full(n_steps, 350.0), np.full(n_steps, 420.0)], axis=1)], axis=1)
    pb, pd = solar_gains.transmitted(rec[:, None, :], (md["normal_x"][windows], md["normal_y"][windows], md["cos_tilt"][windows]),
                                     np.concatenate([rng.uniform(0.3, 0.8, (len(windows), 1)), rng.uniform(-0.05, 0.05, (len(windows), 5))], axis=1),
                                     rng.uniform(0.3, 0.7, len(windows)), area[windows])
    assert (pb > 0).any() and (pb == 0).any()
    v, has = solar_gains.received(pb, pd, n_surfaces=S, **en)
    a2 = np.stack([area, area])
    for k in range(n_steps):
        got = (v[k] * a2).sum()
        want = (pb[k] + pd[k]).sum()
        terms = (np.abs(en["en_beam"] * pb[k][en["en_aperture"]]) + np.abs(en["en_diffuse"] * pd[k][en["en_aperture"]])) * area[en["en_surface"]]
        assert abs(got - want) <= n * 2.0 ** -52 * terms.sum(), (k, got, want)


# ---- heat_solar_gains_check ----
@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


def series(md, **more):
    S = int(md["n_surfaces"])
    chan = np.full(S, -1, np.int32)
    return dict(dict(weather=np.zeros((N_STEPS, 2, 3)), n_sub=2, channel=np.zeros((N_STEPS, 3)), solar_front=chan, solar_back=chan), **more)


def good_sky(md, n_sites=1, mode=None):
    return dict(record=np.random.default_rng(1).random((N_STEPS, n_sites, 8)), mode=mode)


def good_gains(md, n_apertures=12):
    S = int(md["n_surfaces"])
    rng = np.random.default_rng(2)
    windows = np.arange(n_apertures) * 16 + 3
    en = solar_gains.distribute_by_area(md, windows)
    return dict(en, ap_surface=windows, ap_normal=tuple(rng.normal(size=(3, n_apertures))), ap_tau_coef=rng.uniform(-1, 1, (n_apertures, 6)),
                ap_tau_diffuse=rng.random(n_apertures), ap_scale=rng.uniform(1, 5, n_apertures))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def _raw(md, gains, sky_args="good", series_args=None, **fields):
    """heat_solar_gains_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**(series_args or series(md)))
    k, kkeep = binding.make_sky(**binding._sky_for_gains(good_sky(md) if sky_args == "good" else sky_args, None, int(md["n_surfaces"])))
    g, gkeep = binding.make_solar_gains(**gains)
    for name, v in fields.items():
        setattr(g, name, v)
    rc = L.heat_solar_gains_check(C.byref(desc), 1, C.byref(s), C.byref(k) if sky_args is not None else None, C.byref(g))
    return rc, L.heat_last_error().decode()


def test_good_empty_and_absent_gains_are_accepted(model):
    binding.solar_gains_check(model, good_gains(model), good_sky(model), **series(model))
    binding.solar_gains_check(model, good_gains(model), good_sky(model, 3), n_sites=3, **series(model, weather=np.zeros((N_STEPS, 2, 3, 3))))
    binding.solar_gains_check(model, None, good_sky(model), **series(model))                       # gains == NULL
    binding.solar_gains_check(model, {}, good_sky(model), **series(model))                         # neither an aperture nor an entry
    assert _raw(model, {}, None)[0] == 0                                                           # ... which needs no sky
    assert _raw(model, good_gains(model), ap_sum=None)[0] == 0                                     # ap_sum may be NULL
    g = good_gains(model)
    only = {k: v for k, v in g.items() if k.startswith("ap_")}
    binding.solar_gains_check(model, only, good_sky(model), **series(model))                       # apertures nobody receives from
    # n_steps == 0 needs no records
    assert _raw(model, g, dict(record=None), series(model, weather=np.zeros((0, 3)), channel=None))[0] == 0
    # the series' and the sky's own refusals come first
    S = int(model["n_surfaces"])
    code, msg = _code(lambda: binding.solar_gains_check(model, g, good_sky(model), **series(model, solar_front=np.full(S, 3, np.int32))))
    assert code == E_SIZE and "surface 0" in msg, msg
    code, msg = _code(lambda: binding.solar_gains_check(model, g, good_sky(model, mode=np.full(S, 16, np.uint8)), **series(model)))
    assert code == E_INVALID_ARG and "surface 0" in msg, msg


def test_negative_counts_and_null_arrays_are_invalid_arguments(model):
    g = good_gains(model)
    rc, msg = _raw(model, g, n_apertures=-1)
    assert rc == E_INVALID_ARG and "aperture" in msg and "n_apertures -1" in msg, msg
    rc, msg = _raw(model, g, n_entries=-3)
    assert rc == E_INVALID_ARG and "entry" in msg and "n_entries -3" in msg, msg
    for field in ("ap_surface", "ap_normal_x", "ap_normal_y", "ap_normal_z", "ap_tau_coef", "ap_tau_diffuse", "ap_scale"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "aperture 0" in msg and field in msg, (field, msg)
    for field in ("en_surface", "en_side", "en_aperture", "en_beam", "en_diffuse"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "entry 0" in msg and field in msg, (field, msg)
    rc, msg = _raw(model, g, None)
    assert rc == E_INVALID_ARG and "aperture 0" in msg and "sky is NULL" in msg, msg
    rc, msg = _raw(model, g, dict(record=None))
    assert rc == E_INVALID_ARG and "aperture 0" in msg and "sky->record is NULL" in msg, msg


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_values_that_are_not_finite_are_refused(model, bad):
    g = good_gains(model)
    for axis in range(3):
        normal = [a.copy() for a in g["ap_normal"]]
        normal[axis][7] = bad
        code, msg = _code(lambda: binding.solar_gains_check(model, dict(g, ap_normal=normal), good_sky(model), **series(model)))
        assert code == E_INVALID_ARG and "aperture 7:" in msg and "normal_" + "xyz"[axis] in msg, msg
    for j in range(6):
        coef = g["ap_tau_coef"].copy()
        coef[5, j] = bad
        code, msg = _code(lambda: binding.solar_gains_check(model, dict(g, ap_tau_coef=coef), good_sky(model), **series(model)))
        assert code == E_INVALID_ARG and "aperture 5:" in msg and "tau_coef[%d]" % j in msg, msg
    for name, word in (("ap_tau_diffuse", "tau_diffuse"), ("ap_scale", "scale")):
        a = g[name].copy()
        a[11] = bad
        code, msg = _code(lambda: binding.solar_gains_check(model, dict(g, **{name: a}), good_sky(model), **series(model)))
        assert code == E_INVALID_ARG and "aperture 11:" in msg and word in msg, msg
    for name in ("en_beam", "en_diffuse"):
        a = g[name].copy()
        a[41] = bad
        code, msg = _code(lambda: binding.solar_gains_check(model, dict(g, **{name: a}), good_sky(model), **series(model)))
        assert code == E_INVALID_ARG and "entry 41:" in msg, msg


def test_a_side_byte_above_1_is_refused(model):
    g = good_gains(model)
    for bad in (2, 3, 255):
        side = g["en_side"].copy()
        side[19] = bad
        code, msg = _code(lambda: binding.solar_gains_check(model, dict(g, en_side=side), good_sky(model), **series(model)))
        assert code == E_INVALID_ARG and "entry 19:" in msg, msg


def test_indices_out_of_range_are_size_errors(model):
    S = int(model["n_surfaces"])
    g = good_gains(model)
    NA = len(g["ap_surface"])
    for bad in (-1, S, S + 12345):
        a = g["ap_surface"].copy()
        a[4] = bad
        code, msg = _code(lambda: binding.solar_gains_check(model, dict(g, ap_surface=a), good_sky(model), **series(model)))
        assert code == E_SIZE and "aperture 4:" in msg, msg
        a = g["en_surface"].copy()
        a[33] = bad
        code, msg = _code(lambda: binding.solar_gains_check(model, dict(g, en_surface=a), good_sky(model), **series(model)))
        assert code == E_SIZE and "entry 33:" in msg, msg
    for bad in (-1, NA, 2 ** 31 - 1):
        a = g["en_aperture"].copy()
        a[28] = bad
        code, msg = _code(lambda: binding.solar_gains_check(model, dict(g, en_aperture=a), good_sky(model), **series(model)))
        assert code == E_SIZE and "entry 28:" in msg, msg


def test_an_input_has_one_source(model):
    S = int(model["n_surfaces"])
    g = good_gains(model)
    i = 37
    q, side = int(g["en_surface"][i]), int(g["en_side"][i])
    first = int(np.flatnonzero((g["en_surface"] == q) & (g["en_side"] == side))[0])
    name = ("solar_front", "solar_back")[side]
    chan = np.full(S, -1, np.int32)
    chan[q] = 2
    code, msg = _code(lambda: binding.solar_gains_check(model, g, good_sky(model), **series(model, **{name: chan})))
    assert code == E_SIZE and "entry %d:" % first in msg and "channel 2" in msg, msg
    other = ("solar_back", "solar_front")[side]                                                     # the other side's channel is its own
    if not ((g["en_surface"] == q) & (g["en_side"] == 1 - side)).any():
        binding.solar_gains_check(model, g, good_sky(model), **series(model, **{other: chan}))
    mode = np.zeros(S, np.uint8)
    mode[q] = 1 << side
    code, msg = _code(lambda: binding.solar_gains_check(model, g, good_sky(model, mode=mode), **series(model)))
    assert code == E_SIZE and "entry %d:" % first in msg and "sky" in msg, msg
    mode[q] = 4 << side                                                                             # the long-wave bit of the same side is free
    binding.solar_gains_check(model, g, good_sky(model, mode=mode), **series(model))


def test_march_without_a_batch_is_an_invalid_argument(model):
    """What heat_batch_march_series_gains can answer without a batch, and so without a device: good gains or none, a NULL batch
    is refused and failed_step reset. That bad gains are refused BEFORE any device work needs a batch: the GPU test
    test_bad_gains_and_sharded_batches_are_refused_by_the_march finds the device state untouched behind every refusal."""
    L = binding.load_library()
    s, _ = binding.make_series(**series(model))
    k, _ = binding.make_sky(**binding._sky_for_gains(good_sky(model), None, int(model["n_surfaces"])))
    g, _ = binding.make_solar_gains(**good_gains(model))
    failed = C.c_int32(123)
    none = (None,) * 7
    assert L.heat_batch_march_series_gains(None, C.byref(s), C.byref(k), C.byref(g), *none, C.byref(failed)) == E_INVALID_ARG
    assert failed.value == -1
    assert L.heat_batch_march_series_gains(None, None, None, None, *none, None) == E_INVALID_ARG


def test_the_wrapper_reads_the_shapes(model):
    g, keep = binding.make_solar_gains(**good_gains(model))
    NA, NE = g.n_apertures, g.n_entries
    assert NA == 12 and keep["ap_tau_coef"].shape == (NA, 6) and keep["en_side"].dtype == np.uint8 and keep["ap_sum"].shape == (NA,)
    assert keep["en_aperture"].dtype == np.int32 and keep["en_surface"].shape == (NE,) and np.all(keep["ap_sum"] == 0)
    g, keep = binding.make_solar_gains()
    assert g.n_apertures == 0 and g.n_entries == 0 and not g.ap_surface and not g.en_beam and not g.ap_sum
    resume = np.arange(12.0)
    g, keep = binding.make_solar_gains(**dict(good_gains(model), ap_sum=resume))
    assert np.array_equal(keep["ap_sum"], resume) and keep["ap_sum"] is not resume
    for bad in (dict(ap_tau_coef=np.zeros((12, 5))), dict(ap_scale=np.zeros(11)), dict(en_beam=np.zeros(3)), dict(ap_sum=np.zeros(13)),
                dict(ap_normal=(np.zeros(12), np.zeros(12), np.zeros(2)))):
        with pytest.raises(ValueError):
            binding.make_solar_gains(**dict(good_gains(model), **bad))


def test_solar_gains_check_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "solar_gains_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "solar gains host check: all statuses as the header states them" in out.stdout
