"""Room radiation of a series on the host (include/heat_amd.h, heat_room_radiation / heat_room_radiation_check /
heat_batch_march_series_radiation; heat_amd/room_radiation.py): the entry points are declared, exported and bound; the ctypes
mirror has the header's layout; the rule in numpy (room_radiation.emitted / irradiance — the reference of
tests/test_room_radiation_gpu.py) gives the hand-worked cases; every refusal the header lists comes back with its code and
names the receiver or entry, before any device work; the case builder of the GPU tests covers what it promises.
heat_room_radiation_check also runs under AddressSanitizer / UBSan as a stand-alone program
(tests/room_radiation_host_main.cpp) in a child process. No GPU needed.

Reference: the rule is this project's own (the reference's harness feeds EnergyPlus' long-wave columns)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from heat_amd import binding, modeldict as mdl, room_radiation as rrm
import room_radiation_cases as rc
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_room_radiation_check", "heat_batch_march_series_radiation")
E_INVALID_ARG, E_SIZE = -1, -4
N_STEPS = 4
FIELDS = ("n_receivers", "rc_surface", "rc_side", "sum_irradiance", "n_entries", "en_receiver", "en_surface", "en_side", "en_chan", "en_factor")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_room_radiation {" in header
    assert "heat_room_radiation_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_radiation" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("RoomRadiation", "make_room_radiation", "room_radiation_check"))
    assert all(hasattr(rrm, n) for n in ("emitted", "irradiance", "exchange_by_area"))
    assert L.heat_amd_abi_version() == 1 and re.search(r"#define\s+HEAT_AMD_ABI_VERSION\s+1\b", header)
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW) and "pub struct HeatRoomRadiation" in rust


def test_room_radiation_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = (["sizeof(heat_room_radiation)", "sizeof(heat_series)", "sizeof(heat_sky)", "sizeof(heat_solar_gains)", "sizeof(heat_air_paths)",
             "sizeof(heat_shades)", "sizeof(heat_sky_record)"] + ["offsetof(heat_room_radiation, %s)" % f for f in FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    # (the structs beside it keep their sizes: the radiation is a struct of its own)
    assert got == ([C.sizeof(binding.RoomRadiation), C.sizeof(binding.Series), C.sizeof(binding.Sky), C.sizeof(binding.SolarGains),
                    C.sizeof(binding.AirPaths), C.sizeof(binding.Shades), 64] + [getattr(binding.RoomRadiation, f).offset for f in FIELDS])
    assert [f for f, _ in binding.RoomRadiation._fields_] == list(FIELDS)
    assert got[0] == 8 * len(FIELDS)


# ---- the rule in numpy: hand-worked cases ----
def ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def test_an_isothermal_room_radiates_at_its_own_temperature():
    """Factors that sum to 1 over faces at one temperature: v = sigma T^4 up to the rounding of the sum, and the radiant
    temperature the device makes of it is T within 2 ulp. The ulp is that of the absolute temperature, the number the two
    square roots yield: subtracting 273.15 is exact to half an ulp of that magnitude and no better (at T = 0 C an ulp of T
    itself does not exist), so sqrt(sqrt(v / sigma)) is held to 2 ulp of T + 273.15 and the Celsius value to the same distance."""
    rng = np.random.default_rng(9)
    for T in (20.0, -12.5, 0.0, 35.25, 61.0) + tuple(rng.uniform(-40.0, 80.0, 40)):
        for factor in ([0.25, 0.25, 0.25, 0.25], [0.5, 0.125, 0.125, 0.25], [1.0], [0.3, 0.2, 0.1, 0.15, 0.25]):
            n = len(factor)
            E = rrm.emitted(np.full((2, n), T))
            v = rrm.irradiance(E, None, 1, np.zeros(n, np.int64), np.arange(n), np.arange(n) % 2, factor)
            assert v.shape == (1,)
            assert ulps(np.sqrt(np.sqrt(v[0] / rrm.SIGMA)), T + 273.15) <= 2, (T, factor)
            assert abs(float(rrm.rad_temperature(v[0])) - T) <= 2 * np.spacing(T + 273.15), (T, factor)


def test_two_faces_at_20_and_10_degrees():
    e20, e10 = 5.670374419e-8 * 293.15 ** 4, 5.670374419e-8 * 283.15 ** 4
    E = rrm.emitted(np.array([[20.0, 10.0], [10.0, 20.0]]))              # [side, surface]
    assert abs(E[0, 0] - e20) <= 1e-12 * e20 and abs(E[0, 1] - e10) <= 1e-12 * e10 and 418.7 < E[0, 0] < 418.8 and 364.4 < E[0, 1] < 364.6
    # written out: tk * tk, squared, times sigma — one rounded operation each
    t2 = (20.0 + 273.15) * (20.0 + 273.15)
    assert E[0, 0] == 5.670374419e-8 * (t2 * t2)
    # receiver 0 sees 0.75 of the front of surface 0 (20 C) and 0.25 of the front of surface 1 (10 C); receiver 1 the reverse
    v = rrm.irradiance(E, None, 2, [0, 0, 1, 1], [0, 1, 0, 1], [0, 0, 0, 0], [0.75, 0.25, 0.25, 0.75])
    assert v[0] == (0.0 + 0.75 * E[0, 0]) + 0.25 * E[0, 1] and v[1] == (0.0 + 0.25 * E[0, 0]) + 0.75 * E[0, 1]
    assert abs(v[0] - (0.75 * e20 + 0.25 * e10)) < 1e-10 and 405.1 < v[0] < 405.3
    # the back of surface 0 is at 10 C: the side byte picks the last node
    assert rrm.irradiance(E, None, 1, [0], [0], [1], [1.0])[0] == E[1, 0] == E[0, 1]
    # a gain array of the series multiplies last; a receiver without entries gets 0.0; a NaN temperature propagates
    assert rrm.irradiance(E, None, 2, [0], [0], [0], [0.5], gain=[2.0, 3.0]).tolist() == [(0.5 * E[0, 0]) * 2.0, 0.0]
    assert np.isnan(rrm.irradiance(rrm.emitted(np.array([[np.nan], [1.0]])), None, 1, [0, 0], [0, 0], [1, 0], [0.5, 0.5])[0])


def test_a_channel_entry_adds_factor_times_the_rows_value():
    E = rrm.emitted(np.array([[20.0], [10.0]]))
    row = np.array([7.0, 120.0, 33.0])
    v = rrm.irradiance(E, row, 2, [0, 0, 1], [0, -1, -1], [0, 0, 0], [1.0, 0.25, 2.0], en_chan=[-1, 1, 2])
    assert v[0] == 1.0 * E[0, 0] + 0.25 * 120.0 and v[1] == 2.0 * 33.0
    # a table of rows at once: one result per step
    rows = np.array([[0.0, 100.0, 0.0], [0.0, 200.0, 1.0]])
    v = rrm.irradiance(E, rows, 2, [0, 0, 1], [0, -1, -1], [0, 0, 0], [1.0, 0.25, 2.0], en_chan=[-1, 1, 2])
    assert v.shape == (2, 2) and v[:, 0].tolist() == [E[0, 0] + 25.0, E[0, 0] + 50.0] and v[:, 1].tolist() == [0.0, 2.0]
    assert np.isnan(rrm.irradiance(E, np.array([np.nan]), 1, [0], [-1], [0], [1.0], en_chan=[0])[0])


def test_the_callers_order_of_the_entries_matters():
    """Three terms chosen to round differently: 1e16 + 1 + 1 loses both ones one at a time; 1 + 1 + 1e16 keeps their sum."""
    E = np.array([[1e16, 1.0, 1.0], [0.0, 0.0, 0.0]])
    ones = [1.0, 1.0, 1.0]
    a = rrm.irradiance(E, None, 1, [0, 0, 0], [0, 1, 2], [0, 0, 0], ones)[0]
    b = rrm.irradiance(E, None, 1, [0, 0, 0], [1, 2, 0], [0, 0, 0], ones)[0]
    assert a == 1e16 and b == 1e16 + 2.0 and a != b
    # the entries of two receivers interleaved, each in its own order
    v = rrm.irradiance(E, None, 2, [1, 0, 1, 0, 0, 1], [1, 0, 2, 1, 2, 0], [0] * 6, [1.0] * 6)
    assert v.tolist() == [a, b]


def test_exchange_by_area_rows_sum_to_one_and_are_reciprocal():
    md, _ = mdl.rooms_with_windows(300, Z=20, seed=4)
    S = int(md["n_surfaces"])
    for weight in (None, np.asarray(md["front_emissivity"]), np.stack([md["front_emissivity"], md["back_emissivity"]])):
        ex = rrm.exchange_by_area(md, weight)
        R = len(ex["rc_surface"])
        faces = int((np.asarray(md["front_kind"]) == mdl.SPACE).sum() + (np.asarray(md["back_kind"]) == mdl.SPACE).sum())
        assert R == faces and len(np.unique(ex["rc_side"].astype(np.int64) * S + ex["rc_surface"])) == R
        rows = np.zeros(R)
        np.add.at(rows, ex["en_receiver"], ex["en_factor"])
        assert np.abs(rows - 1.0).max() <= 1e-15 * max(1, np.bincount(ex["en_receiver"]).max())
        # every receiver sees its whole room, itself included, and nothing else
        zone = np.where(ex["rc_side"] == 1, np.asarray(md["back_zone"])[ex["rc_surface"]], np.asarray(md["front_zone"])[ex["rc_surface"]])
        key = ex["rc_side"].astype(np.int64) * S + ex["rc_surface"]
        index = {int(k): r for r, k in enumerate(key)}
        seen = np.array([index[int(k)] for k in ex["en_side"].astype(np.int64) * S + ex["en_surface"]])
        assert np.array_equal(zone[seen], zone[ex["en_receiver"]]) and (seen == ex["en_receiver"]).sum() == R
        assert np.array_equal(np.bincount(ex["en_receiver"]), np.bincount(zone)[zone])
        # reciprocity: w_i A_i F_ij = w_j A_j F_ji (w = 1 without weights)
        w = np.ones((2, S)) if weight is None else np.broadcast_to(weight, (2, S))
        wa = w[ex["rc_side"].astype(np.int64), ex["rc_surface"]] * np.asarray(md["area"])[ex["rc_surface"]]
        F = np.zeros((R, R))
        F[ex["en_receiver"], seen] = ex["en_factor"]
        lhs = wa[:, None] * F
        assert np.abs(lhs - lhs.T).max() <= 1e-15 * wa.max() and (F > 0).any()
        binding.room_radiation_check(md, ex, **series(md))
    assert np.abs(rows - 1.0).max() <= 1e-15


# ---- heat_room_radiation_check ----
@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


def series(md, **more):
    S = int(md["n_surfaces"])
    chan = np.full(S, -1, np.int32)
    return dict(dict(weather=np.zeros((N_STEPS, 2, 3)), n_sub=2, channel=np.zeros((N_STEPS, 3)), ir_front=chan, ir_back=chan), **more)


def good_radiation(md, n=90, m=400):
    S = int(md["n_surfaces"])
    rng = np.random.default_rng(3)
    key = rng.permutation(2 * S)[:n]
    surface = rng.integers(-1, S, m)
    return dict(rc_surface=key % S, rc_side=(key // S).astype(np.uint8), en_receiver=rng.integers(0, n, m), en_surface=surface,
                en_side=rng.integers(0, 2, m).astype(np.uint8), en_factor=rng.uniform(-0.5, 1.5, m),
                en_chan=np.where(surface < 0, rng.integers(0, 3, m), -1).astype(np.int32))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def check(md, radiation, sky=None, **more):
    binding.room_radiation_check(md, radiation, sky, **series(md, **more))


def _raw(md, radiation, **fields):
    """heat_room_radiation_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**series(md))
    rr, rkeep = binding.make_room_radiation(**radiation)
    for name, v in fields.items():
        setattr(rr, name, v)
    rc_ = L.heat_room_radiation_check(C.byref(desc), 1, C.byref(s), None, C.byref(rr))
    return rc_, L.heat_last_error().decode()


def test_good_empty_and_absent_radiation_are_accepted(model):
    g = good_radiation(model)
    assert (g["en_surface"] < 0).any() and (g["en_factor"] < 0).any()
    check(model, g)
    check(model, None)
    check(model, {})
    check(model, dict(g, sum_irradiance=np.arange(90.0)))
    check(model, {k: v for k, v in g.items() if k.startswith("rc_")})                               # receivers without entries
    surfaces_only = dict(g, en_surface=np.abs(g["en_surface"]))
    check(model, {k: v for k, v in surfaces_only.items() if k != "en_chan"})                        # en_chan NULL
    S = int(model["n_surfaces"])
    sky = dict(record=np.random.default_rng(1).random((N_STEPS, 1, 8)), mode=np.where(np.isin(np.arange(S), g["rc_surface"]), 3, 15))
    check(model, g, sky)                                                                            # solar bits are not long-wave bits
    binding.room_radiation_check(model, g, dict(sky, record=np.zeros((N_STEPS, 3, 8))), n_sites=3,
                                 **series(model, weather=np.zeros((N_STEPS, 2, 3, 3))))
    # the series' and the sky's own refusals come first
    code, msg = _code(lambda: check(model, g, solar_front=np.full(S, 5, np.int32)))
    assert code == E_SIZE and "surface 0" in msg, msg
    code, msg = _code(lambda: check(model, g, dict(sky, mode=np.full(S, 16))))
    assert code == E_INVALID_ARG and "surface 0" in msg, msg


def test_negative_counts_and_null_arrays_are_invalid_arguments(model):
    g = good_radiation(model)
    rc_, msg = _raw(model, g, n_receivers=-1)
    assert rc_ == E_INVALID_ARG and "receiver" in msg and "n_receivers -1" in msg, msg
    rc_, msg = _raw(model, g, n_entries=-3)
    assert rc_ == E_INVALID_ARG and "entry" in msg and "n_entries -3" in msg, msg
    for field in ("rc_surface", "rc_side"):
        rc_, msg = _raw(model, g, **{field: None})
        assert rc_ == E_INVALID_ARG and "receiver 0" in msg and field in msg, (field, msg)
    for field in ("en_receiver", "en_surface", "en_side", "en_factor"):
        rc_, msg = _raw(model, g, **{field: None})
        assert rc_ == E_INVALID_ARG and "entry 0" in msg and field in msg, (field, msg)
    assert _raw(model, g, sum_irradiance=None)[0] == 0                                              # nullable
    first = int(np.flatnonzero(g["en_surface"] < 0)[0])
    rc_, msg = _raw(model, g, en_chan=None)                                                         # ... with channel entries present
    assert rc_ == E_INVALID_ARG and "entry %d:" % first in msg and "en_chan" in msg, msg


def test_side_bytes_factors_and_stray_channels_are_invalid_arguments(model):
    g = good_radiation(model)
    side = g["rc_side"].copy()
    side[17] = 2
    code, msg = _code(lambda: check(model, dict(g, rc_side=side)))
    assert code == E_INVALID_ARG and "receiver 17:" in msg and "side 2" in msg, msg
    i = int(np.flatnonzero(g["en_surface"] >= 0)[5])
    side = g["en_side"].copy()
    side[i] = 9
    code, msg = _code(lambda: check(model, dict(g, en_side=side)))
    assert code == E_INVALID_ARG and "entry %d:" % i in msg and "side 9" in msg, msg
    for bad in (np.nan, np.inf, -np.inf):
        f = g["en_factor"].copy()
        f[123] = bad
        code, msg = _code(lambda: check(model, dict(g, en_factor=f)))
        assert code == E_INVALID_ARG and "entry 123:" in msg and "not finite" in msg, msg
    chan = g["en_chan"].copy()
    chan[i] = 0
    code, msg = _code(lambda: check(model, dict(g, en_chan=chan)))
    assert code == E_INVALID_ARG and "entry %d:" % i in msg and "channel 0" in msg, msg


def test_numbers_out_of_range_are_size_errors(model):
    S = int(model["n_surfaces"])
    g = good_radiation(model)
    for bad in (-1, S, S + 12345, 2 ** 62):
        a = g["rc_surface"].copy()
        a[4] = bad
        code, msg = _code(lambda: check(model, dict(g, rc_surface=a)))
        assert code == E_SIZE and "receiver 4:" in msg, msg
    i = int(np.flatnonzero(g["en_surface"] >= 0)[7])
    for bad in (-2, S, S + 12345, -2 ** 62):
        a = g["en_surface"].copy()
        a[i] = bad
        code, msg = _code(lambda: check(model, dict(g, en_surface=a)))
        assert code == E_SIZE and "entry %d:" % i in msg and "[-1, %d)" % S in msg, msg
    for bad in (-1, 90, 2 ** 40):
        a = g["en_receiver"].copy()
        a[250] = bad
        code, msg = _code(lambda: check(model, dict(g, en_receiver=a)))
        assert code == E_SIZE and "entry 250:" in msg and "[0, 90)" in msg, msg
    j = int(np.flatnonzero(g["en_surface"] < 0)[2])
    for bad in (-1, -5, 3, 2 ** 31 - 1):
        a = g["en_chan"].copy()
        a[j] = bad
        code, msg = _code(lambda: check(model, dict(g, en_chan=a)))
        assert code == E_SIZE and "entry %d:" % j in msg and "channel" in msg and "[0, 3)" in msg, msg


def test_a_receiver_is_listed_once_and_its_input_has_no_other_source(model):
    S = int(model["n_surfaces"])
    g = good_radiation(model)
    # the same (surface, side) twice; the other side of the same surface is another receiver
    a, side = g["rc_surface"].copy(), g["rc_side"].copy()
    a[60], side[60] = a[11], side[11]
    code, msg = _code(lambda: check(model, dict(g, rc_surface=a, rc_side=side)))
    assert code == E_SIZE and "receiver 60:" in msg and "receiver 11 already" in msg, msg
    taken = set(zip(g["rc_surface"].tolist(), g["rc_side"].tolist()))
    if (int(a[11]), 1 - int(side[11])) not in taken:
        side[60] = 1 - side[11]
        check(model, dict(g, rc_surface=a, rc_side=side))
    # a channel on the receiver's own input; a channel on its other side is none of its business
    q, d = int(g["rc_surface"][33]), int(g["rc_side"][33])
    names = ("ir_front", "ir_back")
    chan = np.full(S, -1, np.int32)
    chan[q] = 2
    code, msg = _code(lambda: check(model, g, **{names[d]: chan}))
    assert code == E_SIZE and "receiver 33:" in msg and "channel 2" in msg and "one source" in msg, msg
    if (q, 1 - d) not in taken:
        check(model, g, **{names[1 - d]: chan})
    # the sky's long-wave bit of that side; its solar bit and the other side's long-wave bit are not
    rec = np.random.default_rng(1).random((N_STEPS, 1, 8))
    mode = np.zeros(S, np.uint8)
    mode[q] = 4 << d
    code, msg = _code(lambda: check(model, g, dict(record=rec, mode=mode)))
    assert code == E_SIZE and "receiver 33:" in msg and "sky" in msg and "mode bit %d" % (2 + d) in msg, msg
    mode[q] = 1 << d
    check(model, g, dict(record=rec, mode=mode))
    if (q, 1 - d) not in taken:
        mode[q] = 4 << (1 - d)
        check(model, g, dict(record=rec, mode=mode))
    # both: the input has two sources before the radiation adds a third — the sky's own refusal comes first and names the surface
    mode[q] = 4 << d
    code, msg = _code(lambda: check(model, g, dict(record=rec, mode=mode), **{names[d]: chan}))
    assert code == E_SIZE and "surface %d:" % q in msg and "one source" in msg, msg
    # an ir_own_face bit on a receiver is refused by the series already: it needs a channel
    own = np.zeros(S, np.uint8)
    own[q] = 1 << d
    code, msg = _code(lambda: check(model, g, ir_own_face=own))
    assert code != 0 and "surface %d" % q in msg, msg


def test_march_without_a_batch_is_an_invalid_argument(model):
    L = binding.load_library()
    s, _ = binding.make_series(**series(model))
    rr, _ = binding.make_room_radiation(**good_radiation(model))
    failed = C.c_int32(123)
    assert L.heat_batch_march_series_radiation(None, C.byref(s), *(None,) * 13, C.byref(rr), None, C.byref(failed)) == E_INVALID_ARG
    assert failed.value == -1


def test_the_wrapper_reads_the_shapes(model):
    g = good_radiation(model)
    rr, keep = binding.make_room_radiation(**g)
    assert rr.n_receivers == 90 and rr.n_entries == 400 and keep["rc_side"].dtype == np.uint8 and keep["en_chan"].dtype == np.int32
    assert keep["en_receiver"].dtype == np.int64 and keep["sum_irradiance"].shape == (90,) and np.all(keep["sum_irradiance"] == 0)
    rr, keep = binding.make_room_radiation()
    assert rr.n_receivers == 0 and rr.n_entries == 0 and not rr.rc_surface and not rr.en_factor and not rr.en_chan and not rr.sum_irradiance
    rr, keep = binding.make_room_radiation(**{k: v for k, v in g.items() if k != "en_chan"})
    assert not rr.en_chan
    given = np.arange(90.0)
    rr, keep = binding.make_room_radiation(**dict(g, sum_irradiance=given))
    assert np.array_equal(keep["sum_irradiance"], given) and keep["sum_irradiance"] is not given    # (it is copied)
    for bad in (dict(rc_side=np.zeros(89, np.uint8)), dict(en_factor=np.ones(399)), dict(en_chan=np.zeros(3)), dict(sum_irradiance=np.zeros(91)),
                dict(en_surface=np.zeros(401))):
        with pytest.raises(ValueError):
            binding.make_room_radiation(**dict(g, **bad))
    with pytest.raises(ValueError):
        check(model, g, ir_front=np.full(3, -1, np.int32))


# ---- the case builder of the GPU tests ----
@pytest.mark.parametrize("seed", [331, 332, 335])
def test_the_case_builder_covers_what_it_promises(seed):
    md, st = mdl.ragged_mixed(700, Z=20, seed=5)
    rng = np.random.default_rng(seed)
    channel, call, ref, rad, info = rc.radiation_case(md, rng, 12)
    assert all(info.values()), info
    NR, S = len(rad["rc_surface"]), int(md["n_surfaces"])
    count = np.bincount(rad["en_receiver"], minlength=NR)
    assert NR > 256 and NR % 64 != 0 and count[rc.EMPTY] == 0 and count[rc.LONG] == rc.N_LONG > 64
    mine = rad["en_receiver"] == rc.SELF
    assert ((rad["en_surface"][mine] == rad["rc_surface"][rc.SELF]) & (rad["en_side"][mine] == rad["rc_side"][rc.SELF])).any()
    assert (rad["en_surface"][mine] < 0).any()
    # both sides of a partition receive, from different rooms
    both = np.intersect1d(rad["rc_surface"][rad["rc_side"] == 0], rad["rc_surface"][rad["rc_side"] == 1])
    assert any(md["front_kind"][q] == mdl.SPACE and md["back_kind"][q] == mdl.SPACE and md["front_zone"][q] != md["back_zone"][q] for q in both)
    # an emitter on a no-mass surface, an emitter that is no receiver, a receiver in another zone than its emitter
    light = rc.nomass_surfaces(md)
    assert len(light) and np.isin(rad["en_surface"][rad["en_receiver"] == rc.NOMASS], light).any()
    # a receiver with a gain array, one without; the receivers have lost their channels, the other sides keep some
    assert call["ir_back"][1] is not None and call["ir_front"][1] is None and (rad["rc_side"] == 1).any() and (rad["rc_side"] == 0).any()
    for name, side in (("ir_front", 0), ("ir_back", 1)):
        assert np.all(call[name][0][rad["rc_surface"][rad["rc_side"] == side]] == -1) and (call[name][0] >= 0).any()
    # the entries are not sorted by receiver: the planner has something to do
    assert (np.diff(rad["en_receiver"]) < 0).any()
    v = rc.rule(md, st, channel[0], rad, ref)
    assert v.shape == (NR,) and v[rc.EMPTY] == 0.0 and np.all(np.isfinite(v)) and np.all(v[np.arange(NR) != rc.EMPTY] > 100.0)
    binding.room_radiation_check(md, rad, weather=np.zeros((12, 1, 3)), n_sub=1, channel=channel,
                                 **{name: chan for name, (chan, _) in call.items()})


def test_room_radiation_check_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "room_radiation_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "room radiation host check: all statuses as the header states them" in out.stdout
