"""Series march on the host (include/heat_amd.h, heat_series / heat_series_check / heat_batch_march_series): the entry
points are declared, exported and bound; every refusal the header lists comes back with its code and names the surface or
the probe, before any device work; the probes resolve against the descriptor's slots; the ctypes mirror has the header's
layout. heat_series_check also runs under AddressSanitizer / UBSan in a child process, like tests/test_sites_host.py.
No GPU needed.

Reference: a series is ThermalModel::march (src/model.rs:359-427) repeated with the inputs set between the calls as the
validation harness sets them (tests/validate_wall_heat_transfer.rs:675-705)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from heat_amd import binding, build as hb, modeldict as mdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_series_check", "heat_batch_march_series")
E_INVALID_ARG, E_SIZE = -1, -4


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
    assert "typedef struct heat_series {" in header
    assert "heat_series_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series" not in binding.HOST_ONLY_SYMBOLS
    assert hasattr(binding.HeatBatch, "march_series") and hasattr(binding, "series_check")


def test_series_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(heat_series), offsetof(heat_series, n_zone_term_steps), '
        'offsetof(heat_series, channel), offsetof(heat_series, ir_own_face), offsetof(heat_series, probe_slot));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = binding.Series
    assert got == [C.sizeof(S), S.n_zone_term_steps.offset, S.channel.offset, S.ir_own_face.offset, S.probe_slot.offset]


@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def _raw(md, n_sites=1, **fields):
    """heat_series_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(np.zeros((4, 2, 3)), 2, probes=md["zone_slot"][:1])
    for k, v in fields.items():
        setattr(s, k, v)
    rc = L.heat_series_check(C.byref(desc), n_sites, C.byref(s))
    return rc, L.heat_last_error().decode()


def test_a_plain_series_is_accepted(model):
    S, Z = model["n_surfaces"], model["n_zones"]
    binding.series_check(model, weather=np.zeros((4, 2, 3)), n_sub=2)
    binding.series_check(model, weather=np.zeros((4, 2, 3)), n_sub=2, channel=np.zeros((4, 3)),
                         solar_front=np.full(S, 2, np.int32), ir_back=(np.full(S, -1, np.int32), np.ones(S)),
                         zone_a0=np.zeros(Z), zone_b0=np.zeros(Z), probes=model["zone_slot"])
    assert _raw(model)[0] == 0


def test_null_and_negative_counts_are_invalid_arguments(model):
    L = binding.load_library()
    desc, keep = binding.make_desc(model)
    assert L.heat_series_check(C.byref(desc), 1, None) == E_INVALID_ARG
    s, _ = binding.make_series(np.zeros((4, 2, 3)), 2)
    assert L.heat_series_check(None, 1, C.byref(s)) == E_INVALID_ARG
    for field in ("n_steps", "n_sub", "n_channels", "n_probes", "n_zone_term_steps"):
        rc, msg = _raw(model, **{field: -1})
        assert rc == E_INVALID_ARG, (field, msg)
    assert _raw(model, weather=None)[0] == E_INVALID_ARG                     # n_steps * n_sub records wanted
    assert _raw(model, n_channels=3)[0] == E_INVALID_ARG                     # a table of 4 x 3 wanted, NULL given
    assert _raw(model, n_probes=2, probe_slot=None)[0] == E_INVALID_ARG
    assert _raw(model, n_sites=0)[0] == E_INVALID_ARG


@pytest.mark.parametrize("rows", [2, 3, 5])
def test_zone_term_rows_other_than_0_1_n_steps_are_refused(model, rows):
    Z = model["n_zones"]
    code, msg = _code(lambda: binding.series_check(model, weather=np.zeros((4, 2, 3)), n_sub=2, zone_a0=np.zeros((rows, Z))))
    assert code == E_INVALID_ARG and "n_zone_term_steps" in msg
    for ok in (1, 4):
        binding.series_check(model, weather=np.zeros((4, 2, 3)), n_sub=2, zone_a0=np.zeros((ok, Z)), zone_b0=np.zeros((ok, Z)))


@pytest.mark.parametrize("which", ["solar_front", "solar_back", "ir_front", "ir_back"])
@pytest.mark.parametrize("bad", [-2, 3, 1 << 20])
def test_channel_out_of_range_is_refused_naming_the_surface(model, which, bad):
    chan = np.full(model["n_surfaces"], -1, np.int32)
    chan[:50] = 1
    chan[137] = bad
    code, msg = _code(lambda: binding.series_check(model, weather=np.zeros((4, 2, 3)), n_sub=2, channel=np.zeros((4, 3)),
                                                   **{which: chan}))
    assert code == E_SIZE and "surface 137" in msg, msg


def test_own_face_on_an_undriven_side_is_refused_naming_the_surface(model):
    S = model["n_surfaces"]
    kw = dict(weather=np.zeros((4, 2, 3)), n_sub=2, channel=np.zeros((4, 3)))
    front = np.zeros(S, np.int32)
    front[61] = -1
    own = np.ones(S, np.uint8)
    code, msg = _code(lambda: binding.series_check(model, ir_front=front, ir_own_face=own, **kw))
    assert code == E_SIZE and "surface 61" in msg, msg
    own[61] = 0
    binding.series_check(model, ir_front=front, ir_own_face=own, **kw)
    own[88] = 2  # the back side's bit, and no back channels at all
    code, msg = _code(lambda: binding.series_check(model, ir_front=front, ir_own_face=own, **kw))
    assert code == E_SIZE and "surface 88" in msg, msg


def test_weather_record_limit_applies_per_step(model):
    # 2^24 records per step on a batch of several sites; the series as a whole may hold more
    rc, msg = _raw(model, n_sites=4096, n_sub=4097)
    assert rc == E_INVALID_ARG and "per step" in msg
    assert _raw(model, n_sites=4096, n_sub=4096, n_steps=100)[0] == 0  # (the check reads no record)


def _owned(md):
    return dict(nodes=mdl.node_slots(md), hs_front=md["hs_front_slot"], hs_back=md["hs_back_slot"],
                flow_front=md["flow_front_slot"], flow_back=md["flow_back_slot"], zones=md["zone_slot"])


@pytest.mark.parametrize("gen", ["ragged_mixed", "rooms_with_windows"])
def test_every_owned_slot_is_a_probe_and_nothing_else_is(gen):
    md, _ = getattr(mdl, gen)(300, Z=12, seed=9)
    kw = dict(weather=np.zeros((2, 1, 3)), n_sub=1)
    owned = _owned(md)
    for name, slots in owned.items():
        binding.series_check(md, probes=slots, **kw)
    binding.series_check(md, probes=np.concatenate(list(owned.values()))[::-1], **kw)
    every = np.concatenate(list(owned.values()))
    for key in ("solar_front_slot", "solar_back_slot", "ir_front_slot", "ir_back_slot"):
        for s_ in (0, 151, 299):
            code, msg = _code(lambda: binding.series_check(md, probes=[every[0], every[5], md[key][s_]], **kw))
            assert code == E_SIZE and "probe 2" in msg, (key, s_, msg)
    for bad in (-1, md["n_state"], md["n_state"] + 1000, 1 << 40):
        code, msg = _code(lambda: binding.series_check(md, probes=[bad], **kw))
        assert code == E_SIZE and "probe 0" in msg, msg


def test_the_empty_series_are_legal(model):
    S = model["n_surfaces"]
    binding.series_check(model, weather=np.zeros((0, 3)), n_sub=2)                                     # n_steps = 0
    binding.series_check(model, weather=None, n_sub=0, n_steps=5, channel=np.zeros((5, 2)),
                         solar_front=np.zeros(S, np.int32), probes=model["zone_slot"])                 # n_sub = 0
    binding.series_check(model, weather=np.zeros((3, 2, 3)), n_sub=2, probes=[])                       # n_probes = 0
    binding.series_check(model, weather=np.zeros((3, 2, 3)), n_sub=2, solar_front=np.full(S, -1, np.int32))  # n_channels = 0
    code, _ = _code(lambda: binding.series_check(model, weather=np.zeros((3, 2, 3)), n_sub=2, solar_front=np.zeros(S, np.int32)))
    assert code == E_SIZE  # channel 0 of a table without channels


def test_march_series_refuses_before_any_device_work():
    """What heat_batch_march_series can answer without a batch: the same with or without a device."""
    L = binding.load_library()
    s, _ = binding.make_series(np.zeros((4, 2, 3)), 2)
    failed = C.c_int32(123)
    assert L.heat_batch_march_series(None, C.byref(s), None, C.byref(failed)) == E_INVALID_ARG
    assert failed.value == -1
    assert L.heat_batch_march_series(None, None, None, None) == E_INVALID_ARG


def test_the_wrapper_reads_the_shapes():
    s, keep = binding.make_series(np.zeros((7, 3, 3)), 3, channel=np.zeros((7, 4)), zone_a0=np.zeros(5), probes=[1, 2])
    assert (s.n_steps, s.n_sub, s.n_channels, s.n_zone_term_steps, s.n_probes) == (7, 3, 4, 1, 2)
    s, keep = binding.make_series(np.zeros((7, 3, 2, 3)), 3, n_sites=2, zone_a0=np.zeros((7, 5)), zone_b0=np.zeros((7, 5)))
    assert (s.n_steps, s.n_zone_term_steps) == (7, 7)
    for bad in (lambda: binding.make_series(np.zeros((7, 3)), 2),                      # no whole number of steps
                lambda: binding.make_series(np.zeros((6, 3)), 2, channel=np.zeros((4, 1))),
                lambda: binding.make_series(np.zeros((6, 3)), 2, n_sites=2),
                lambda: binding.make_series(np.zeros((6, 3)), 2, zone_a0=np.zeros((1, 5)), zone_b0=np.zeros((3, 5))),
                lambda: binding.make_series(np.zeros((6, 3)), 2, solar_front=(np.zeros(4, np.int32), np.zeros(5)))):
        with pytest.raises(ValueError):
            bad()


def test_series_check_under_address_and_ub_sanitizers():
    asan = _asan_runtime()
    if asan is None:
        pytest.skip("gcc has no libasan here")
    lib = hb.build_plan_host()
    env = dict(os.environ)
    env["LD_PRELOAD"] = asan
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "series_host_worker.py"), lib], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-6000:])
    assert "series host check" in out.stdout
