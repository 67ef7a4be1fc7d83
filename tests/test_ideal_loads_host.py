"""Ideal loads of a series on the host (include/heat_amd.h, heat_ideal_loads / heat_ideal_loads_check /
heat_batch_march_series_ideal): the entry points are declared, exported and bound; the ctypes mirror has the header's layout;
every refusal the header lists comes back with its code and names the ideal load, before any device work; valid loads —
with +inf and NULL capacities — are accepted. heat_ideal_loads_check also runs under AddressSanitizer / UBSan in a child
process, like tests/test_zone_loads_host.py. No GPU needed.

Reference: the controller is this project's own (IdealHeaterCooler is a todo!() in heating_cooling.rs:66-119)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from heat_amd import binding, build as hb, modeldict as mdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_ideal_loads_check", "heat_batch_march_series_ideal")
E_INVALID_ARG, E_SIZE = -1, -4
N_CHANNELS = 6


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
    assert "typedef struct heat_ideal_loads {" in header
    assert "heat_ideal_loads_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_ideal" not in binding.HOST_ONLY_SYMBOLS
    assert hasattr(binding, "IdealLoads") and hasattr(binding, "make_ideal_loads") and hasattr(binding, "ideal_loads_check")
    assert L.heat_amd_abi_version() == 1


FIELDS = ("n_loads", "zone", "cool_chan", "heat_cap", "cool_cap", "resume", "step_base", "sum_heating", "peak_heating",
          "step_peak_heating", "peak_cooling", "step_peak_cooling", "n_sat_heating", "n_sat_cooling")


def test_ideal_loads_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    fmt = " ".join(["%zu"] * (4 + len(FIELDS)))
    args = ", ".join(["sizeof(heat_ideal_loads)", "sizeof(heat_series)", "sizeof(heat_zone_loads)", "sizeof(heat_series_report)"] +
                     ["offsetof(heat_ideal_loads, %s)" % f for f in FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (fmt, args))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    I = binding.IdealLoads
    # (the three structs beside it keep their sizes: the ideal loads are a struct of their own)
    assert got == [C.sizeof(I), C.sizeof(binding.Series), C.sizeof(binding.ZoneLoads), C.sizeof(binding.Report)] + [
        getattr(I, f).offset for f in FIELDS]


@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


SERIES = dict(weather=np.zeros((4, 2, 3)), n_sub=2, channel=np.zeros((4, N_CHANNELS)))


def good_ideal(n=5):
    return dict(zone=np.arange(n)[::-1].copy(), heat_chan=np.where(np.arange(n) % 3 == 1, -1, 2), cool_chan=np.where(np.arange(n) % 3 == 0, -1, 3),
                heat_cap=np.array([0.0, 150.0, np.inf, 1e9, 20.0])[:n], cool_cap=np.full(n, np.inf))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def _with(ideal, key, i, value):
    out = dict(ideal)
    a = np.array(out[key], dtype=np.float64 if key.endswith("cap") else np.int64)
    a[i] = value
    out[key] = a
    return out


def _raw(md, ideal, **fields):
    """heat_ideal_loads_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**SERIES)
    il, ikeep = binding.make_ideal_loads(**ideal)
    for k, v in fields.items():
        setattr(il, k, v)
    rc = L.heat_ideal_loads_check(C.byref(desc), C.byref(s), C.byref(il))
    return rc, L.heat_last_error().decode()


def test_good_and_empty_loads_are_accepted(model):
    binding.ideal_loads_check(model, ideal=good_ideal(), **SERIES)
    binding.ideal_loads_check(model, ideal={}, **SERIES)
    binding.ideal_loads_check(model, ideal=dict(zone=[3], heat_chan=[0]), **SERIES)               # capacities NULL = unlimited
    binding.ideal_loads_check(model, ideal=dict(zone=np.arange(6), cool_chan=np.full(6, 5), stats=()), **SERIES)
    assert _raw(model, good_ideal(), heat_cap=None, cool_cap=None)[0] == 0
    for field in binding.IDEAL_STATS:                                                             # every accumulator nullable
        if not field.startswith("peak_"):                                                         # (a step array needs its peak)
            assert _raw(model, good_ideal(), **{field: None})[0] == 0, field
    assert _raw(model, good_ideal(), peak_heating=None, step_peak_heating=None)[0] == 0
    L = binding.load_library()
    desc, keep = binding.make_desc(model)
    s, skeep = binding.make_series(**SERIES)
    assert L.heat_ideal_loads_check(C.byref(desc), C.byref(s), None) == 0                         # il == NULL is no loads
    assert L.heat_ideal_loads_check(C.byref(desc), None, None) == E_INVALID_ARG
    assert L.heat_ideal_loads_check(None, C.byref(s), None) == E_INVALID_ARG


def test_negative_count_null_arrays_and_orphan_step_arrays_are_invalid_arguments(model):
    rc, msg = _raw(model, good_ideal(), n_loads=-1)
    assert rc == E_INVALID_ARG and "n_loads" in msg, msg
    for field in ("zone", "heat_chan", "cool_chan"):
        rc, msg = _raw(model, good_ideal(), **{field: None})
        assert rc == E_INVALID_ARG, (field, msg)
    assert _raw(model, good_ideal(), n_loads=0, zone=None, heat_chan=None, cool_chan=None)[0] == 0
    for peak in ("peak_heating", "peak_cooling"):
        rc, msg = _raw(model, good_ideal(), **{peak: None})
        assert rc == E_INVALID_ARG and "step_" + peak in msg, msg


@pytest.mark.parametrize("bad", [-1, 6, 1 << 20])
def test_zone_out_of_range_is_refused_naming_the_load(model, bad):
    assert model["n_zones"] == 6
    code, msg = _code(lambda: binding.ideal_loads_check(model, ideal=_with(good_ideal(), "zone", 3, bad), **SERIES))
    assert code == E_SIZE and "ideal load 3" in msg, msg


@pytest.mark.parametrize("key", ["heat_chan", "cool_chan"])
@pytest.mark.parametrize("bad", [-2, N_CHANNELS, 1 << 20])
def test_channel_out_of_range_is_refused_naming_the_load(model, key, bad):
    code, msg = _code(lambda: binding.ideal_loads_check(model, ideal=_with(good_ideal(), key, 2, bad), **SERIES))
    assert code == E_SIZE and "ideal load 2" in msg, msg


def test_a_load_needs_a_setpoint_channel(model):
    ideal = good_ideal()
    assert ideal["heat_chan"][1] == -1 and ideal["cool_chan"][0] == -1                          # heating only, cooling only: fine
    code, msg = _code(lambda: binding.ideal_loads_check(model, ideal=_with(ideal, "cool_chan", 1, -1), **SERIES))
    assert code == E_SIZE and "ideal load 1" in msg, msg


@pytest.mark.parametrize("key", ["heat_cap", "cool_cap"])
@pytest.mark.parametrize("bad", [-1.0, -1e-300, np.nan, -np.inf])
def test_capacity_negative_or_nan_is_refused(model, key, bad):
    code, msg = _code(lambda: binding.ideal_loads_check(model, ideal=_with(good_ideal(), key, 4, bad), **SERIES))
    assert code == E_INVALID_ARG and "ideal load 4" in msg, msg
    for fine in (0.0, np.inf):
        binding.ideal_loads_check(model, ideal=_with(good_ideal(), key, 4, fine), **SERIES)


def test_a_second_load_on_a_zone_is_refused(model):
    ideal = good_ideal()
    code, msg = _code(lambda: binding.ideal_loads_check(model, ideal=_with(ideal, "zone", 3, int(ideal["zone"][1])), **SERIES))
    assert code == E_INVALID_ARG and "ideal load 3" in msg and "ideal load 1" in msg, msg


def test_march_refuses_before_any_device_work():
    """What heat_batch_march_series_ideal can answer without a batch: the same with or without a device."""
    L = binding.load_library()
    s, _ = binding.make_series(**SERIES)
    il, _ = binding.make_ideal_loads(**good_ideal())
    failed = C.c_int32(123)
    assert L.heat_batch_march_series_ideal(None, C.byref(s), None, C.byref(il), None, None, None, None, C.byref(failed)) == E_INVALID_ARG
    assert failed.value == -1
    assert L.heat_batch_march_series_ideal(None, None, None, None, None, None, None, None, None) == E_INVALID_ARG


def test_the_wrapper_reads_the_shapes():
    il, keep = binding.make_ideal_loads(**good_ideal())
    assert il.n_loads == 5 and il.resume == 0 and sorted(k for k in keep if k in binding.IDEAL_STATS) == sorted(binding.IDEAL_STATS)
    assert keep["n_sat_heating"].dtype == np.int64 and keep["peak_cooling"].dtype == np.float64
    il, keep = binding.make_ideal_loads()
    assert il.n_loads == 0 and not il.zone and not il.heat_cap
    il, keep = binding.make_ideal_loads(zone=[1, 2], heat_chan=[0, 0], stats=("sum_heating",), resume=dict(sum_heating=[1.0, 2.0]), step_base=7)
    assert il.resume == 1 and il.step_base == 7 and list(keep["sum_heating"]) == [1.0, 2.0] and not il.peak_heating
    assert list(keep["cool_chan"]) == [-1, -1]
    for bad in (lambda: binding.make_ideal_loads(zone=[0, 1], heat_chan=[0]),
                lambda: binding.make_ideal_loads(zone=[0], heat_chan=[0], stats=("sum",)),
                lambda: binding.make_ideal_loads(zone=[0], heat_chan=[0], stats=("sum_heating",), resume={})):
        with pytest.raises(ValueError):
            bad()


def test_ideal_loads_check_under_address_and_ub_sanitizers():
    asan = _asan_runtime()
    if asan is None:
        pytest.skip("gcc has no libasan here")
    lib = hb.build_plan_host()
    env = dict(os.environ)
    env["LD_PRELOAD"] = asan
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ideal_loads_host_worker.py"), lib], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-6000:])
    assert "ideal loads host check" in out.stdout
