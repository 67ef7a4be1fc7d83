"""Zone loads of a series on the host (include/heat_amd.h, heat_zone_loads / heat_zone_loads_check /
heat_batch_march_series_loads): the entry points are declared, exported and bound; the ctypes mirror has the header's
layout; every refusal the header lists comes back with its code and names the gain, flow or thermostat, before any device
work; empty loads are accepted. heat_zone_loads_check also runs under AddressSanitizer / UBSan in a child process, like
tests/test_series_host.py. No GPU needed.

Reference: the terms are those of calculate_zones_abc (src/model.rs:500-544); the thermostat is this project's own."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from heat_amd import binding, build as hb, modeldict as mdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_zone_loads_check", "heat_batch_march_series_loads")
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
    assert "typedef struct heat_zone_loads {" in header
    assert "heat_zone_loads_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_loads" not in binding.HOST_ONLY_SYMBOLS
    assert hasattr(binding, "ZoneLoads") and hasattr(binding, "make_zone_loads") and hasattr(binding, "zone_loads_check")
    assert L.heat_amd_abi_version() == 1


FIELDS = ("n_gains", "gain_factor", "n_flows", "flow_temp_chan", "flow_volume_gain", "n_thermostats", "th_cool_chan",
          "th_heat_power", "th_band", "th_mode")


def test_zone_loads_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    fmt = " ".join(["%zu"] * (1 + len(FIELDS)))
    args = ", ".join(["sizeof(heat_zone_loads)"] + ["offsetof(heat_zone_loads, %s)" % f for f in FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (fmt, args))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    Z = binding.ZoneLoads
    assert got == [C.sizeof(Z)] + [getattr(Z, f).offset for f in FIELDS]
    # heat_series keeps its layout (tests/test_series_host.py checks the offsets): the loads are a struct of their own
    assert [n for n, _ in binding.Series._fields_][-2:] == ["n_probes", "probe_slot"]


@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


SERIES = dict(weather=np.zeros((4, 2, 3)), n_sub=2, channel=np.zeros((4, N_CHANNELS)))


def good_loads(Z, n=5):
    return dict(
        gains=dict(zone=np.arange(n) % Z, chan=np.arange(n) % N_CHANNELS, factor=np.linspace(0.5, 1.5, n)),
        flows=dict(zone=(np.arange(n) + 1) % Z, volume_chan=np.full(n, 1), temp_chan=np.full(n, 2), volume_gain=np.ones(n)),
        thermostats=dict(sensor_zone=np.arange(n) % Z, target_zone=(np.arange(n) + 2) % Z, heat_chan=np.full(n, 3),
                         cool_chan=np.full(n, -1), heat_power=np.full(n, 100.0), cool_power=np.zeros(n), band=np.ones(n),
                         mode=np.arange(n) % 3))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def _with(loads, group, key, i, value):
    out = {g: dict(v) for g, v in loads.items()}
    a = np.array(out[group][key])
    a[i] = value
    out[group][key] = a
    return out


def _raw(md, loads, **fields):
    """heat_zone_loads_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**SERIES)
    l, lkeep = binding.make_zone_loads(**loads)
    for k, v in fields.items():
        setattr(l, k, v)
    rc = L.heat_zone_loads_check(C.byref(desc), C.byref(s), C.byref(l))
    return rc, L.heat_last_error().decode()


def test_good_and_empty_loads_are_accepted(model):
    Z = model["n_zones"]
    binding.zone_loads_check(model, loads=good_loads(Z), **SERIES)
    binding.zone_loads_check(model, loads={}, **SERIES)
    binding.zone_loads_check(model, loads=dict(gains=dict(zone=[0], chan=[0])), **SERIES)             # factor NULL = 1
    binding.zone_loads_check(model, loads=dict(flows=(np.zeros(2), np.zeros(2), np.ones(2))), **SERIES)
    assert _raw(model, good_loads(Z), th_mode=None)[0] == 0                                           # modes nullable
    # l == NULL is no loads
    L = binding.load_library()
    desc, keep = binding.make_desc(model)
    s, skeep = binding.make_series(**SERIES)
    assert L.heat_zone_loads_check(C.byref(desc), C.byref(s), None) == 0
    assert L.heat_zone_loads_check(C.byref(desc), None, None) == E_INVALID_ARG
    assert L.heat_zone_loads_check(None, C.byref(s), None) == E_INVALID_ARG


def test_negative_counts_and_null_arrays_are_invalid_arguments(model):
    loads = good_loads(model["n_zones"])
    for field in ("n_gains", "n_flows", "n_thermostats"):
        rc, msg = _raw(model, loads, **{field: -1})
        assert rc == E_INVALID_ARG, (field, msg)
    needed = ("gain_zone", "gain_chan", "flow_zone", "flow_volume_chan", "flow_temp_chan", "th_sensor_zone", "th_target_zone",
              "th_heat_chan", "th_cool_chan", "th_heat_power", "th_cool_power", "th_band")
    for field in needed:
        rc, msg = _raw(model, loads, **{field: None})
        assert rc == E_INVALID_ARG, (field, msg)
    for field in ("gain_factor", "flow_volume_gain", "th_mode"):
        assert _raw(model, loads, **{field: None})[0] == 0, field
    # a NULL array of a count of zero is fine
    assert _raw(model, loads, n_gains=0, gain_zone=None, gain_chan=None)[0] == 0


@pytest.mark.parametrize("group,key,name", [("gains", "zone", "gain"), ("flows", "zone", "flow"),
                                            ("thermostats", "sensor_zone", "thermostat"),
                                            ("thermostats", "target_zone", "thermostat")])
@pytest.mark.parametrize("bad", [-1, 6, 1 << 20])
def test_zone_out_of_range_is_refused_naming_the_term(model, group, key, name, bad):
    assert model["n_zones"] == 6
    code, msg = _code(lambda: binding.zone_loads_check(model, loads=_with(good_loads(6), group, key, 3, bad), **SERIES))
    assert code == E_SIZE and "%s 3" % name in msg, msg


@pytest.mark.parametrize("group,key,name", [("gains", "chan", "gain"), ("flows", "volume_chan", "flow"),
                                            ("flows", "temp_chan", "flow"), ("thermostats", "heat_chan", "thermostat"),
                                            ("thermostats", "cool_chan", "thermostat")])
@pytest.mark.parametrize("bad", [-2, N_CHANNELS, 1 << 20])
def test_channel_out_of_range_is_refused_naming_the_term(model, group, key, name, bad):
    code, msg = _code(lambda: binding.zone_loads_check(model, loads=_with(good_loads(6), group, key, 2, bad), **SERIES))
    assert code == E_SIZE and "%s 2" % name in msg, msg


def test_only_a_setpoint_channel_may_be_minus_one(model):
    for group, key, name in (("gains", "chan", "gain"), ("flows", "volume_chan", "flow"), ("flows", "temp_chan", "flow")):
        code, msg = _code(lambda: binding.zone_loads_check(model, loads=_with(good_loads(6), group, key, 4, -1), **SERIES))
        assert code == E_SIZE and "%s 4" % name in msg, msg
    # heating only (good_loads) and cooling only are fine, neither is not
    cooling = _with(_with(good_loads(6), "thermostats", "heat_chan", 1, -1), "thermostats", "cool_chan", 1, 4)
    binding.zone_loads_check(model, loads=cooling, **SERIES)
    code, msg = _code(lambda: binding.zone_loads_check(model, loads=_with(good_loads(6), "thermostats", "heat_chan", 1, -1), **SERIES))
    assert code == E_SIZE and "thermostat 1" in msg, msg


@pytest.mark.parametrize("key", ["heat_power", "cool_power", "band"])
@pytest.mark.parametrize("bad", [-1.0, -1e-300, np.nan, np.inf, -np.inf])
def test_power_or_band_negative_or_not_finite_is_refused(model, key, bad):
    code, msg = _code(lambda: binding.zone_loads_check(model, loads=_with(good_loads(6), "thermostats", key, 3, bad), **SERIES))
    assert code == E_INVALID_ARG and "thermostat 3" in msg, msg
    binding.zone_loads_check(model, loads=_with(good_loads(6), "thermostats", key, 3, 0.0), **SERIES)


@pytest.mark.parametrize("bad", [3, 255])
def test_mode_byte_above_two_is_refused(model, bad):
    code, msg = _code(lambda: binding.zone_loads_check(model, loads=_with(good_loads(6), "thermostats", "mode", 4, bad), **SERIES))
    assert code == E_INVALID_ARG and "thermostat 4" in msg, msg


def test_march_refuses_before_any_device_work():
    """What heat_batch_march_series_loads can answer without a batch: the same with or without a device."""
    L = binding.load_library()
    s, _ = binding.make_series(**SERIES)
    l, _ = binding.make_zone_loads(**good_loads(6))
    failed = C.c_int32(123)
    assert L.heat_batch_march_series_loads(None, C.byref(s), C.byref(l), None, None, C.byref(failed)) == E_INVALID_ARG
    assert failed.value == -1
    assert L.heat_batch_march_series_loads(None, None, None, None, None, None) == E_INVALID_ARG


def test_the_wrapper_reads_the_shapes():
    l, keep = binding.make_zone_loads(**good_loads(6, n=7))
    assert (l.n_gains, l.n_flows, l.n_thermostats) == (7, 7, 7)
    assert keep["th_mode"].dtype == np.uint8 and list(keep["th_mode"]) == [0, 1, 2, 0, 1, 2, 0]
    l, keep = binding.make_zone_loads()
    assert (l.n_gains, l.n_flows, l.n_thermostats) == (0, 0, 0) and not l.gain_zone and not l.th_mode
    l, keep = binding.make_zone_loads(thermostats=dict(sensor_zone=[0, 1], target_zone=[1, 0], heat_chan=[0, 0], cool_chan=[-1, 1],
                                                       heat_power=[1.0, 2.0], cool_power=[0.0, 3.0], band=[0.5, 0.5]))
    assert l.n_thermostats == 2 and list(keep["th_mode"]) == [0, 0]                  # all start off, and come back
    for bad in (lambda: binding.make_zone_loads(gains=dict(zone=[0, 1], chan=[0])),
                lambda: binding.make_zone_loads(gains=dict(zone=[0, 1])),
                lambda: binding.make_zone_loads(flows=dict(zone=[0], volume_chan=[0], temp_chan=[0], gain=[1.0])),
                lambda: binding.make_zone_loads(thermostats=dict(sensor_zone=[0], target_zone=[0], heat_chan=[0]))):
        with pytest.raises(ValueError):
            bad()


def test_zone_loads_check_under_address_and_ub_sanitizers():
    asan = _asan_runtime()
    if asan is None:
        pytest.skip("gcc has no libasan here")
    lib = hb.build_plan_host()
    env = dict(os.environ)
    env["LD_PRELOAD"] = asan
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "zone_loads_host_worker.py"), lib], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-6000:])
    assert "zone loads host check" in out.stdout
