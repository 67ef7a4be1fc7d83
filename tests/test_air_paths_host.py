"""Air paths of a series on the host (include/heat_amd.h, heat_air_paths / heat_air_paths_check / heat_batch_march_series_air;
heat_amd/air_paths.py): the entry points are declared, exported and bound; the ctypes mirror has the header's layout; the rule
in numpy (air_paths.apply — the reference of tests/test_air_paths_gpu.py) gives the hand-worked two-zone cases at, just below
and just above both thresholds of the hysteresis; every refusal the header lists comes back with its code and names the path,
before any device work; the generator's cases are accepted and — run through the CPU oracle alone — exercise the
controllers. heat_air_paths_check — with the table builder and its verification — also runs under AddressSanitizer / UBSan
as a stand-alone program (tests/air_paths_host_main.cpp) in a child process. No GPU needed.

Reference: the rule is this project's own (the reference leaves the mixing of air between zones unimplemented,
model.rs:546,592-593); the air properties are the reference's (gas.rs:49,165-179)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from heat_amd import air_paths, binding, modeldict as mdl
import air_paths_cases as apc
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_air_paths_check", "heat_batch_march_series_air")
E_INVALID_ARG, E_SIZE = -1, -4
N_STEPS = 4
FIELDS = ("n_paths", "target", "source", "temp_chan", "volume_chan", "volume_gain", "open_chan", "sense", "band", "min_delta",
          "state", "sum_q", "steps_open", "switches")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_air_paths {" in header
    assert "heat_air_paths_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_air" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("AirPaths", "make_air_paths", "air_paths_check"))
    assert all(hasattr(air_paths, n) for n in ("apply", "doorway"))
    assert L.heat_amd_abi_version() == 1
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW)


def test_air_paths_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = (["sizeof(heat_air_paths)", "sizeof(heat_solar_gains)", "sizeof(heat_series)", "sizeof(heat_zone_loads)",
             "sizeof(heat_series_report)", "sizeof(heat_ideal_loads)"] + ["offsetof(heat_air_paths, %s)" % f for f in FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    # (the structs beside it keep their sizes: the air paths are a struct of their own)
    assert got == ([C.sizeof(binding.AirPaths), C.sizeof(binding.SolarGains), C.sizeof(binding.Series), C.sizeof(binding.ZoneLoads),
                    C.sizeof(binding.Report), C.sizeof(binding.IdealLoads)] + [getattr(binding.AirPaths, f).offset for f in FIELDS])
    assert [f for f, _ in binding.AirPaths._fields_] == list(FIELDS)
    assert got[0] == 8 * len(FIELDS)


# ---- the rule in numpy: hand-worked two-zone cases ----
VOLUME, SET = 0.03, 22.0


def air_mass_flow(ts, v=VOLUME):
    tk = ts + 273.15
    rho = 101325. * 28.97 / (8314.46261815324 * tk)
    cp = 1002.7370 + 1.2324e-2 * tk
    return (rho * v) * cp


def vent(sense=1, band=1.0, min_delta=0.5, source=1):
    """One controlled path into zone 0: channel 0 its volume, 1 the setpoint, 2 the supply temperature."""
    return dict(target=np.array([0]), source=np.array([source]), temp_chan=np.array([2 if source < 0 else -1]),
                volume_chan=np.array([0]), open_chan=np.array([1]), sense=np.array([sense]), band=np.array([band]),
                min_delta=np.array([min_delta]))


def step(air, tt, ts, state, setpoint=SET):
    st = np.array([state], np.uint8)
    row = np.array([VOLUME, setpoint, ts])
    a0, b0, q = air_paths.apply(np.array([tt, ts]), row, np.array([7.0, 3.0]), np.array([2.0, 1.0]), air, st)
    return int(st[0]), a0, b0, float(q[0])


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def test_an_open_path_adds_m_ts_and_m_and_reports_m_dt():
    air = dict(target=np.array([0, 1]), source=np.array([1, -1]), temp_chan=np.array([-1, 2]), volume_chan=np.array([0, 0]),
               volume_gain=np.array([1.0, 2.0]))
    T, row = np.array([24.0, 20.0]), np.array([VOLUME, SET, 5.0])
    state = np.zeros(2, np.uint8)
    a0, b0, q = air_paths.apply(T, row, np.array([7.0, 3.0]), np.array([2.0, 1.0]), air, state)
    m0, m1 = air_mass_flow(20.0), air_mass_flow(5.0, 2.0 * VOLUME)
    assert 30.0 < m0 < 40.0                                         # 0.03 m3/s of air: about 36 W/K
    assert a0[0] == 7.0 + m0 * 20.0 and b0[0] == 2.0 + m0 and q[0] == m0 * (20.0 - 24.0)
    assert a0[1] == 3.0 + m1 * 5.0 and b0[1] == 1.0 + m1 and q[1] == m1 * (5.0 - 20.0)
    assert not state.any()                                          # uncontrolled: the bytes are left alone
    # no terms given: zeros; the caller's arrays are not written
    a0, b0, q = air_paths.apply(T, row, None, None, air, state)
    assert a0[0] == m0 * 20.0 and b0[1] == m1
    # the caller's order inside a zone: ((a + x1) + x2) + x3, not any other grouping
    three = dict(target=np.array([0, 0, 0]), source=np.array([-1, 1, -1]), temp_chan=np.array([2, -1, 2]),
                 volume_chan=np.array([0, 0, 0]), volume_gain=np.array([1e-3, 1.0, 3e3]))
    a0, b0, q = air_paths.apply(T, row, np.array([0.1, 0.0]), np.array([0.1, 0.0]), three, np.zeros(3, np.uint8))
    m = [air_mass_flow(5.0, 1e-3 * VOLUME), air_mass_flow(20.0), air_mass_flow(5.0, 3e3 * VOLUME)]
    assert b0[0] == ((0.1 + m[0]) + m[1]) + m[2] and a0[0] == ((0.1 + m[0] * 5.0) + m[1] * 20.0) + m[2] * 5.0


def test_the_opening_threshold_at_just_below_and_just_above_the_limit():
    air = vent(sense=1, band=1.0, min_delta=0.5)                    # d = 0.5: opens when Tt - 22 > 0.5 and Tt - Ts > 0.5
    limit = SET + 0.5
    for tt, want in ((limit, 0), (down(limit), 0), (up(limit), 1)):
        state, a0, b0, q = step(air, tt, 18.0, 0)
        assert state == want, tt
        if want:
            m = air_mass_flow(18.0)
            assert a0[0] == 7.0 + m * 18.0 and b0[0] == 2.0 + m and q == m * (18.0 - tt)
        else:
            assert a0[0] == 7.0 and b0[0] == 2.0 and q == 0.0       # closed: nothing added
    # the source must help by more than min_delta
    tt = 24.0
    for ts, want in ((tt - 0.5, 0), (up(tt - 0.5), 0), (down(tt - 0.5), 1)):
        assert step(air, tt, ts, 0)[0] == want, ts
    # the mirror image, a heating vent: opens when 22 - Tt > 0.5 and Ts - Tt > 0.5
    heat = vent(sense=-1, band=1.0, min_delta=0.5)
    limit = SET - 0.5
    for tt, want in ((limit, 0), (up(limit), 0), (down(limit), 1)):
        assert step(heat, tt, 30.0, 0)[0] == want, tt
    assert step(heat, 20.0, 20.5, 0)[0] == 0 and step(heat, 20.0, up(20.5), 0)[0] == 1
    assert step(heat, 20.0, 18.0, 0)[0] == 0                        # a colder source does not help a heating vent
    # a band of 0 and a min_delta of 0: strict inequalities still
    sharp = vent(sense=1, band=0.0, min_delta=0.0)
    assert step(sharp, SET, 18.0, 0)[0] == 0 and step(sharp, up(SET), 18.0, 0)[0] == 1
    assert step(sharp, 24.0, 24.0, 0)[0] == 0 and step(sharp, 24.0, down(24.0), 0)[0] == 1


def test_the_closing_threshold_at_just_below_and_just_above_the_limit():
    air = vent(sense=1, band=1.0, min_delta=0.5)                    # closes when Tt - 22 < -0.5, or when Tt - Ts <= 0
    limit = SET - 0.5
    for tt, want in ((limit, 1), (up(limit), 1), (down(limit), 0)):
        state, a0, b0, q = step(air, tt, 18.0, 1)
        assert state == want, tt
        assert (q != 0.0) == bool(want) and (b0[0] != 2.0) == bool(want)
    # inside the dead band an open path stays open and a closed one closed
    assert step(air, SET + 0.25, 18.0, 1)[0] == 1 and step(air, SET + 0.25, 18.0, 0)[0] == 0
    # open with a source that helps by less than min_delta: it stays open (min_delta is an opening condition only) ...
    assert step(air, SET, SET - 0.25, 1)[0] == 1
    # ... until the source helps no more: g <= 0 closes, at exactly 0 too
    for ts, want in ((SET, 0), (up(SET), 0), (down(SET), 1)):
        assert step(air, SET, ts, 1)[0] == want, ts
    # ... even far beyond the setpoint, where e > d: the opening condition fails on g, the closing one holds
    assert step(air, 30.0, 31.0, 1)[0] == 0
    heat = vent(sense=-1, band=1.0, min_delta=0.5)
    limit = SET + 0.5
    for tt, want in ((limit, 1), (down(limit), 1), (up(limit), 0)):
        assert step(heat, tt, 35.0, 1)[0] == want, tt
    for ts, want in ((SET, 0), (down(SET), 0), (up(SET), 1)):
        assert step(heat, SET, ts, 1)[0] == want, ts


def test_a_nan_keeps_the_state():
    air = vent(sense=1)
    for state in (0, 1):
        got, a0, b0, q = step(air, 30.0, 18.0, state, setpoint=np.nan)   # would open
        assert got == state and (q != 0.0) == bool(state)
        got, _, _, _ = step(air, 10.0, 5.0, state, setpoint=np.nan)      # would close on e < -d; the source still helps
        assert got == state
        assert step(air, 10.0, 18.0, state, setpoint=np.nan)[0] == 0     # g <= 0 is no NaN: it closes whatever the setpoint
    supply = vent(sense=1, source=-1)
    for state in (0, 1):                                                 # a NaN source temperature: g is NaN
        st = np.array([state], np.uint8)
        a0, b0, q = air_paths.apply(np.array([30.0, 0.0]), np.array([VOLUME, SET, np.nan]), None, None, supply, st)
        assert int(st[0]) == state
        assert np.isnan(q[0]) == bool(state) and np.isnan(a0[0]) == bool(state)   # open: the NaN reaches the zone's terms
    # a NaN volume on a closed path poisons nothing
    st = np.zeros(1, np.uint8)
    a0, b0, q = air_paths.apply(np.array([20.0, 18.0]), np.array([np.nan, SET, 0.0]), None, None, air, st)
    assert q[0] == 0.0 and a0[0] == 0.0 and b0[0] == 0.0


def test_sources_are_read_at_the_start_of_the_step_and_a_doorway_is_two_paths():
    chain = dict(target=np.array([2, 1]), source=np.array([1, 0]), volume_chan=np.array([0, 0]))   # B -> C listed before A -> B
    T = np.array([30.0, 20.0, 10.0])
    a0, b0, q = air_paths.apply(T, np.array([VOLUME]), None, None, chain, np.zeros(2, np.uint8))
    assert q[0] == air_mass_flow(20.0) * (20.0 - 10.0) and q[1] == air_mass_flow(30.0) * (30.0 - 20.0)
    d = air_paths.doorway([0, 2], [1, 3], 0, volume_gain=[1.0, 2.0])
    assert d["target"].tolist() == [1, 3, 0, 2] and d["source"].tolist() == [0, 2, 1, 3] and d["volume_gain"].tolist() == [1.0, 2.0, 1.0, 2.0]
    one = air_paths.doorway(4, 5, 3)
    assert one["target"].tolist() == [5, 4] and one["source"].tolist() == [4, 5] and one["volume_chan"].tolist() == [3, 3]
    a0, b0, q = air_paths.apply(np.array([26.0, 20.0]), np.array([VOLUME]), None, None, air_paths.doorway(0, 1, 0), np.zeros(2, np.uint8))
    assert q[0] > 0.0 > q[1]                                        # the cold room gains what the warm room loses, up to rho cp (T)
    assert abs(q[0] + q[1]) < 0.03 * q[0]


# ---- heat_air_paths_check ----
@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


def series(md, **more):
    return dict(dict(weather=np.zeros((N_STEPS, 2, 3)), n_sub=2, channel=np.zeros((N_STEPS, 5))), **more)


def good_air(md):
    """Twelve paths into the six zones: channels 0-1 volumes, 2 a supply temperature, 3-4 setpoints."""
    Z = int(md["n_zones"])
    n = 2 * Z
    target = np.arange(n, dtype=np.int32) % Z
    source = np.where(np.arange(n) % 3 == 0, -1, (target + 1) % Z).astype(np.int32)
    return dict(target=target, source=source, temp_chan=np.where(source < 0, 2, -1).astype(np.int32),
                volume_chan=(np.arange(n) % 2).astype(np.int32), volume_gain=np.linspace(0.5, 1.5, n),
                open_chan=np.where(np.arange(n) % 2 == 0, 3 + np.arange(n) % 2, -1).astype(np.int32),
                sense=np.where(np.arange(n) % 4 < 2, 1, -1).astype(np.int8), band=np.full(n, 0.5), min_delta=np.full(n, 0.2))


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


def _raw(md, air, series_args=None, **fields):
    """heat_air_paths_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**(series_args or series(md)))
    a, akeep = binding.make_air_paths(**air)
    for name, v in fields.items():
        setattr(a, name, v)
    rc = L.heat_air_paths_check(C.byref(desc), 1, C.byref(s), C.byref(a))
    return rc, L.heat_last_error().decode()


def changed(air, key, i, value):
    a = np.array(air[key])
    a[i] = value
    return dict(air, **{key: a})


def test_good_empty_and_absent_paths_are_accepted(model):
    g = good_air(model)
    binding.air_paths_check(model, g, **series(model))
    binding.air_paths_check(model, g, n_sites=3, **series(model, weather=np.zeros((N_STEPS, 2, 3, 3))))
    binding.air_paths_check(model, None, **series(model))                                    # air == NULL
    binding.air_paths_check(model, {}, **series(model))                                      # no path
    for field in ("state", "sum_q", "steps_open", "switches", "volume_gain"):                # nullable
        assert _raw(model, g, **{field: None})[0] == 0, field
    plain = {k: v for k, v in g.items() if k in ("target", "volume_chan", "volume_gain")}
    plain["source"] = (g["target"] + 1) % int(model["n_zones"])
    binding.air_paths_check(model, plain, **series(model))                                   # uncontrolled zone-to-zone: four arrays
    binding.air_paths_check(model, dict(g, state=np.arange(12) % 2, sum_q=np.arange(12.0), switches=np.arange(12)), **series(model))
    # sense, band and min_delta are read only where the path is controlled
    binding.air_paths_check(model, changed(changed(changed(g, "sense", 1, 0), "band", 1, -1.0), "min_delta", 1, np.nan), **series(model))
    # the series' own refusals come first
    code, msg = _code(lambda: binding.air_paths_check(model, g, **series(model, probes=[10 ** 9])))
    assert code == E_SIZE and "probe 0" in msg, msg


def test_negative_counts_and_null_arrays_are_invalid_arguments(model):
    g = good_air(model)
    rc, msg = _raw(model, g, n_paths=-1)
    assert rc == E_INVALID_ARG and "air path" in msg and "n_paths -1" in msg, msg
    for field in ("target", "source", "volume_chan"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "air path 0" in msg and field in msg, (field, msg)
    for field in ("sense", "band", "min_delta"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "air path 0:" in msg and field in msg, (field, msg)


def test_a_path_from_a_zone_into_itself_is_refused(model):
    g = good_air(model)
    code, msg = _code(lambda: binding.air_paths_check(model, changed(g, "source", 7, g["target"][7]), **series(model)))
    assert code == E_INVALID_ARG and "air path 7:" in msg and "same zone" in msg, msg


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, -0.5])
def test_bands_deltas_and_gains_that_are_negative_or_not_finite_are_refused(model, bad):
    g = good_air(model)
    for key in ("band", "min_delta"):
        code, msg = _code(lambda: binding.air_paths_check(model, changed(g, key, 4, bad), **series(model)))      # path 4 is controlled
        assert code == E_INVALID_ARG and "air path 4:" in msg and key in msg, msg
    if not np.isfinite(bad):
        code, msg = _code(lambda: binding.air_paths_check(model, changed(g, "volume_gain", 5, bad), **series(model)))
        assert code == E_INVALID_ARG and "air path 5:" in msg and "volume_gain" in msg, msg
    else:
        binding.air_paths_check(model, changed(g, "volume_gain", 5, bad), **series(model))   # a negative gain is the caller's business


def test_a_sense_other_than_plus_or_minus_one_and_a_state_above_one_are_refused(model):
    g = good_air(model)
    for bad in (0, 2, -2, 127, -128):
        code, msg = _code(lambda: binding.air_paths_check(model, changed(g, "sense", 6, bad), **series(model)))
        assert code == E_INVALID_ARG and "air path 6:" in msg and "sense" in msg, msg
    for bad in (2, 255):
        state = np.zeros(12, np.uint8)
        state[9] = bad
        code, msg = _code(lambda: binding.air_paths_check(model, dict(g, state=state), **series(model)))
        assert code == E_INVALID_ARG and "air path 9:" in msg and "state" in msg, msg


def test_zones_and_channels_out_of_range_are_size_errors(model):
    Z = int(model["n_zones"])
    g = good_air(model)
    for bad in (-1, Z, Z + 12345, -2 ** 31):
        code, msg = _code(lambda: binding.air_paths_check(model, changed(g, "target", 3, bad), **series(model)))
        assert code == E_SIZE and "air path 3:" in msg and "target" in msg, msg
    for bad in (-2, Z, 2 ** 31 - 1):
        code, msg = _code(lambda: binding.air_paths_check(model, changed(g, "source", 4, bad), **series(model)))
        assert code == E_SIZE and "air path 4:" in msg and "source" in msg, msg
    for bad in (-1, 5, 2 ** 31 - 1):
        code, msg = _code(lambda: binding.air_paths_check(model, changed(g, "volume_chan", 8, bad), **series(model)))
        assert code == E_SIZE and "air path 8:" in msg and "volume channel" in msg, msg
    for bad in (-2, 5, -2 ** 31):
        code, msg = _code(lambda: binding.air_paths_check(model, changed(g, "open_chan", 8, bad), **series(model)))
        assert code == E_SIZE and "air path 8:" in msg and "open channel" in msg, msg
    # no channels at all: every volume channel is out of range
    code, msg = _code(lambda: binding.air_paths_check(model, g, **series(model, channel=None)))
    assert code == E_SIZE and "air path 0:" in msg, msg


def test_an_input_has_one_source(model):
    g = good_air(model)
    assert g["source"][0] == -1 and g["source"][1] >= 0
    for bad in (-1, -7, 5):                                                                  # supply air without a temperature channel
        code, msg = _code(lambda: binding.air_paths_check(model, changed(g, "temp_chan", 0, bad), **series(model)))
        assert code == E_SIZE and "air path 0:" in msg and "temperature channel" in msg, msg
    rc, msg = _raw(model, g, temp_chan=None)
    assert rc == E_SIZE and "air path 0:" in msg and "temp_chan is NULL" in msg, msg
    for bad in (0, 2, 5, -2):                                                                # a zone source AND a temperature channel
        code, msg = _code(lambda: binding.air_paths_check(model, changed(g, "temp_chan", 1, bad), **series(model)))
        assert code == E_SIZE and "air path 1:" in msg and "one source" in msg, msg


def test_march_without_a_batch_is_an_invalid_argument(model):
    """What heat_batch_march_series_air can answer without a batch, and so without a device: a NULL batch is refused and
    failed_step reset. That bad paths are refused BEFORE any device work needs a batch: the GPU test
    test_bad_paths_and_sharded_batches_are_refused_by_the_march finds the device state untouched behind every refusal."""
    L = binding.load_library()
    s, _ = binding.make_series(**series(model))
    a, _ = binding.make_air_paths(**good_air(model))
    failed = C.c_int32(123)
    assert L.heat_batch_march_series_air(None, C.byref(s), None, None, None, C.byref(a), None, None, None, None, None, None, None,
                                         C.byref(failed)) == E_INVALID_ARG
    assert failed.value == -1
    assert L.heat_batch_march_series_air(*([None] * 14)) == E_INVALID_ARG


def test_the_wrapper_reads_the_shapes(model):
    a, keep = binding.make_air_paths(**good_air(model))
    assert a.n_paths == 12 and keep["sense"].dtype == np.int8 and keep["state"].dtype == np.uint8 and keep["switches"].dtype == np.int64
    assert not keep["state"].any() and not keep["sum_q"].any() and keep["steps_open"].shape == (12,)
    a, keep = binding.make_air_paths()
    assert a.n_paths == 0 and not a.target and not a.state and not a.sum_q
    resume = np.arange(12.0)
    a, keep = binding.make_air_paths(**dict(good_air(model), sum_q=resume))
    assert np.array_equal(keep["sum_q"], resume) and keep["sum_q"] is not resume
    a, keep = binding.make_air_paths(**dict(good_air(model), stats=("switches",)))
    assert not a.sum_q and not a.steps_open and a.switches and "sum_q" not in keep
    for bad in (dict(source=np.zeros(11)), dict(band=np.zeros(3)), dict(state=np.zeros(13)), dict(stats=("sum",)),
                dict(stats=(), sum_q=np.zeros(12))):
        with pytest.raises(ValueError):
            binding.make_air_paths(**dict(good_air(model), **bad))


# ---- the generator's cases: accepted, and — through the CPU oracle alone — they exercise the controllers ----
COVERAGE_CASES = [("rooms_with_windows", 2), ("rooms_with_windows", 5), ("ragged_mixed", 2)]


@pytest.mark.parametrize("model_name,n_sub", COVERAGE_CASES)
def test_the_generators_cases_are_accepted_and_their_vents_move(oracle, model_name, n_sub):
    c = apc.case(model_name, 24, n_sub, 2, apc.SEED)
    md, air, info = c["md"], c["air"], c["info"]
    kw = dict(weather=c["w"], n_sub=n_sub, channel=c["channel"], probes=c["probes"])
    binding.air_paths_check(md, air, **kw)
    binding.zone_loads_check(md, c["loads"], **kw)
    # what the generator promises
    n, Z = len(air["target"]), int(md["n_zones"])
    per_zone = np.bincount(air["target"], minlength=Z)
    assert per_zone[info["hub"]] == apc.HUB_PATHS and len(info["none"]) >= 2 and not per_zone[info["none"]].any()
    assert (air["source"] < 0).any() and (air["source"] >= 0).any()
    ctl = air["open_chan"] >= 0
    assert 0.35 < ctl.mean() < 0.65 and {1, -1} <= set(air["sense"][ctl].tolist())
    ab, bc = info["chain"]
    assert (air["source"][ab], air["target"][ab], air["source"][bc], air["target"][bc]) == (4, 5, 5, 6)
    i, j = info["pair"]
    assert (air["source"][i], air["target"][i]) == (air["target"][j], air["source"][j]) == (8, 9)
    assert np.isnan(c["channel"][info["nan_steps"], air["open_chan"][info["nan"]]]).all() and len(info["nan_steps"]) >= 3
    order = np.argsort(air["target"], kind="stable")
    assert not np.array_equal(order, np.arange(n))                                           # shuffled
    # the oracle loop alone
    m = oracle.OracleModel(md)

    def march(s, wk, za, zb):
        assert m.march(s, wk, za, zb)[0] == 0

    out = apc.loop_with_rules(march, c, c["st"].copy())
    open_share, switching_share, senses = apc.coverage(air, out)
    print("%s n_sub=%d: %d paths, %d controlled; %.0f %% of the controlled step-paths open, %.0f %% of the controlled paths switch, senses %s"
          % (model_name, n_sub, n, int(ctl.sum()), 100 * open_share, 100 * switching_share, sorted(senses)))
    assert 0.25 <= open_share <= 0.75
    assert switching_share >= 0.25
    assert senses == {1, -1}
    assert np.all(np.isfinite(out["trace"])) and np.all(np.isfinite(out["path_q"]))
    # the accumulators are those of the returned rows
    assert np.array_equal(out["steps_open"][ctl], out["states"][:, ctl].sum(axis=0))
    assert np.all(out["steps_open"][~ctl] == 24) and not out["switches"][~ctl].any()


def test_air_paths_check_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "air_paths_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "air paths host check: all statuses as the header states them" in out.stdout
