"""Report of a series on the host (include/heat_amd.h, heat_series_report / heat_series_report_check /
heat_batch_march_series_report): the entry points are declared, exported and bound; the ctypes mirror has the header's
layout; every refusal the header lists comes back with its code and names the group or the group entry, before any device
work; good and empty reports are accepted. heat_series_report_check — which also builds the group tables — runs under
AddressSanitizer / UBSan in a child process, like tests/test_zone_loads_host.py. No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from heat_amd import binding, build as hb, modeldict as mdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_series_report_check", "heat_batch_march_series_report")
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
    assert "typedef struct heat_series_report {" in header
    assert "heat_series_report_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_report" not in binding.HOST_ONLY_SYMBOLS
    assert hasattr(binding, "Report") and hasattr(binding, "make_report") and hasattr(binding, "series_report_check")
    assert L.heat_amd_abi_version() == 1


def test_report_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in binding.Report._fields_]
    src = tmp_path / "sz.c"
    fmt = " ".join(["%zu"] * (1 + len(fields)))
    args = ", ".join(["sizeof(heat_series_report)"] + ["offsetof(heat_series_report, %s)" % f for f in fields])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (fmt, args))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = binding.Report
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f in fields]
    # the series and the loads keep their layouts: the report is a struct of its own
    assert [n for n, _ in binding.Series._fields_][-2:] == ["n_probes", "probe_slot"]
    assert [n for n, _ in binding.ZoneLoads._fields_][-1] == "th_mode"


@pytest.fixture(scope="module")
def model():
    md, _ = mdl.ragged_mixed(200, Z=6, seed=5)
    return md


def series(md):
    return dict(weather=np.zeros((4, 2, 3)), n_sub=2, channel=np.zeros((4, N_CHANNELS)), probes=md["zone_slot"][:3])


def thermostats(n=2):
    return dict(thermostats=dict(sensor_zone=np.arange(n), target_zone=np.arange(n), heat_chan=np.full(n, 3),
                                 cool_chan=np.full(n, -1), heat_power=np.full(n, 100.0), cool_power=np.zeros(n), band=np.ones(n)))


def good_groups(md):
    """Empty, single, weighted and unweighted groups of every kind of slot."""
    return [(md["flow_front_slot"][:7], np.linspace(-1.0, 2.0, 7)), np.zeros(0, np.int64), md["zone_slot"][:1],
            (np.concatenate([md["hs_back_slot"][:5], md["first_node_slot"][:5] + 1, md["zone_slot"][:2]]), np.arange(12) - 5.0),
            md["flow_back_slot"]]


def good_report(md, Q=None):
    Q = 3 + len(good_groups(md)) if Q is None else Q
    return dict(groups=good_groups(md), stats=binding.Q_STATS, limits=dict(lo=np.zeros(Q), hi=np.ones(Q)),
                thermostat_stats=binding.TH_STATS, group_trace=True)


def _raw(md, report=None, loads=None, **fields):
    """heat_series_report_check on a hand-made struct (what the Python wrapper would not let through)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(md)
    s, skeep = binding.make_series(**series(md))
    l, lkeep = binding.make_zone_loads(**(thermostats() if loads is None else loads))
    r, rkeep = binding.make_report(n_probes=s.n_probes, n_thermostats=l.n_thermostats, n_steps=s.n_steps,
                                   **(good_report(md) if report is None else report))
    for k, v in fields.items():
        setattr(r, k, v)
    rc = L.heat_series_report_check(C.byref(desc), C.byref(s), C.byref(l), C.byref(r))
    return rc, L.heat_last_error().decode()


def test_good_and_empty_reports_are_accepted(model):
    binding.series_report_check(model, report=good_report(model), loads=thermostats(), **series(model))
    binding.series_report_check(model, report={}, **series(model))
    binding.series_report_check(model, report=dict(stats=("min",)), **series(model))
    binding.series_report_check(model, report=dict(groups=[]), **series(model))
    binding.series_report_check(model, report=dict(groups=[[], []], stats=("sum",)), **series(model))
    # r == NULL is no report; the other arguments are still checked
    L = binding.load_library()
    desc, keep = binding.make_desc(model)
    s, skeep = binding.make_series(**series(model))
    assert L.heat_series_report_check(C.byref(desc), C.byref(s), None, None) == 0
    assert L.heat_series_report_check(C.byref(desc), None, None, None) == E_INVALID_ARG
    assert L.heat_series_report_check(None, C.byref(s), None, None) == E_INVALID_ARG
    # every statistic is nullable on its own (a step needs its extremum, a count its limit: below)
    for field in ("group_weight", "group_trace", "q_step_min", "q_step_max", "q_sum", "q_n_below", "q_deg_below", "q_n_above",
                  "q_deg_above", "th_steps_heating", "th_steps_cooling", "th_switches", "th_sum_heating", "th_sum_cooling"):
        assert _raw(model, **{field: None})[0] == 0, field


def test_negative_count_and_missing_arrays_are_invalid_arguments(model):
    rc, msg = _raw(model, n_groups=-1)
    assert rc == E_INVALID_ARG and "n_groups" in msg, msg
    for field in ("group_offset", "group_slot"):
        rc, msg = _raw(model, **{field: None})
        assert rc == E_INVALID_ARG and field in msg, (field, msg)
    # a NULL array of a count of zero is fine
    assert _raw(model, report=dict(stats=("min",)), n_groups=0, group_offset=None, group_slot=None)[0] == 0


def test_group_offsets_must_start_at_zero_and_never_decrease(model):
    slots = model["flow_front_slot"][:10]
    for off, name in (([1, 4, 10], "group 0"), ([0, 6, 4, 10], "group 1"), ([0, 4, 10, 9], "group 2"), ([0, -1], "group 0")):
        off_a = np.array(off, np.int64)
        rc, msg = _raw(model, report=dict(groups=dict(offset=[0, 10], slot=slots)),
                       n_groups=len(off) - 1, group_offset=off_a.ctypes.data_as(binding._i64p))
        assert rc == E_INVALID_ARG and name in msg, (off, msg)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_weight_that_is_not_finite_is_refused_naming_the_entry(model, bad):
    w = np.ones(10)
    w[6] = bad
    with pytest.raises(binding.HeatError) as e:
        binding.series_report_check(model, report=dict(groups=[(model["flow_front_slot"][:4], w[:4]), (model["zone_slot"][:6], w[4:])]),
                                    **series(model))
    assert e.value.code == E_INVALID_ARG and "group entry 6" in str(e.value), str(e.value)


def test_statistics_without_what_they_need_are_refused(model):
    for field in ("q_lo", "q_hi", "q_min", "q_max"):
        rc, msg = _raw(model, **{field: None})
        assert rc == E_INVALID_ARG, (field, msg)
    for gone, kept in ((("q_lo", "q_n_below"), "q_deg_below"), (("q_lo", "q_deg_below"), "q_n_below"),
                       (("q_hi", "q_n_above"), "q_deg_above"), (("q_hi", "q_deg_above"), "q_n_above")):
        rc, msg = _raw(model, **{f: None for f in gone})
        assert rc == E_INVALID_ARG and kept in msg, (kept, msg)
    # limits alone ask nothing and are fine
    assert _raw(model, q_n_below=None, q_deg_below=None, q_n_above=None, q_deg_above=None)[0] == 0


@pytest.mark.parametrize("stat", binding.TH_STATS)
def test_thermostat_statistics_without_thermostats_are_refused(model, stat):
    report = dict(thermostat_stats=(stat,))
    for loads in ({}, dict(gains=dict(zone=[0], chan=[0]))):
        rc, msg = _raw(model, report=report, loads=loads)
        assert rc == E_INVALID_ARG and "thermostat" in msg, msg
    L = binding.load_library()                                         # ... and with l == NULL
    desc, keep = binding.make_desc(model)
    s, skeep = binding.make_series(**series(model))
    r, rkeep = binding.make_report(n_probes=3, n_thermostats=2, **report)
    assert L.heat_series_report_check(C.byref(desc), C.byref(s), None, C.byref(r)) == E_INVALID_ARG
    assert _raw(model, report=report, loads=thermostats())[0] == 0


def test_a_group_slot_that_is_no_output_of_the_path_is_refused_naming_the_entry(model):
    good = model["flow_front_slot"][:8]
    for bad in (int(model["solar_front_slot"][3]), int(model["ir_back_slot"][0]), -1, int(model["n_state"]) + 5):
        slots = good.copy()
        slots[5] = bad
        with pytest.raises(binding.HeatError) as e:
            binding.series_report_check(model, report=dict(groups=[slots[:2], slots[2:]]), **series(model))
        assert e.value.code == E_SIZE and "group entry 5" in str(e.value), str(e.value)


def test_a_report_of_many_entries_is_checked_like_a_small_one(model):
    """Hundreds of thousands of entries in groups of very different sizes: the same answers, the lowest bad entry named."""
    rng = np.random.default_rng(2)
    pool = np.concatenate([model["flow_front_slot"], model["hs_back_slot"], model["zone_slot"], mdl.node_slots(model)]).astype(np.int64)
    slots = pool[rng.integers(0, len(pool), 300_000)]
    groups = dict(offset=[0, 10, 200_000, 200_000, 300_000], slot=slots, weight=rng.normal(size=len(slots)))
    binding.series_report_check(model, report=dict(groups=groups, stats=("sum",)), **series(model))
    bad = slots.copy()
    bad[[123_456, 250_001, 299_999]] = int(model["solar_back_slot"][0])
    with pytest.raises(binding.HeatError) as e:
        binding.series_report_check(model, report=dict(groups=dict(groups, slot=bad)), **series(model))
    assert e.value.code == E_SIZE and "group entry 123456:" in str(e.value), str(e.value)


def test_bad_loads_and_series_are_refused_as_by_their_own_checks(model):
    with pytest.raises(binding.HeatError) as e:
        binding.series_report_check(model, report=good_report(model, 8), loads=dict(gains=dict(zone=[0, 6], chan=[0, 0])),
                                    **series(model))
    assert e.value.code == E_SIZE and "gain 1" in str(e.value)


def test_march_refuses_before_any_device_work(model):
    """What heat_batch_march_series_report can answer without a batch: the same with or without a device."""
    L = binding.load_library()
    s, _ = binding.make_series(**series(model))
    l, _ = binding.make_zone_loads(**thermostats())
    r, _ = binding.make_report(n_probes=3, n_thermostats=2, n_steps=4, **good_report(model))
    failed = C.c_int32(123)
    assert L.heat_batch_march_series_report(None, C.byref(s), C.byref(l), C.byref(r), None, None, C.byref(failed)) == E_INVALID_ARG
    assert failed.value == -1
    assert L.heat_batch_march_series_report(None, None, None, None, None, None, None) == E_INVALID_ARG


def test_the_wrapper_reads_the_shapes(model):
    r, keep = binding.make_report(n_probes=3, n_thermostats=2, n_steps=4, **good_report(model))
    assert r.n_groups == 5 and r.resume == 0 and r.step_base == 0
    assert list(keep["group_offset"]) == [0, 7, 7, 8, 20, 20 + model["n_surfaces"]]
    assert keep["group_weight"][7] == 1.0 and keep["group_weight"][8] == -5.0     # (a group without weights among weighted ones)
    assert keep["group_trace"].shape == (4, 5)
    assert all(keep["q_" + k].shape == (8,) for k in binding.Q_STATS) and keep["q_step_max"].dtype == np.int64
    assert all(keep["th_" + k].shape == (2,) for k in binding.TH_STATS) and keep["th_sum_cooling"].dtype == np.float64
    r, keep = binding.make_report()
    assert r.n_groups == 0 and not r.group_offset and not r.q_min and not r.th_switches
    first = dict(q_min=np.arange(3.0), q_step_min=np.arange(3))
    r, keep = binding.make_report(n_probes=3, stats=("min", "step_min"), resume=first, step_base=7)
    assert r.resume == 1 and r.step_base == 7 and list(keep["q_min"]) == [0.0, 1.0, 2.0] and keep["q_min"] is not first["q_min"]
    for bad in (lambda: binding.make_report(stats=("mean",)),
                lambda: binding.make_report(n_probes=2, limits=dict(lo=[0.0])),
                lambda: binding.make_report(n_probes=2, limits=dict(low=[0.0, 0.0])),
                lambda: binding.make_report(n_probes=3, stats=("min", "max"), resume=first),
                lambda: binding.make_report(groups=[([1, 2], [1.0])]),
                lambda: binding.make_report(group_trace=True),
                lambda: binding.make_report(thermostat_stats=("cycles",))):
        with pytest.raises(ValueError):
            bad()


def test_series_report_check_under_address_and_ub_sanitizers():
    asan = _asan_runtime()
    if asan is None:
        pytest.skip("gcc has no libasan here")
    lib = hb.build_plan_host()
    env = dict(os.environ)
    env["LD_PRELOAD"] = asan
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "series_report_host_worker.py"), lib], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-6000:])
    assert "series report host check" in out.stdout
