"""Ideal loads in the cluster-resident march, on the host (include/heat_amd.h: heat_batch_set_ideal_resident,
heat_batch_ideal_resident, heat_plan_ideal_resident): the entry points are declared, exported, bound and in the Rust FFI; no
public struct changed its size; the planner's answer — eligible or why not — for the models the GPU tests march, under the
three fusion options, cross-checked against heat_plan_check's count of resident surfaces. heat_plan_ideal_resident also runs
under AddressSanitizer / UBSan as a stand-alone program (tests/ideal_resident_host_main.cpp) in a child process. No GPU needed.

The expected answers are the plan's: which clusters the cost model marches resident by default, and which kernel variant
their workgroups take (batch.hip, enqueue_fused), decide them — a workgroup list without an ideal instantiation of its
kernel makes the whole batch ineligible (plan.hpp, ideal_resident_reason)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
from heat_amd import binding, modeldict as mdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_batch_set_ideal_resident", "heat_batch_ideal_resident", "heat_plan_ideal_resident")
OK, NONE_PLANNED, TEAMS, CAVITY_CLASS, CHUNK_LOOP_CLASS = range(5)


def test_new_symbols_are_declared_exported_bound_and_in_the_rust_ffi():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    bound = {name: (res, args) for name, res, args in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
        assert re.search(r"pub fn %s\(" % name, ffi), name
    assert "heat_plan_ideal_resident" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_set_ideal_resident" not in binding.HOST_ONLY_SYMBOLS and "heat_batch_ideal_resident" not in binding.HOST_ONLY_SYMBOLS
    # the planner query takes the arguments of heat_plan_check_sites plus the reason
    assert bound["heat_plan_ideal_resident"][1][:4] == bound["heat_plan_check_sites"][1][:4]
    assert bound["heat_plan_ideal_resident"][1][4] == C.POINTER(C.c_int32)
    assert hasattr(binding.HeatBatch, "set_ideal_resident") and isinstance(binding.HeatBatch.ideal_resident, property)
    assert (binding.IDEAL_RESIDENT_OK, binding.IDEAL_RESIDENT_NONE_PLANNED, binding.IDEAL_RESIDENT_TEAMS, binding.IDEAL_RESIDENT_CAVITY_CLASS,
            binding.IDEAL_RESIDENT_CHUNK_LOOP_CLASS) == (OK, NONE_PLANNED, TEAMS, CAVITY_CLASS, CHUNK_LOOP_CLASS)
    for i, name in enumerate(("OK", "NONE_PLANNED", "TEAMS", "CAVITY_CLASS", "CHUNK_LOOP_CLASS")):
        assert re.search(r"HEAT_IDEAL_RESIDENT_%s = %d\b" % (name, i), header), name
    assert L.heat_amd_abi_version() == 1 and re.search(r"#define\s+HEAT_AMD_ABI_VERSION\s+1\b", header)
    # a NULL batch: refused / 0, without a device
    assert L.heat_batch_set_ideal_resident(None, 1) == -1 and L.heat_batch_ideal_resident(None) == 0


STRUCTS = dict(heat_batch_desc="Desc", heat_batch_options="Options", heat_series="Series", heat_zone_loads="ZoneLoads",
               heat_series_report="Report", heat_ideal_loads="IdealLoads", heat_air_paths="AirPaths", heat_comfort="Comfort",
               heat_air_handlers="AirHandlers", heat_series_call="SeriesCall")


def test_no_public_struct_changed_its_size(tmp_path):
    """sizeof, as a C compiler sees the header, against the ctypes mirrors (which this change leaves alone) and against the
    sizes the structs had before it."""
    names = sorted(STRUCTS)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(names)), ", ".join("sizeof(%s)" % n for n in names)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(zip(names, (int(x) for x in subprocess.check_output([str(exe)]).split())))
    assert got == {n: C.sizeof(getattr(binding, STRUCTS[n])) for n in names}
    before = dict(heat_batch_desc=320, heat_batch_options=40, heat_series=144, heat_zone_loads=144, heat_series_report=184,
                  heat_ideal_loads=128, heat_air_paths=112, heat_comfort=208, heat_air_handlers=208, heat_series_call=192)
    assert got == before


def teams_model():
    # (two buildings of 40 rooms, as tests/resident_prio_queue_worker.py builds them: larger than a workgroup)
    return mdl.partitioned_buildings(2 * 40 * 12, 32, rooms=40, walls_per_room=12, dt=45.0, seed=64)[0]


# model -> (default options, no_fusion, fuse_always): (eligible, reason), as planned
CASES = {
    "partitioned_buildings": (lambda: mdl.partitioned_buildings(960, 12, seed=8)[0], (True, OK), (False, NONE_PLANNED), (True, OK)),
    # rooms with windows: the cost model streams them by default; resident, their workgroups hold small-surface wavefronts
    # and march the universal variant of their blocking factor, which has its ideal instantiation
    "rooms_with_windows": (lambda: mdl.rooms_with_windows(900, Z=60, seed=6)[0], (False, NONE_PLANNED), (False, NONE_PLANNED), (True, OK)),
    "teams": (teams_model, (False, TEAMS), (False, NONE_PLANNED), (False, TEAMS)),
    # double glazing beside Trombe walls: windows in every workgroup, so the universal variant again
    "glazing_cavity": (lambda: mdl.glazing_cavity(300, Z=4, seed=7)[0], (False, NONE_PLANNED), (False, NONE_PLANNED), (True, OK)),
    # Trombe walls only: workgroups of walls in a class with gas cavities
    "trombe_walls": (lambda: mdl.glazing_cavity(300, Z=4, seed=7, trombe_fraction=1.0)[0], (False, CAVITY_CLASS), (False, NONE_PLANNED),
                     (False, CAVITY_CLASS)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_planner_says_whether_a_batch_is_eligible_and_why_not(case):
    make, *want = CASES[case]
    md = make()
    for opts, (eligible, reason) in zip((dict(), dict(no_fusion=True), dict(fuse_always=True)), want):
        got = binding.plan_ideal_resident(md, **opts)
        summary = binding.plan_check(md, **opts)
        print(case, opts, got, "resident surfaces", summary[5], "workgroups", summary[6])
        assert got == (eligible, reason), (case, opts)
        # "nothing planned resident" exactly when heat_plan_check counts no resident surface
        assert (summary[5] == 0) == (got[1] == NONE_PLANNED), (case, opts, summary)
        assert got[0] == (got[1] == OK)
    if case != "teams":  # as a batch of weather sites (a building per site): the same answers
        opts = dict(fuse_always=True)
        both, site = mdl.concat([md, md])
        assert binding.plan_ideal_resident(both, n_sites=2, site_of_surface=site, **opts) == want[2]


def test_a_model_nothing_of_which_is_planned_resident():
    md = mdl.partitioned_buildings(960, 12, seed=8)[0]
    for opts in (dict(force_general=True), dict(no_palette=True), dict(force_general=True, fuse_always=True)):
        assert binding.plan_check(md, **opts)[5] == 0
        assert binding.plan_ideal_resident(md, **opts) == (False, NONE_PLANNED)


def test_bad_arguments_come_back_as_the_plan_check_returns_them():
    md = mdl.partitioned_buildings(96, 12, seed=8)[0]
    site = np.zeros(int(md["n_surfaces"]), dtype=np.int32)
    site[5] = 2
    with pytest.raises(binding.HeatError) as e:
        binding.plan_ideal_resident(md, n_sites=2, site_of_surface=site)
    with pytest.raises(binding.HeatError) as e2:
        binding.plan_check_sites(md, 2, site)
    assert e.value.code == e2.value.code < 0
    L = binding.load_library()
    reason = C.c_int32(77)
    assert L.heat_plan_ideal_resident(None, None, 1, None, C.byref(reason)) < 0 and reason.value == NONE_PLANNED


def test_the_planner_query_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main, compiled together with the planner: nothing is preloaded."""
    exe = helpers.build_host_main(tmp_path, "ideal_resident_host_main")
    env = dict(os.environ)   # (the sanitizers' runtimes are linked into the program)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ideal resident host check: every answer as the header states it" in out.stdout
