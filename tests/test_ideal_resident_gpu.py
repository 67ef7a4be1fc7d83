"""Ideal loads in the cluster-resident march on the GPU (include/heat_amd.h, heat_ideal_loads, RESIDENT FORM;
heat_batch_set_ideal_resident): the lane that finishes a zone in the resident march applies the rule of the loads.

The expected result is DEFINED by tests/ideal_loads_ref.py, as for the streamed form (tests/test_ideal_loads_gpu.py), and
held at the same tolerances: state and trace at rtol = atol = 1e-9, |dq| <= 1e-9 * n_sub * S, saturation counts equal where
the reference's margin exceeds 1e-7. The resident form is NOT bit-equal to the streamed form (its zone sums are the resident
march's), but everything the rule makes exact is tested exactly: the setpoint itself, cut and resume, repeatability, the
accumulators against the returned rows, and — for zones without a load — the bits of the plain resident march. Without the
opt-in, on a batch that is not eligible and in calls too short to march resident, the series has the bits and the launches
of the default path. Every resident case asserts ideal_resident == 1 and n_fused_launches > 0.

Shapes: the models of tests/test_series_gpu.py (buildings of 8 rooms: a row of 16 lanes per zone; rooms with windows:
workgroups with small-surface wavefronts), clusters of one zone on two wavefronts each (a wavefront per zone), walls of 32
nodes at 4, 8 and 16 nodes per lane, and buildings beside a ragged remainder that is streamed."""
import os
import re
import subprocess
import sys
from contextlib import contextmanager

import numpy as np
import pytest

from heat_amd import HeatBatch, binding, modeldict as mdl
from ideal_loads_ref import accumulate, cpu_series
from ideal_resident_queue_worker import N_STEPS
from test_ideal_loads_gpu import ACC, SAT, ideal_case, reference, run
from test_series_gpu import MODELS, assert_close, owned_slots, series_kwargs
from test_series_report_gpu import assert_same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RES = dict(ideal_resident=True)


def zone_per_wavefront():
    """Twelve clusters of one zone and 60 walls of 32 nodes — two wavefronts at 16 nodes per lane; the planner joins
    neighbours up to four wavefronts: two zones on four wavefronts, a wavefront per zone."""
    sizes = [60] * 12
    md, st = mdl.uniform_massive(sum(sizes), 32, Z=len(sizes), dt=45.0, seed=66)
    md["back_zone"] = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    mdl.set_ir_from_air(md, st, 10.0)
    return md, st


def resident_and_streamed():
    """Buildings (resident) beside a ragged mix of which nearly everything is streamed, zones of both with loads."""
    (m1, s1), (m2, s2) = mdl.partitioned_buildings(960, 12, seed=8), mdl.ragged_mixed(700, Z=20, seed=5)
    md, _ = mdl.concat([m1, m2])
    return md, np.concatenate([s1, s2])


# case -> (model, batch options beside the opt-in, seed offset of ideal_case)
CASES = {
    "partitioned_buildings": ("partitioned_buildings", dict(), 300),                        # rows of 16 lanes per zone
    "rooms_with_windows": ("rooms_with_windows", dict(fuse_always=True), 300),               # workgroups with small surfaces
    "zone_per_wavefront": (zone_per_wavefront, dict(nodes_per_lane=16, fuse_always=True), 300),
    "resident_and_streamed": (resident_and_streamed, dict(fuse_always=True), 300),
    "walls32-4": (lambda: mdl.partitioned_buildings(384, 32, rooms=4, seed=18), dict(nodes_per_lane=4, fuse_always=True), 300),
    "walls32-8": (lambda: mdl.partitioned_buildings(384, 32, rooms=4, seed=18), dict(nodes_per_lane=8, fuse_always=True), 300),
    "walls32-16": (lambda: mdl.partitioned_buildings(384, 32, rooms=4, seed=18), dict(nodes_per_lane=16, fuse_always=True), 300),
}


@contextmanager
def model_named(name, make):
    """ideal_case (tests/test_ideal_loads_gpu.py) looks its model up in tests/test_series_gpu.MODELS: a model of this file is
    there under its own name while the case is built, and not afterwards."""
    if not callable(make):
        yield make
        return
    key = "ideal_resident:" + name
    MODELS[key] = make
    try:
        yield key
    finally:
        del MODELS[key]


def case_of(name, n_steps, n_sub, seed=None, caps="mixed"):
    make, opts, seed0 = CASES[name]
    with model_named(name, make) as key:
        return ideal_case(key, n_steps, n_sub, seed0 + n_sub if seed is None else seed, caps=caps), opts


_REF = {}


def reference_of(oracle, name, n_steps, n_sub):
    """The CPU reference of a case, computed once (the two models of tests/test_ideal_loads_gpu.py share that file's cache)."""
    make, _, seed0 = CASES[name]
    if not callable(make):
        return reference(oracle, make, n_steps, n_sub)
    key = (name, n_steps, n_sub)
    if key not in _REF:
        (md, st, channel, drives, probes, a0, b0, loads, ideal, w), _ = case_of(name, n_steps, n_sub)
        ref = st.copy()
        _REF[key] = (cpu_series(oracle, md, ref, w, n_sub, channel, drives, probes, loads, ideal, a0, b0), ref)
    return _REF[key]


def run_resident(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts, seen=None, **more):
    """run() of tests/test_ideal_loads_gpu.py with the opt-in — plus what every resident case asserts of its batch.
    seen (a dict): receives the batch's n_fused_launches after the series."""
    got = st.copy()
    with HeatBatch(md, **dict(opts, **RES)) as b:
        assert b.ideal_resident == 1, "the batch is not eligible"
        fused_surfaces, n_surfaces = b.n_fused_surfaces, b.n_surfaces
        b.upload_state(got)
        out = b.march_series(w, n_sub, loads=loads, ideal=ideal, **dict(series_kwargs(channel, drives, probes, a0, b0), **more))
        b.download_state(got)
        assert b.n_fused_launches > 0, "the ideal series was streamed"
        if seen is not None:
            seen["n_fused_launches"] = b.n_fused_launches
    assert out["failed_step"] == -1
    return out, got, (fused_surfaces, n_surfaces)


def hold_to_the_reference(what, md, n_sub, ideal, ref, ref_state, out, got):
    """The assertions of test_ideal_series_matches_the_cpu_reference, its preconditions on the reference included."""
    print("%s n_sub=%d: %d loads; reference sub-timesteps heating %d, cooling %d, floating %d; saturated %d + %d; smallest "
          "|need - cap| / S = %.3g" % (what, n_sub, len(ideal["zone"]), ref["n_heat"], ref["n_cool"], ref["n_free"], ref["n_sat_heating"].sum(),
                                       ref["n_sat_cooling"].sum(), ref["margin"]))
    assert ref["n_heat"] > 0 and ref["n_cool"] > 0 and ref["n_free"] > 0
    assert 0 < ref["n_sat_heating"].sum() < ref["n_heat"] and 0 < ref["n_sat_cooling"].sum() < ref["n_cool"]
    assert (ref["applied"] != 0).any()
    assert ref["margin"] > 1e-7
    assert_close(ref["trace"], out["trace"], "%s n_sub=%d trace" % (what, n_sub))
    own = owned_slots(md)
    assert_close(ref_state[own], got[own], "%s n_sub=%d final state" % (what, n_sub))
    assert_close(ref["applied"], out["applied"], "%s n_sub=%d applied" % (what, n_sub))
    assert np.array_equal(ref["modes"], out["modes"])
    dq = np.abs(out["ideal_q"] - ref["ideal_q"]) / ref["scale"]
    print("%s n_sub=%d ideal_q: worst |dq| / S = %.3e (bound %.1e)" % (what, n_sub, dq.max(), 1e-9 * n_sub))
    assert np.all(np.isfinite(out["ideal_q"])) and dq.max() <= 1e-9 * n_sub
    for k in SAT:
        assert np.array_equal(ref[k], out["ideal"][k]), k


# ---- 1. against the CPU reference ----
@pytest.mark.parametrize("n_sub,n_steps", [(2, 24), (20, 8)])
@pytest.mark.parametrize("name", ["partitioned_buildings", "rooms_with_windows", "zone_per_wavefront"])
def test_resident_ideal_series_matches_the_cpu_reference(oracle, name, n_sub, n_steps):
    (md, st, channel, drives, probes, a0, b0, loads, ideal, w), opts = case_of(name, n_steps, n_sub)
    ref, ref_state = reference_of(oracle, name, n_steps, n_sub)
    out, got, (fused, total) = run_resident(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts)
    assert fused == total                                  # every zone is finished by a workgroup
    hold_to_the_reference(name, md, n_sub, ideal, ref, ref_state, out, got)


@pytest.mark.parametrize("nodes_per_lane", [4, 8, 16])
def test_every_blocking_factor_matches_the_cpu_reference(oracle, nodes_per_lane):
    name, n_steps, n_sub = "walls32-%d" % nodes_per_lane, 24, 2
    (md, st, channel, drives, probes, a0, b0, loads, ideal, w), opts = case_of(name, n_steps, n_sub)
    ref, ref_state = reference_of(oracle, "walls32-4", n_steps, n_sub)   # (one model, one reference)
    out, got, (fused, total) = run_resident(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts)
    with HeatBatch(md, **opts) as b:
        counts = b.class_counts()
    assert fused == total and counts[{4: 0, 8: 1, 16: 2}[nodes_per_lane]] == total, counts
    hold_to_the_reference(name, md, n_sub, ideal, ref, ref_state, out, got)


# ---- 2. resident and streamed in one batch ----
@pytest.mark.parametrize("n_sub,n_steps", [(2, 24), (20, 8)])
def test_resident_and_streamed_zones_in_one_batch(oracle, n_sub, n_steps):
    """The zones no workgroup owns get the rule from the streamed zone update restricted to them: a zone update that wrote
    a zone it does not own would overwrite what a workgroup holds in LDS with a temperature from stale sums."""
    name = "resident_and_streamed"
    (md, st, channel, drives, probes, a0, b0, loads, ideal, w), opts = case_of(name, n_steps, n_sub)
    ref, ref_state = reference_of(oracle, name, n_steps, n_sub)
    out, got, (fused, total) = run_resident(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts)
    assert 0 < fused < total
    # loads on zones of both: of the buildings (the first 80 zones) and of the ragged remainder
    n_first = int(mdl.partitioned_buildings(960, 12, seed=8)[0]["n_zones"])
    assert (ideal["zone"] < n_first).any() and (ideal["zone"] >= n_first).any()
    hold_to_the_reference(name, md, n_sub, ideal, ref, ref_state, out, got)


# ---- 3. zones without a load ----
def test_zones_without_a_load_have_the_bits_of_the_plain_resident_march():
    n_steps, n_sub = 12, 3
    (md, st, channel, drives, probes, a0, b0, loads, ideal, w), opts = case_of("partitioned_buildings", n_steps, n_sub, seed=91)
    rooms = 8
    keep = (ideal["zone"] // rooms) % 2 == 0               # loads on the zones of every second building only
    half = {k: (v[keep] if isinstance(v, np.ndarray) and len(v) == len(keep) else v) for k, v in ideal.items()}
    assert 0 < keep.sum() < len(keep)
    free_zone = (np.arange(md["n_zones"]) // rooms) % 2 == 1
    out, got, _ = run_resident(md, st, w, n_sub, channel, drives, md["zone_slot"], a0, b0, loads, half, opts)
    assert (out["ideal_q"] != 0).any()
    plain = st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(plain)
        trace, failed, applied, modes = b.march_series(w, n_sub, loads=loads, **series_kwargs(channel, drives, md["zone_slot"], a0, b0))
        b.download_state(plain)
        assert failed == -1 and b.n_fused_launches > 0
    assert np.array_equal(out["trace"][:, free_zone], trace[:, free_zone])
    assert not np.array_equal(out["trace"][:, ~free_zone], trace[:, ~free_zone])
    # the final state of the other buildings' slots: their zones, and every wall that faces one of them
    S = int(md["n_surfaces"])
    faces = np.zeros(S, dtype=bool)
    for kind, zone in ((md["front_kind"], md["front_zone"]), (md["back_kind"], md["back_zone"])):
        faces |= (np.asarray(kind) == mdl.SPACE) & free_zone[np.clip(zone, 0, md["n_zones"] - 1)]
    n_nodes = np.diff(md["node_offset"])
    slots = [md["zone_slot"][free_zone]]
    for s in np.flatnonzero(faces):
        slots.append(md["first_node_slot"][s] + np.arange(n_nodes[s]))
        slots.append(np.array([md[k][s] for k in ("hs_front_slot", "hs_back_slot", "flow_front_slot", "flow_back_slot")]))
    slots = np.concatenate(slots).astype(np.int64)
    assert len(slots) > S and np.array_equal(got[slots], plain[slots])


# ---- 4. exact properties, resident ----
def test_unlimited_loads_on_one_constant_channel_hold_it_bit_for_bit_resident():
    n_steps, n_sub = 12, 3
    (md, st, channel, drives, probes, a0, b0, loads, ideal, w), opts = case_of("rooms_with_windows", n_steps, n_sub, seed=21, caps="none")
    sp = float(np.median(st[md["zone_slot"]])) + 0.3217
    channel = np.concatenate([channel, np.full((n_steps, 1), sp)], axis=1)
    c = channel.shape[1] - 1
    zone = ideal["zone"]
    ideal = dict(zone=zone, heat_chan=np.full(len(zone), c), cool_chan=np.full(len(zone), c))
    out, got, _ = run_resident(md, st, w, n_sub, channel, drives, md["zone_slot"], a0, b0, loads, ideal, opts)
    assert np.array_equal(out["trace"][:, zone], np.full((n_steps, len(zone)), sp))
    assert (out["ideal_q"] != 0).any() and not out["ideal"]["n_sat_heating"].any() and not out["ideal"]["n_sat_cooling"].any()
    others = np.setdiff1d(np.arange(md["n_zones"]), zone)
    assert (out["trace"][:, others] != sp).all()


@pytest.mark.parametrize("name", ["partitioned_buildings", "resident_and_streamed"])
def test_a_resident_series_cut_and_resumed_gives_the_bits_of_the_whole(name):
    n_steps, n_sub = 14, 3
    (md, st, channel, drives, probes, a0, b0, loads, ideal, w), opts = case_of(name, n_steps, n_sub, seed=33)
    whole, whole_state, _ = run_resident(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts)
    again, again_state, _ = run_resident(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts)
    for k in ("trace", "ideal_q", "applied", "modes"):
        assert np.array_equal(whole[k], again[k]), k                       # two runs, the same bits
    assert_same(whole["ideal"], again["ideal"], ACC + SAT, "repeat")
    assert np.array_equal(whole_state, again_state)
    assert_same(accumulate(whole["ideal_q"]), whole["ideal"], ACC, "accumulators")   # a plain loop over the rows
    assert (whole["ideal"]["n_sat_heating"] > 0).any() and (whole["ideal"]["n_sat_cooling"] > 0).any()
    cut = 5                                                                # (an odd number of calls before the cut: the zig-zag parity differs)
    got = st.copy()
    with HeatBatch(md, **dict(opts, **RES)) as b:
        b.upload_state(got)
        kw = lambda steps: series_kwargs(channel, drives, probes, a0, b0, steps=steps)
        first = b.march_series(w[:cut], n_sub, loads=loads, ideal=ideal, **kw(slice(0, cut)))
        loads2 = dict(loads, thermostats=dict(loads["thermostats"], mode=first["modes"]))
        second = b.march_series(w[cut:], n_sub, loads=loads2, ideal=dict(ideal, resume=first["ideal"], step_base=cut), **kw(slice(cut, None)))
        b.download_state(got)
        assert b.ideal_resident == 1 and b.n_fused_launches > 0
    assert first["failed_step"] == -1 and second["failed_step"] == -1
    for k in ("trace", "ideal_q", "applied"):
        assert np.array_equal(whole[k], np.concatenate([first[k], second[k]])), k
    assert np.array_equal(whole["modes"], second["modes"])
    assert_same(whole["ideal"], second["ideal"], ACC + SAT, "cut at %d" % cut)
    assert np.array_equal(whole_state, got)


def test_capacities_of_zero_give_no_power_resident():
    n_steps, n_sub = 8, 3
    (md, st, channel, drives, probes, a0, b0, loads, ideal, w), opts = case_of("partitioned_buildings", n_steps, n_sub, seed=51, caps="zero")
    out, got, _ = run_resident(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts)
    assert not out["ideal_q"].any() and not out["ideal"]["n_sat_heating"].any() and not out["ideal"]["n_sat_cooling"].any()


# ---- 5. opt-in hygiene ----
def test_the_opt_in_switched_off_is_the_default_path_again():
    n_steps, n_sub = 8, 3
    (md, st, channel, drives, probes, a0, b0, loads, ideal, w), opts = case_of("partitioned_buildings", n_steps, n_sub, seed=81)
    kw = series_kwargs(channel, drives, probes, a0, b0)
    fresh, fresh_state = run(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts)
    got = st.copy()
    with HeatBatch(md, **opts) as b:
        assert b.ideal_resident == 0
        b.set_ideal_resident(True)
        assert b.ideal_resident == 1
        b.set_fusion(False)
        assert b.ideal_resident == 0                                       # (independent settings; both are needed)
        b.set_fusion(True)
        b.upload_state(st.copy())
        first = b.march_series(w, n_sub, loads=loads, ideal=ideal, **kw)
        launches = b.n_fused_launches
        assert first["failed_step"] == -1 and launches > 0
        b.set_ideal_resident(False)
        assert b.ideal_resident == 0
        b.upload_state(got)
        second = b.march_series(w, n_sub, loads=loads, ideal=ideal, **kw)
        b.download_state(got)
        assert b.n_fused_launches == launches                              # no fused launch was added
    assert second["failed_step"] == -1
    for k in ("trace", "ideal_q", "applied", "modes"):
        assert np.array_equal(fresh[k], second[k]), k
    assert_same(fresh["ideal"], second["ideal"], ACC + SAT, "default path")
    assert np.array_equal(fresh_state, got)
    assert not np.array_equal(first["trace"], second["trace"])             # (the resident form differs by the sums' rounding)


def test_a_plain_series_after_a_resident_ideal_one_is_the_plain_series_of_a_fresh_batch():
    n_steps, n_sub = 8, 3
    (md, st, channel, drives, probes, a0, b0, loads, ideal, w), opts = case_of("partitioned_buildings", n_steps, n_sub, seed=81)
    kw = series_kwargs(channel, drives, probes, a0, b0)
    with HeatBatch(md, **opts) as b:
        ref = st.copy()
        b.upload_state(ref)
        trace, failed = b.march_series(w, n_sub, **kw)
        b.download_state(ref)
        fused = b.n_fused_launches
    with HeatBatch(md, **dict(opts, **RES)) as b:
        b.upload_state(st.copy())
        out = b.march_series(w, n_sub, loads=loads, ideal=ideal, **kw)
        ideal_launches = b.n_fused_launches
        assert out["failed_step"] == -1 and ideal_launches > 0
        got = st.copy()
        b.upload_state(got)
        trace2, failed2 = b.march_series(w, n_sub, **kw)
        b.download_state(got)
        assert b.n_fused_launches == ideal_launches + fused
    assert failed == -1 and failed2 == -1
    assert np.array_equal(trace, trace2) and np.array_equal(ref, got)


def test_a_batch_of_teams_keeps_the_default_path():
    n_steps, n_sub = 4, 3
    make = lambda: mdl.partitioned_buildings(2 * 40 * 12, 32, rooms=40, walls_per_room=12, dt=45.0, seed=64)
    opts = dict(nodes_per_lane=16, fuse_always=True)
    with model_named("teams", make) as key:
        md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case(key, n_steps, n_sub, 71)
    assert binding.plan_ideal_resident(md, **opts) == (False, binding.IDEAL_RESIDENT_TEAMS)
    fresh, fresh_state = run(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts)
    got = st.copy()
    with HeatBatch(md, **dict(opts, **RES)) as b:
        assert b.ideal_resident == 0 and b.n_fused_surfaces > 0
        b.upload_state(got)
        out = b.march_series(w, n_sub, loads=loads, ideal=ideal, **series_kwargs(channel, drives, probes, a0, b0))
        b.download_state(got)
        assert b.n_fused_launches == 0
    for k in ("trace", "ideal_q", "applied", "modes"):
        assert np.array_equal(fresh[k], out[k]), k
    assert_same(fresh["ideal"], out["ideal"], ACC + SAT, "teams")
    assert np.array_equal(fresh_state, got)


def test_one_sub_timestep_on_a_large_batch_streams():
    n_steps = 3
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case("partitioned_buildings_large", n_steps, 1, 72)
    assert md["n_surfaces"] > 8192
    kw = series_kwargs(channel, drives, probes, a0, b0)
    fresh, fresh_state = run(md, st, w, 1, channel, drives, probes, a0, b0, loads, ideal)
    got = st.copy()
    with HeatBatch(md, **RES) as b:
        assert b.ideal_resident == 1
        b.upload_state(got)
        out = b.march_series(w, 1, loads=loads, ideal=ideal, **kw)
        b.download_state(got)
        assert b.n_fused_launches == 0                                     # (the call-length rule of the plain march)
    assert np.array_equal(fresh["trace"], out["trace"]) and np.array_equal(fresh["ideal_q"], out["ideal_q"])
    assert np.array_equal(fresh_state, got)


# ---- 6. the work queue ----
WORKER = os.path.join(HERE, "ideal_resident_queue_worker.py")
TIMEOUT = 180.0
FUSED_LINE = re.compile(r"heat_amd: fused launch( on the work queue)? with ideal loads: (\d+) workgroups for (\d+) blocks \(class (\d+), list (\d+), (\d+) sub-timesteps\)")
_runs = {}
_stopped = []  # why no further child is started (a child that died or hung)


def child(tmp, n_sub, **env):
    key = (n_sub, tuple(sorted(env.items())))
    if key in _runs:
        return _runs[key]
    if _stopped:
        pytest.fail("not started: " + _stopped[0])
    out_path = os.path.join(str(tmp), "queue-%d%s.npz" % (n_sub, "".join("-%s" % v for _, v in key[1])))
    full_env = {k: v for k, v in os.environ.items() if k not in ("HEAT_AMD_FUSED_ROOM", "HEAT_AMD_FUSED_RESERVE", "HEAT_AMD_FUSED_PERSIST")}
    full_env.update(env, HEAT_AMD_TRACE="1")
    try:
        r = subprocess.run([sys.executable, WORKER, str(n_sub), out_path], capture_output=True, text=True, timeout=TIMEOUT, env=full_env)
    except subprocess.TimeoutExpired:
        _stopped.append("queue-%d %s ran into its limit of %.0f s" % (n_sub, env, TIMEOUT))
        pytest.fail(_stopped[0])
    if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in r.stdout + r.stderr:
        _stopped.append("queue-%d %s died with %d" % (n_sub, env, r.returncode))
    assert r.returncode == 0 and "IDEAL RESIDENT OK" in r.stdout, "exit %s\n%s\n%s" % (
        r.returncode, r.stdout[-2000:], "\n".join(l for l in r.stderr.splitlines() if "launch" not in l)[-4000:])
    fused = [(bool(m.group(1)),) + tuple(int(x) for x in m.groups()[1:]) for m in FUSED_LINE.finditer(r.stderr)]
    _runs[key] = (fused, dict(np.load(out_path)))
    return _runs[key]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("ideal_resident_queue")


@pytest.mark.parametrize("n_sub", [2, 5])
def test_work_queue_gives_the_bits_of_one_workgroup_per_block(tmp, n_sub):
    """Ten clusters on three persistent workgroups: the per-zone arrays of the loads are refilled for every block a
    workgroup takes, and a zone's q-sum and counts are handed back by the workgroup that marched it."""
    n_steps = N_STEPS                                                     # (steps of each of the two series)
    queued, got = child(tmp, n_sub, HEAT_AMD_FUSED_ROOM="3", HEAT_AMD_FUSED_PERSIST="1")
    assert queued and queued == [(True, 3, 10, queued[0][3], queued[0][4], n_sub)] * (2 * n_steps), queued
    plain, want = child(tmp, n_sub)
    assert plain == [(False, 10, 10, queued[0][3], queued[0][4], n_sub)] * (2 * n_steps), plain
    assert sorted(got) == sorted(want) and {"trace", "ideal_q", "state"} <= set(got)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
