"""Every ideal-loads instantiation of the cluster-resident march on the GPU (kernels.hip, launch_surfaces_fused: the 18 IDEAL
instantiations of k_surfaces_fast — M in {4, 8, 16} x no-mass facings or not x 4 or 8 wavefronts, and M x 4 or 8 wavefronts
for mixed workgroups).

tests/test_ideal_resident_gpu.py marches four of them with a zone under the rule. Here every one marches a model of its own
(tests/ideal_variants_cases.py: which instantiation a case reaches is held on the host, tests/test_ideal_variants_host.py),
and so do double glazing in mixed workgroups, a workgroup at the kFusedMaxZones = 32 limit of the per-zone LDS arrays, the
work queue on an 8-wavefront mixed and an 8-wavefront no-mass list, and a call with every other term of a series.

The expected result is DEFINED by tests/ideal_loads_ref.py and held through hold_to_the_reference at the project's tolerances
(state, trace and applied at rtol = atol = 1e-9, |dq| <= 1e-9 n_sub S, modes and saturation counts exact); nothing here has a
tolerance of its own. The run is tied to the instantiation its case names by the launch count: enqueue_fused counts one
launch per non-empty workgroup list per call and a series makes one call per step, so n_fused_launches is n_steps x the
number of lists the host-side plan has."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ambient_cases as ac
import helpers
import ideal_variants_cases as ivc
import test_ideal_resident_gpu as tir
import test_series_all_terms_gpu as tat
from heat_amd import HeatBatch, binding
from ideal_loads_ref import accumulate
from ideal_resident_queue_worker import N_STEPS
from test_ideal_loads_gpu import ACC, SAT
from test_ideal_resident_gpu import RES, hold_to_the_reference, run_resident
from test_series_gpu import owned_slots, series_kwargs
from test_series_report_gpu import assert_same

pytestmark = pytest.mark.gpu

ROWS = ("trace", "ideal_q", "applied", "modes")
MARCHED = ivc.INSTANTIATIONS + ["glazing-4", "glazing-8", "zones32"]
_runs = {}


def full_run(oracle, name, n_sub, n_steps):
    """The case marched resident with every statistic, once: (case, out, final state). Asserts what ties the run to its
    instantiation."""
    key = (name, n_sub, n_steps)
    if key not in _runs:
        c = ivc.build(oracle, name, n_steps, n_sub)
        seen = {}
        out, got, (fused, total) = run_resident(*c.args[:2], c.args[9], n_sub, *c.args[2:9], c.opts, seen=seen)
        lists = ivc.plan_of(name)["lists"]
        assert fused == total                                            # every zone is finished by a workgroup
        assert seen["n_fused_launches"] == n_steps * len(lists), (seen, lists)
        _runs[key] = (c, out, got)
    return _runs[key]


def again(c, n_sub, ideal=None, **more):
    md, st, channel, drives, probes, a0, b0, loads, ideal0, w = c.args
    return run_resident(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal0 if ideal is None else ideal, c.opts, **more)[:2]


# ---- 1. every instantiation against the CPU reference ----
@pytest.mark.parametrize("n_sub,n_steps", ivc.CALLS)
@pytest.mark.parametrize("name", MARCHED)
def test_every_instantiation_matches_the_cpu_reference(oracle, name, n_sub, n_steps):
    c, out, got = full_run(oracle, name, n_sub, n_steps)
    md, ideal = c.args[0], c.args[8]
    print("%s: lists %s" % (name, ivc.plan_of(name)["lists"]))
    hold_to_the_reference(name, md, n_sub, ideal, c.ref, c.ref_state, out, got)


# ---- 2. statistics not asked for ----
@pytest.mark.parametrize("name", ["M8-nm1-8w", "M8-mixed-8w"])
def test_statistics_not_asked_for_leave_every_other_bit(oracle, name):
    """Without n_sat_heating / n_sat_cooling the write-back of the resident form has no counter to add to."""
    n_sub, n_steps = ivc.CALLS[0]
    c, full, full_state = full_run(oracle, name, n_sub, n_steps)
    assert (full["ideal"]["n_sat_heating"] > 0).any() and (full["ideal"]["n_sat_cooling"] > 0).any()
    for stats in ((), ("n_sat_heating",)):
        out, got = again(c, n_sub, ideal=dict(c.args[8], stats=stats))
        for k in ROWS:
            assert np.array_equal(full[k], out[k]), (stats, k)
        assert np.array_equal(full_state, got), stats
        assert sorted(out["ideal"]) == sorted(stats)                    # (make_ideal_loads: only those in stats are maintained)
        assert_same(full["ideal"], out["ideal"], stats, "stats=%s" % (stats,))


# ---- 3. exact properties on the new variants ----
EXACT = ["M16-nm1-8w", "M4-mixed-8w", "zones32"]


@pytest.mark.parametrize("name", EXACT)
def test_a_variant_cut_and_resumed_gives_the_bits_of_the_whole(oracle, name):
    n_sub, n_steps = ivc.CALLS[0]
    c, whole, whole_state = full_run(oracle, name, n_sub, n_steps)
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = c.args
    twice, twice_state = again(c, n_sub)
    for k in ROWS:
        assert np.array_equal(whole[k], twice[k]), k                        # two runs, the same bits
    assert_same(whole["ideal"], twice["ideal"], ACC + SAT, "repeat")
    assert np.array_equal(whole_state, twice_state)
    assert_same(accumulate(whole["ideal_q"]), whole["ideal"], ACC, "accumulators")
    assert (whole["ideal"]["n_sat_heating"] > 0).any() and (whole["ideal"]["n_sat_cooling"] > 0).any()
    cut = 5                                                                 # (an odd number of calls before the cut: the zig-zag parity differs)
    got = st.copy()
    with HeatBatch(md, **dict(c.opts, **RES)) as b:
        b.upload_state(got)
        kw = lambda steps: series_kwargs(channel, drives, probes, a0, b0, steps=steps)
        first = b.march_series(w[:cut], n_sub, loads=loads, ideal=ideal, **kw(slice(0, cut)))
        loads2 = dict(loads, thermostats=dict(loads["thermostats"], mode=first["modes"]))
        second = b.march_series(w[cut:], n_sub, loads=loads2, ideal=dict(ideal, resume=first["ideal"], step_base=cut), **kw(slice(cut, None)))
        b.download_state(got)
        assert b.ideal_resident == 1 and b.n_fused_launches == n_steps * len(ivc.plan_of(name)["lists"])
    assert first["failed_step"] == -1 and second["failed_step"] == -1
    for k in ("trace", "ideal_q", "applied"):
        assert np.array_equal(whole[k], np.concatenate([first[k], second[k]])), k
    assert np.array_equal(whole["modes"], second["modes"])
    assert_same(whole["ideal"], second["ideal"], ACC + SAT, "cut at %d" % cut)
    assert np.array_equal(whole_state, got)


@pytest.mark.parametrize("name", EXACT)
def test_unlimited_loads_on_one_constant_channel_hold_it_bit_for_bit(oracle, name):
    n_steps, n_sub = 12, 3
    c = ivc.build(oracle, name, n_steps, n_sub, seed=21, caps="none")
    md, st, channel = c.args[0], c.args[1], c.args[2]
    sp = float(np.median(st[md["zone_slot"]])) + 0.3217
    channel = np.concatenate([channel, np.full((n_steps, 1), sp)], axis=1)
    ch = channel.shape[1] - 1
    Z = int(md["n_zones"])
    zone = c.args[8]["zone"][:3 * Z // 4]                                   # (shuffled: three zones in four)
    ideal = dict(zone=zone, heat_chan=np.full(len(zone), ch), cool_chan=np.full(len(zone), ch))
    c2 = ivc.Case()
    c2.args, c2.opts = (md, st, channel) + c.args[3:4] + (md["zone_slot"],) + c.args[5:8] + (ideal, c.args[9]), c.opts
    out, got = again(c2, n_sub)
    assert np.array_equal(out["trace"][:, zone], np.full((n_steps, len(zone)), sp))
    assert (out["ideal_q"] != 0).any() and not out["ideal"]["n_sat_heating"].any() and not out["ideal"]["n_sat_cooling"].any()
    others = np.setdiff1d(np.arange(Z), zone)
    assert len(others) > 0 and (out["trace"][:, others] != sp).all()


# ---- 4. the work queue on other variants ----
_queue = {}


def queue_child(tmp, name, n_sub, **env):
    """tests/ideal_resident_queue_worker.py on a case of ideal_variants_cases, in a child under the time limit of
    test_ideal_resident_gpu; once a child of either file has died or hung, none is started."""
    key = (name, n_sub, tuple(sorted(env.items())))
    if key in _queue:
        return _queue[key]
    if tir._stopped:
        pytest.fail("not started: " + tir._stopped[0])
    out_path = os.path.join(str(tmp), "%s-%d%s.npz" % (name, n_sub, "".join("-%s" % v for _, v in key[2])))
    full_env = {k: v for k, v in os.environ.items() if k not in ("HEAT_AMD_FUSED_ROOM", "HEAT_AMD_FUSED_RESERVE", "HEAT_AMD_FUSED_PERSIST")}
    full_env.update(env, HEAT_AMD_TRACE="1")
    try:
        r = subprocess.run([sys.executable, tir.WORKER, str(n_sub), out_path, name], capture_output=True, text=True, timeout=tir.TIMEOUT,
                           env=full_env)
    except subprocess.TimeoutExpired:
        tir._stopped.append("%s-%d %s ran into its limit of %.0f s" % (name, n_sub, env, tir.TIMEOUT))
        pytest.fail(tir._stopped[0])
    if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in r.stdout + r.stderr:
        tir._stopped.append("%s-%d %s died with %d" % (name, n_sub, env, r.returncode))
    assert r.returncode == 0 and "IDEAL RESIDENT OK" in r.stdout, "exit %s\n%s\n%s" % (
        r.returncode, r.stdout[-2000:], "\n".join(l for l in r.stderr.splitlines() if "launch" not in l)[-4000:])
    fused = [(bool(m.group(1)),) + tuple(int(x) for x in m.groups()[1:]) for m in tir.FUSED_LINE.finditer(r.stderr)]
    _queue[key] = (fused, dict(np.load(out_path)))
    return _queue[key]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("ideal_variants_queue")


@pytest.mark.parametrize("name,n_sub", [("queue-mixed-8w", 2), ("queue-nm1-8w", 5)])
def test_work_queue_on_other_variants_gives_the_bits_of_one_workgroup_per_block(tmp, name, n_sub):
    """Four blocks on two and five on three persistent workgroups of eight wavefronts: the per-zone arrays of the loads, behind a
    front of LDS twice as large, are refilled for every block a workgroup takes."""
    ((c, g2), blocks), = ivc.plan_of(name)["lists"].items()
    assert blocks > 3 and g2 & 1
    # (a batch with general-layout tiles — the small surfaces of mixed workgroups are such — marches on a stream of its own
    # and leaves part of its room to the batch's stream: enqueue_fused's reserve, min(room / 2, ...) = 1 of a room of 3)
    workgroups = 2 if g2 >> 1 else 3
    queued, got = queue_child(tmp, name, n_sub, HEAT_AMD_FUSED_ROOM="3", HEAT_AMD_FUSED_PERSIST="1")
    assert queued == [(True, workgroups, blocks, c, g2, n_sub)] * (2 * N_STEPS), queued
    plain, want = queue_child(tmp, name, n_sub)
    assert plain == [(False, blocks, blocks, c, g2, n_sub)] * (2 * N_STEPS), plain
    assert sorted(got) == sorted(want) and {"trace", "ideal_q", "applied", "modes", "state"} | set(ACC + SAT) <= set(got)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# ---- 5. every term in one call, resident with ideal loads ----
ALL_TERMS = "clustered_massive-fuse_always"


def run_all_terms(calls):
    """run() of tests/test_series_all_terms_gpu.py on a batch with the opt-in. Returns (results, final state, fused launches)."""
    c = ac.case(ALL_TERMS)
    state, outs = c.state.copy(), []
    with HeatBatch(c.md, **dict(c.opts, **RES)) as b:
        assert b.ideal_resident == 1 and b.n_fused_surfaces > 0
        b.upload_state(state)
        for call in calls:
            w, kw = call(outs[-1] if outs else None)
            outs.append(tat.named(b.march_series(w, c.n_sub, **kw)))
            assert outs[-1]["failed_step"] == -1
        b.download_state(state)
        launches = b.n_fused_launches
    return outs, state, launches


def test_every_term_in_one_resident_ideal_call_equals_the_call_cut_in_two():
    """(Not held against the streamed form: thermostat and vent switches may differ by the rounding of the zone sums.)"""
    c, kwargs = ac.case(ALL_TERMS), tat.everything(ALL_TERMS, True)
    own = owned_slots(c.md)
    assert binding.plan_ideal_resident(c.md, **c.opts) == (True, binding.IDEAL_RESIDENT_OK)
    (one,), state1, launches1 = run_all_terms([lambda _: (c.weather, kwargs())])
    (first, second), state2, launches2 = run_all_terms([lambda _: (c.weather[:tat.CUT], kwargs(slice(0, tat.CUT))),
                                                        lambda before: (c.weather[tat.CUT:], kwargs(slice(tat.CUT, None), before))])
    lists = helpers.plan_lists(c.md, **c.opts)["lists"]
    assert len(lists) > 0 and launches1 == c.n_steps * len(lists) and launches2 == launches1   # every list, every step
    r1, ra, rb = tat.rows_of(one), tat.rows_of(first), tat.rows_of(second)
    assert set(r1) == set(tat.ROWS) | {"ideal_q"}
    for k, v in r1.items():
        assert v.shape[0] == c.n_steps and v.shape[1] > 0, k
        assert tat.same(v, np.concatenate([ra[k], rb[k]])), "%s: %d values differ" % (k, int((v != np.concatenate([ra[k], rb[k]])).sum()))
        assert np.any(np.nan_to_num(v) != 0) and not tat.same(v[0], v[-1]), k   # the term acts, and not alike at every step
    a1, a2 = tat.accumulators_of(one), tat.accumulators_of(second)
    for k, v in a1.items():
        assert tat.same(v, a2[k]), k
    assert tat.same(state1[own], state2[own]) and not tat.same(state1[own], c.state[own])
    assert one["report"]["th_switches"].sum() > 0 and one["air"]["switches"].sum() > 0
