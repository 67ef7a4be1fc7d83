"""Room radiation of a series on the GPU (include/heat_amd.h, heat_room_radiation / heat_batch_march_series_radiation): the
long-wave irradiance of the faces of a room, formed on the device at every step from sigma T^4 of the faces they see — the node
temperatures the device holds when the step starts — and from channels.

The rule is this library's own contract; its reference is heat_amd/room_radiation.py (emitted() and irradiance(): the rule in
numpy, line for line). The reference loops here are the test's own: before call k they take the state as it is, apply the
rule to the face nodes, write the long-wave slots of the receivers and march one call — through heat_batch_march_ex, where
the series must be equal bit for bit (the rule is exempt from nothing), and through the oracle, at the project's
rtol = atol = 1e-9. tests/test_room_radiation_host.py asserts the cases' coverage on the CPU."""
import ctypes as C

import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, binding, modeldict as mdl, room_radiation as rrm
import room_radiation_cases as rc
import shades_cases as sc
from air_paths_cases import random_air
from test_ideal_loads_gpu import ideal_case
from test_series_gpu import (MODELS, RTOL, assert_close, owned_slots, probes_of_every_kind, term_row, write_inputs, zone_terms, _id)
from test_sky_gpu import OPTIONS

pytestmark = pytest.mark.gpu

N_STEPS = 12
RADIANT_MODELS = {"rooms_with_windows": MODELS["rooms_with_windows"], "ragged_mixed": MODELS["ragged_mixed"],
                  "glazing_cavity": MODELS["glazing_cavity"], "clustered_massive": lambda: mdl.clustered_massive(600, Z=24, seed=3)}


def per_call_radiant_series(b, md, state, weather, channel, ref, probes, a0, b0, rad):
    """The path a radiant series replaces: a state download, the rule on the host and an upload per step."""
    slots = rc.receiver_slots(md, rad)
    trace = np.zeros((len(weather), len(probes)))
    irradiance = np.zeros((len(weather), len(slots)))
    total = np.zeros(len(slots))
    for k in range(len(weather)):
        b.download_state(state)
        write_inputs(md, state, k, channel, ref)
        v = rc.rule(md, state, channel[k], rad, ref)
        state[slots] = v
        b.march(state, weather[k], term_row(a0, k), term_row(b0, k), outputs=b.OUT_ALL)
        trace[k], irradiance[k] = state[probes], v
        total = total + v
    return trace, irradiance, total


# ---- 1. bit for bit against the per-call path ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model", sorted(RADIANT_MODELS))
def test_radiant_series_equals_the_per_call_path_bit_for_bit(model, opts):
    md, st = RADIANT_MODELS[model]()
    own = owned_slots(md)
    for form, n_sub in enumerate((1, 2, 5)):
        rng = np.random.default_rng(330 + n_sub)
        channel, call, ref, rad, info = rc.radiation_case(md, rng, N_STEPS)
        probes = probes_of_every_kind(md, rng)
        a0, b0 = zone_terms(md, rng, N_STEPS, form)
        w = mdl.weather_series(N_STEPS * n_sub, md["dt"]).reshape(N_STEPS, n_sub, 3)
        want = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(want)
            ref_trace, ref_irr, ref_sum = per_call_radiant_series(b, md, want, w, channel, ref, probes, a0, b0, rad)
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(got)
            trace, failed, irradiance, total = b.march_series(w, n_sub, **rc.radiant_kwargs(channel, call, probes, a0, b0, rad))
            b.download_state(got)
        assert failed == -1 and np.all(np.isfinite(trace))
        assert np.array_equal(ref_irr, irradiance), "n_sub=%d: %d irradiances differ, worst %.3e" % (
            n_sub, int((ref_irr != irradiance).sum()), np.abs(ref_irr - irradiance).max())
        assert np.array_equal(ref_sum, total), "n_sub=%d: %d irradiance sums differ" % (n_sub, int((ref_sum != total).sum()))
        assert np.array_equal(ref_trace, trace), "n_sub=%d: %d trace values differ, worst %.3e" % (
            n_sub, int((ref_trace != trace).sum()), np.abs(ref_trace - trace).max())
        assert np.array_equal(want[own], got[own]), "n_sub=%d: %d state slots differ" % (n_sub, int((want[own] != got[own]).sum()))
        assert not np.array_equal(irradiance[0], irradiance[-1])       # (the faces move: the rule follows them)


# ---- 2. against the oracle loop, with sites ----
def test_radiant_series_of_weather_sites_matches_the_oracle_loop(oracle):
    """The four-part model of test_sky_gpu, each site with its own weather, and receivers that see sides of other zones and
    other sites: the oracles of the four parts march in lockstep on one state, the rule applied between their marches."""
    parts = [mdl.clustered_massive(240, Z=10, seed=31), mdl.rooms_with_windows(200, Z=10, seed=32),
             mdl.glazing_cavity(80, Z=2, seed=33), mdl.ragged_mixed(150, Z=6, seed=34)]
    K = len(parts)
    md, site = mdl.concat([m for m, _ in parts])
    state = np.concatenate([s for _, s in parts])
    n_sub = 3
    rng = np.random.default_rng(318)
    w = mdl.weather_sites(N_STEPS * n_sub, 45.0, K, seed=2).reshape(N_STEPS, n_sub, K, 3)
    channel, call, ref, rad, info = rc.radiation_case(md, rng, N_STEPS)
    probes = probes_of_every_kind(md, rng, 120)
    a0, b0 = zone_terms(md, rng, N_STEPS, 2)
    emitter_site = site[rad["en_surface"][rad["en_surface"] >= 0]]
    receiver_site = site[rad["rc_surface"][rad["en_receiver"][rad["en_surface"] >= 0]]]
    assert (emitter_site != receiver_site).any()                        # a receiver sees a side at another site
    slots = rc.receiver_slots(md, rad)
    want = state.copy()
    models = [oracle.OracleModel(m) for m, _ in parts]
    ref_trace, ref_irr, ref_sum, iters = np.zeros((N_STEPS, len(probes))), np.zeros((N_STEPS, len(slots))), np.zeros(len(slots)), 0
    for k in range(N_STEPS):
        write_inputs(md, want, k, channel, ref)
        v = rc.rule(md, want, channel[k], rad, ref)
        want[slots] = v
        slot0 = z0 = 0
        for j, (m, _) in enumerate(parts):
            Z = m["n_zones"]
            code, it = models[j].march(want[slot0:slot0 + m["n_state"]], w[k, :, j, :], a0[k, z0:z0 + Z], b0[k, z0:z0 + Z])
            assert code == 0
            iters += it
            slot0, z0 = slot0 + m["n_state"], z0 + Z
        ref_trace[k], ref_irr[k] = want[probes], v
        ref_sum = ref_sum + v
    own = owned_slots(md)
    for opts in (dict(), dict(no_fusion=True), dict(use_graph=True), dict(fuse_always=True)):
        got = state.copy()
        with HeatBatch(md, sites=site, **opts) as b:
            b.upload_state(got)
            trace, failed, irradiance, total = b.march_series(w, n_sub, **rc.radiant_kwargs(channel, call, probes, a0, b0, rad))
            b.download_state(got)
            assert b.nomass_iterations() == iters
        assert failed == -1
        assert_close(ref_trace, trace, "radiant sites trace %s" % _id(opts))
        assert_close(want[own], got[own], "radiant sites final state %s" % _id(opts))
        # (formed from temperatures that themselves agree only to the tolerance)
        worst = (np.abs(irradiance - ref_irr) / (1.0 + np.abs(ref_irr))).max()
        print("radiant sites irradiance %s: worst |diff| / (1 + |ref|) = %.3e" % (_id(opts), worst))
        assert np.all(np.isfinite(irradiance)) and worst <= RTOL
        assert np.all(np.abs(total - ref_sum) <= N_STEPS * RTOL * (1.0 + np.abs(ref_irr).max(axis=0)))
        assert np.array_equal(irradiance[0], ref_irr[0])                # (step 0 is formed from the uploaded state itself)


# ---- 3. self-consistent in any combination ----
def test_radiation_with_loads_air_paths_ideal_loads_a_report_sky_gains_and_shades():
    """Everything a series can carry in one call; the face nodes of all emitters are among the probes, so the irradiance of
    step k must be the numpy rule applied to row k - 1 of this call's own trace — step 0 to the uploaded state."""
    n_steps, n_sub = sc.N_SUNS, 2
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case("ragged_mixed", n_steps, n_sub, 340)
    rng = np.random.default_rng(341)
    channel, call, _, args, gains, shades = sc.shades_case(md, rng, n_steps, channel, drives)
    channel, air, _ = random_air(md, st, rng, n_steps, channel)
    channel, rcall, ref, rad, info = rc.radiation_case(md, rng, n_steps, channel, {n: (c, drives[n][1]) for n, (c, _) in call.items()})
    S = int(md["n_surfaces"])
    # an input has one source: a receiver takes nothing from the sky either
    mode = args["mode"].copy()
    mode[rad["rc_surface"][rad["rc_side"] == 0]] &= np.uint8(~4 & 0xff)
    mode[rad["rc_surface"][rad["rc_side"] == 1]] &= np.uint8(~8 & 0xff)
    args = dict(args, mode=mode)
    call = {name: (rcall[name][0], call[name][1]) for name in call}
    on = rad["en_surface"] >= 0
    faces = np.unique(rrm.face_slots(md, rad["en_surface"][on], rad["en_side"][on]))
    P = len(probes)
    probes = np.concatenate([probes, faces])
    groups = [(probes[rng.integers(0, P, n)], rng.uniform(-2.0, 3.0, n)) for n in (5, 0, 40)]
    report = dict(stats=("min", "step_min", "max", "step_max", "sum"), group_trace=True, groups=groups)
    kw = dict(sc.shaded_kwargs(channel, call, probes, a0, b0, args, gains, shades), radiation=rad)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        out = b.march_series(w, n_sub, loads=loads, ideal=ideal, report=report, air=air, **kw)
    assert out["failed_step"] == -1 and np.all(np.isfinite(out["trace"]))
    assert out["sunlit"].shape == (n_steps, sc.N_SHADES) and out["transmitted"].shape[0] == n_steps and (out["ideal_q"] != 0).any()
    held = np.full(int(md["n_state"]), np.nan)      # (only the emitters' face nodes are read)
    total = np.zeros(len(rad["rc_surface"]))
    for k in range(n_steps):
        held[faces] = st[faces] if k == 0 else out["trace"][k - 1, P:]
        v = rc.rule(md, held, channel[k], rad, ref)
        assert np.array_equal(v, out["irradiance"][k]), "step %d: %d irradiances differ" % (k, int((v != out["irradiance"][k]).sum()))
        total = total + v
    assert np.array_equal(total, out["sum_irradiance"]) and not np.isnan(total).any()


# ---- 4. the rule has no memory but sum_irradiance ----
@pytest.mark.parametrize("opts", [dict(), dict(use_graph=True), dict(no_fusion=True)], ids=_id)
def test_radiant_series_cut_in_two_equals_the_series_in_one(opts):
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(312)
    n_sub, cut = 3, 5
    channel, call, _, rad, info = rc.radiation_case(md, rng, N_STEPS)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, N_STEPS, 2)
    w = mdl.weather_series(N_STEPS * n_sub, md["dt"]).reshape(N_STEPS, n_sub, 3)
    one, two = st.copy(), st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(one)
        trace1, _, irr1, sum1 = b.march_series(w, n_sub, **rc.radiant_kwargs(channel, call, probes, a0, b0, rad))
        b.download_state(one)
    with HeatBatch(md, **opts) as b:
        b.upload_state(two)
        ta, _, ia, sum_a = b.march_series(w[:cut], n_sub, **rc.radiant_kwargs(channel, call, probes, a0, b0, rad, slice(0, cut)))
        tb, _, ib, sum_b = b.march_series(w[cut:], n_sub, **rc.radiant_kwargs(channel, call, probes, a0, b0, rad, slice(cut, None), sum_a))
        b.download_state(two)
    assert np.array_equal(trace1, np.concatenate([ta, tb])) and np.array_equal(irr1, np.concatenate([ia, ib]))
    assert np.array_equal(sum1, sum_b) and not np.array_equal(sum_a, sum_b) and np.array_equal(one, two)
    # an irradiance array that is not asked for changes no bit of the others
    none = st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(none)
        t0, _, i0, s0 = b.march_series(w, n_sub, irradiance=False, **rc.radiant_kwargs(channel, call, probes, a0, b0, rad))
        b.download_state(none)
    assert i0.shape == (0, len(rad["rc_surface"])) and np.array_equal(t0, trace1) and np.array_equal(s0, sum1) and np.array_equal(none, one)


# ---- 5. n_sub == 0 ----
def test_no_sub_timestep_still_evaluates_every_step():
    md, st = MODELS["ragged_mixed"]()
    rng = np.random.default_rng(320)
    channel, call, ref, rad, info = rc.radiation_case(md, rng, N_STEPS)
    channel[:] = channel[0]                                             # (nothing marches: with one row every step is the same)
    probes = probes_of_every_kind(md, rng)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, irradiance, total = b.march_series(None, 0, n_steps=N_STEPS, **rc.radiant_kwargs(channel, call, probes, None, None, rad))
    v = rc.rule(md, st, channel[0], rad, ref)
    assert failed == -1 and np.array_equal(trace, np.tile(st[probes], (N_STEPS, 1)))
    assert np.array_equal(irradiance, np.tile(v, (N_STEPS, 1))) and (v != 0).any()
    want = np.zeros(len(v))
    for k in range(N_STEPS):
        want = want + v
    assert np.array_equal(total, want)


# ---- 6. no radiation is the call without radiation ----
def test_absent_and_empty_radiation_are_the_call_without_radiation():
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(323)
    n_sub = 2
    channel, call, _, rad, info = rc.radiation_case(md, rng, N_STEPS)
    probes = probes_of_every_kind(md, rng)
    w = mdl.weather_series(N_STEPS * n_sub, md["dt"]).reshape(N_STEPS, n_sub, 3)
    kw = rc.radiant_kwargs(channel, call, probes, None, None, rad)
    del kw["radiation"]
    plain = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(plain)
        trace, failed = b.march_series(w, n_sub, **kw)
        b.download_state(plain)
    assert failed == -1
    for what in (None, {}):
        same = st.copy()
        with HeatBatch(md) as b:
            b.upload_state(same)
            out = b.march_series(w, n_sub, radiation=what, **kw)
            b.download_state(same)
        assert np.array_equal(trace, out[0]) and out[1] == -1 and np.array_equal(plain, same)
        if what is not None:
            assert out[2].shape == (N_STEPS, 0) and out[3].shape == (0,)
    # radiation == NULL through the new entry point: the series without it
    null = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(null)
        s, keep = binding.make_series(w, n_sub, **kw)
        t1, f1, irr = np.zeros_like(trace), C.c_int32(5), np.full((N_STEPS, 3), 7.0)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert b._L.heat_batch_march_series_radiation(b._h, C.byref(s), *(None,) * 7, dp(t1), *(None,) * 5, None, dp(irr), C.byref(f1)) == 0
        b.download_state(null)
    assert f1.value == -1 and np.array_equal(trace, t1) and np.array_equal(plain, null) and np.all(irr == 7.0)
    # a plain series after a radiant one: the bits of a fresh batch; and the radiant one differs from it
    after = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        radiant = b.march_series(w, n_sub, radiation=rad, **kw)
        assert radiant[1] == -1 and not np.array_equal(radiant[0], trace)
        b.upload_state(after)
        t2, _ = b.march_series(w, n_sub, **kw)
        b.download_state(after)
    assert np.array_equal(trace, t2) and np.array_equal(plain, after)


# ---- 7. refusals through the batch ----
def test_bad_radiation_and_sharded_batches_are_refused_by_the_march():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    S = int(md["n_surfaces"])
    rng = np.random.default_rng(329)
    n_steps, n_sub = 3, 1
    w = np.zeros((n_steps, n_sub, 3))
    channel = rng.uniform(300.0, 450.0, (n_steps, 2))
    chan = np.full(S, -1, np.int32)
    chan[7] = 1
    n = 20
    rad = dict(rc_surface=np.arange(n) * 3, rc_side=np.zeros(n, np.uint8), en_receiver=np.repeat(np.arange(n), 2),
               en_surface=rng.integers(0, S, 2 * n), en_side=rng.integers(0, 2, 2 * n).astype(np.uint8), en_factor=np.full(2 * n, 0.5))
    series = dict(channel=channel, ir_front=(chan, None), probes=md["zone_slot"])
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        for bad, code, names in ((dict(rc_surface=np.where(np.arange(n) == 4, 7, rad["rc_surface"])), -4, "receiver 4:"),    # has a channel
                                 (dict(rc_surface=np.where(np.arange(n) == 9, 3, rad["rc_surface"])), -4, "receiver 9:"),    # twice
                                 (dict(rc_surface=np.where(np.arange(n) == 2, S, rad["rc_surface"])), -4, "receiver 2:"),
                                 (dict(rc_side=np.where(np.arange(n) == 5, 2, 0).astype(np.uint8)), -1, "receiver 5:"),
                                 (dict(en_factor=np.where(np.arange(2 * n) == 11, np.nan, 0.5)), -1, "entry 11:"),
                                 (dict(en_receiver=np.where(np.arange(2 * n) == 13, n, rad["en_receiver"])), -4, "entry 13:"),
                                 (dict(en_surface=np.where(np.arange(2 * n) == 6, -1, rad["en_surface"]),
                                       en_chan=np.where(np.arange(2 * n) == 6, 2, -1)), -4, "entry 6:")):                   # channel 2 of 2
            with pytest.raises(HeatError) as e:
                b.march_series(w, n_sub, radiation=dict(rad, **bad), **series)
            assert e.value.code == code and names in str(e.value), str(e.value)
        mode = np.zeros(S, np.uint8)
        mode[12] = 4                                                                                # receiver 4's front is the sky's
        with pytest.raises(HeatError) as e:
            b.march_series(w, n_sub, radiation=rad, sky=dict(record=np.ones((n_steps, 1, 8)), mode=mode), **series)
        assert e.value.code == -4 and "receiver 4:" in str(e.value) and "sky" in str(e.value)
        # refused before any device work: every slot the batch owns is what was uploaded, to the bit
        own = owned_slots(md)
        behind = st.copy()
        behind[own] = np.nan
        b.download_state(behind)
        assert np.array_equal(behind[own], st[own])
        # ... and the batch marches a good radiation afterwards
        trace, failed, irradiance, total = b.march_series(w, n_sub, radiation=rad, **series)
        assert failed == -1 and np.all(np.isfinite(trace)) and irradiance.shape == (n_steps, n) and np.all(irradiance > 0)
        b.download_state(behind)
        assert not np.array_equal(behind[own], st[own])                      # (a series that runs does move them)
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, n_sub, radiation=rad, **series)
        assert e.value.code == -1 and "sharded" in str(e.value)
