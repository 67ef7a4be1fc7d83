"""Shades of a series on the GPU (include/heat_amd.h, heat_shades / heat_batch_march_series_shaded): the sunlit fraction of the
beam under overhangs, between fins and behind a horizon, formed on the device at every step from the sun vector of the sky's
records, and applied to the sky-driven solar sides and the apertures that refer to a shade.

The rule is this library's own contract; its reference is heat_amd/shading.py (sunlit(): the rule in numpy, line for line)
with sky.incident(..., shade=) and solar_gains.transmitted(..., shade=). Every reference loop here — the per-call path
(test_series_gpu.per_call_series), the oracle loop (oracle_series), the CPU definition of the ideal loads
(ideal_loads_ref.cpu_series) — writes its inputs as gain x channel value: the shaded inputs enter them as channel columns
(shades_cases.reference), so those loops run unchanged. Against the per-call path the series must be equal bit for bit;
against the oracle at the project's rtol = atol = 1e-9. tests/test_shades_host.py asserts the cases' coverage on the CPU."""
import ctypes as C

import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, air_paths, binding, modeldict as mdl
import ideal_loads_ref
import shades_cases as sc
from air_paths_cases import random_air
from ideal_loads_ref import accumulate, cpu_series
from test_ideal_loads_gpu import ACC, SAT, ideal_case
from test_series_gpu import (MODELS, RTOL, assert_close, oracle_series, owned_slots, per_call_series, probes_of_every_kind, series_kwargs,
                             zone_terms, _id)
from test_series_report_gpu import assert_same, replay
from test_sky_gpu import OPTIONS, SKY_MODELS, call_kwargs
from test_solar_gains_gpu import gains_kwargs

pytestmark = pytest.mark.gpu

N_STEPS = sc.N_SUNS


# ---- 1. bit for bit against the per-call path ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model", sorted(SKY_MODELS))
def test_shaded_series_equals_the_per_call_path_bit_for_bit(model, opts):
    md, st = SKY_MODELS[model]()
    own = owned_slots(md)
    for form, n_sub in enumerate((1, 2, 5)):
        rng = np.random.default_rng(270 + n_sub)
        channel, call, ref_drives, args, gains, shades = sc.shades_case(md, rng, N_STEPS)
        probes = probes_of_every_kind(md, rng)
        a0, b0 = zone_terms(md, rng, N_STEPS, form)
        w = mdl.weather_series(N_STEPS * n_sub, md["dt"]).reshape(N_STEPS, n_sub, 3)
        ref_channel, ref_drives, ref_f, ref_p, ref_sum = sc.reference(md, channel, ref_drives, args, gains, shades)
        ref = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(ref)
            ref_trace = per_call_series(b, md, ref, w, ref_channel, ref_drives, probes, a0, b0)
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(got)
            trace, failed, transmitted, ap_sum, sunlit = b.march_series(
                w, n_sub, **sc.shaded_kwargs(channel, call, probes, a0, b0, args, gains, shades))
            b.download_state(got)
        assert failed == -1
        assert np.array_equal(ref_f, sunlit), "n_sub=%d: %d sunlit fractions differ, worst %.3e" % (
            n_sub, int((ref_f != sunlit).sum()), np.abs(ref_f - sunlit).max())
        assert np.array_equal(ref_p, transmitted), "n_sub=%d: %d transmitted powers differ" % (n_sub, int((ref_p != transmitted).sum()))
        assert np.array_equal(ref_sum, ap_sum), "n_sub=%d: %d aperture sums differ" % (n_sub, int((ref_sum != ap_sum).sum()))
        assert np.array_equal(ref_trace, trace), "n_sub=%d: %d trace values differ, worst %.3e" % (
            n_sub, int((ref_trace != trace).sum()), np.abs(ref_trace - trace).max())
        assert np.array_equal(ref[own], got[own]), "n_sub=%d: %d state slots differ" % (n_sub, int((ref[own] != got[own]).sum()))


# ---- 2. against the oracle loop, with sites ----
def test_shaded_series_of_weather_sites_matches_the_oracle_loop(oracle):
    """The four-part model of test_sky_gpu, each site with its own weather, channels, sky records, windows and shades, against
    one oracle loop per site: a shade that reads another site's record shows here — every site's suns are the pattern
    shifted by a number of steps of its own."""
    parts = [mdl.clustered_massive(240, Z=10, seed=31), mdl.rooms_with_windows(200, Z=10, seed=32),
             mdl.glazing_cavity(80, Z=2, seed=33), mdl.ragged_mixed(150, Z=6, seed=34)]
    K = len(parts)
    md, site = mdl.concat([m for m, _ in parts])
    state = np.concatenate([s for _, s in parts])
    n_sub = 3
    rng = np.random.default_rng(218)
    w = mdl.weather_sites(N_STEPS * n_sub, 45.0, K, seed=2).reshape(N_STEPS, n_sub, K, 3)
    S_all = md["n_surfaces"]
    channel = np.zeros((N_STEPS, 8 * K))
    call = {name: (np.full(S_all, -1, np.int32), np.ones(S_all) if name in ("solar_front", "ir_back") else None)
            for name in ("solar_front", "solar_back", "ir_front", "ir_back")}
    record = np.zeros((N_STEPS, K, 8))
    mode = np.zeros(S_all, np.uint8)
    normals = tuple(np.zeros(S_all) for _ in range(3))
    probes, ref_trace, ref_state, ref_f, ref_p, ref_sum, all_gains, all_shades, iters = [], [], [], [], [], [], [], [], 0
    s0 = slot0 = z0 = ap0 = sh0 = hz0 = 0
    a0 = np.zeros((N_STEPS, md["n_zones"]))
    b0 = np.zeros((N_STEPS, md["n_zones"]))
    for k, (m, st) in enumerate(parts):
        ch, cl, rf, args, gains, shades = sc.shades_case(m, rng, N_STEPS)
        pr = probes_of_every_kind(m, rng, 40)
        ta, tb = zone_terms(m, rng, N_STEPS, 2)
        S = m["n_surfaces"]
        channel[:, 8 * k:8 * k + 8] = ch
        for name in call:
            call[name][0][s0:s0 + S] = np.where(cl[name][0] >= 0, cl[name][0] + 8 * k, -1)
            if call[name][1] is not None:
                call[name][1][s0:s0 + S] = cl[name][1]
        record[:, k] = args["record"][:, 0]
        mode[s0:s0 + S] = args["mode"]
        for a in range(3):
            normals[a][s0:s0 + S] = args["normals"][a]
        a0[:, z0:z0 + m["n_zones"]], b0[:, z0:z0 + m["n_zones"]] = ta, tb
        ref = st.copy()
        ref_channel, ref_drives, f, p, total = sc.reference(m, ch, rf, args, gains, shades)
        t, it = oracle_series(oracle, m, ref, w[:, :, k, :], ref_channel, ref_drives, pr, ta, tb)
        all_gains.append(dict(gains, ap_surface=gains["ap_surface"] + s0, en_surface=gains["en_surface"] + s0,
                              en_aperture=gains["en_aperture"] + ap0))
        moved = lambda a, by: np.where(a >= 0, a + by, -1).astype(np.int32)
        all_shades.append(dict(shades, surface=shades["surface"] + s0, horizon=moved(shades["horizon"], hz0),
                               front_shade=moved(shades["front_shade"], sh0), back_shade=moved(shades["back_shade"], sh0),
                               aperture_shade=moved(shades["aperture_shade"], sh0)))
        probes.append(pr + slot0)
        ref_trace.append(t)
        ref_state.append(ref)
        ref_f.append(f)
        ref_p.append(p)
        ref_sum.append(total)
        iters += it
        s0, slot0, z0, ap0 = s0 + S, slot0 + m["n_state"], z0 + m["n_zones"], ap0 + len(gains["ap_surface"])
        sh0, hz0 = sh0 + len(shades["surface"]), hz0 + len(shades["horizon_tan2"])
    assert len(set(tuple(np.nan_to_num(record[:, k, 0], nan=9.0)) for k in range(K))) == K       # every site has suns of its own
    probes, ref_trace, ref_state = np.concatenate(probes), np.concatenate(ref_trace, axis=1), np.concatenate(ref_state)
    gains = {k: np.concatenate([g[k] for g in all_gains]) for k in all_gains[0] if k != "ap_normal"}
    gains["ap_normal"] = tuple(np.concatenate([g["ap_normal"][a] for g in all_gains]) for a in range(3))
    shades = {k: np.concatenate([h[k] for h in all_shades]) for k in all_shades[0] if k not in ("normal", "right", "up")}
    for key in ("normal", "right", "up"):
        shades[key] = tuple(np.concatenate([h[key][a] for h in all_shades]) for a in range(3))
    own = owned_slots(md)
    args = dict(record=record, mode=mode, normals=normals)
    for opts in (dict(), dict(no_fusion=True), dict(use_graph=True), dict(fuse_always=True)):
        got = state.copy()
        with HeatBatch(md, sites=site, **opts) as b:
            b.upload_state(got)
            trace, failed, transmitted, ap_sum, sunlit = b.march_series(
                w, n_sub, **sc.shaded_kwargs(channel, call, probes, a0, b0, args, gains, shades))
            b.download_state(got)
            assert b.nomass_iterations() == iters
        assert failed == -1
        assert np.array_equal(np.concatenate(ref_f, axis=1), sunlit)
        assert np.array_equal(np.concatenate(ref_p, axis=1), transmitted) and np.array_equal(np.concatenate(ref_sum), ap_sum)
        assert_close(ref_trace, trace, "shaded sites trace %s" % _id(opts))
        assert_close(ref_state[own], got[own], "shaded sites final state %s" % _id(opts))


# ---- 3. a shade has no memory ----
@pytest.mark.parametrize("opts", [dict(), dict(use_graph=True), dict(no_fusion=True)], ids=_id)
def test_shaded_series_cut_in_two_equals_the_series_in_one(opts):
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(212)
    n_sub, cut = 3, 7
    channel, call, _, args, gains, shades = sc.shades_case(md, rng, N_STEPS)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, N_STEPS, 2)
    w = mdl.weather_series(N_STEPS * n_sub, md["dt"]).reshape(N_STEPS, n_sub, 3)
    one, two = st.copy(), st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(one)
        trace1, _, p1, sum1, f1 = b.march_series(w, n_sub, **sc.shaded_kwargs(channel, call, probes, a0, b0, args, gains, shades))
        b.download_state(one)
    with HeatBatch(md, **opts) as b:
        b.upload_state(two)
        ta, _, pa, sum_a, fa = b.march_series(w[:cut], n_sub, **sc.shaded_kwargs(channel, call, probes, a0, b0, args, gains, shades, slice(0, cut)))
        tb, _, pb, sum_b, fb = b.march_series(w[cut:], n_sub,
                                              **sc.shaded_kwargs(channel, call, probes, a0, b0, args, gains, shades, slice(cut, None), sum_a))
        b.download_state(two)
    assert np.array_equal(trace1, np.concatenate([ta, tb])) and np.array_equal(p1, np.concatenate([pa, pb]))
    assert np.array_equal(f1, np.concatenate([fa, fb])) and ((f1 > 0) & (f1 < 1)).any()
    assert np.array_equal(sum1, sum_b) and np.array_equal(one, two)


def test_no_sub_timestep_still_evaluates_the_shades():
    md, st = MODELS["ragged_mixed"]()
    rng = np.random.default_rng(220)
    channel, call, ref_drives, args, gains, shades = sc.shades_case(md, rng, N_STEPS)
    probes = probes_of_every_kind(md, rng)
    _, _, ref_f, ref_p, ref_sum = sc.reference(md, channel, ref_drives, args, gains, shades)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, transmitted, ap_sum, sunlit = b.march_series(
            None, 0, n_steps=N_STEPS, **sc.shaded_kwargs(channel, call, probes, None, None, args, gains, shades))
    assert failed == -1 and np.array_equal(trace, np.tile(st[probes], (N_STEPS, 1)))
    assert np.array_equal(ref_f, sunlit) and np.array_equal(ref_p, transmitted) and np.array_equal(ref_sum, ap_sum)


# ---- 4. no shades is the call without shades ----
def test_no_shades_and_shades_that_shade_nothing_are_the_call_without_shades():
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(223)
    n_sub = 2
    channel, call, _, args, gains, shades = sc.shades_case(md, rng, N_STEPS)
    probes = probes_of_every_kind(md, rng)
    w = mdl.weather_series(N_STEPS * n_sub, md["dt"]).reshape(N_STEPS, n_sub, 3)
    kw = gains_kwargs(channel, call, probes, None, None, args, gains)          # the sky and the gains of the case, and no shades
    plain = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(plain)
        trace, failed, p, total = b.march_series(w, n_sub, **kw)
        b.download_state(plain)
    assert failed == -1
    transparent = sc.transparent_shades(md, args, gains)
    for what in (None, {}, transparent):
        same = st.copy()
        with HeatBatch(md) as b:
            b.upload_state(same)
            out = b.march_series(w, n_sub, shades=what, **kw)
            b.download_state(same)
        assert np.array_equal(trace, out[0]) and out[1] == -1 and np.array_equal(p, out[2]) and np.array_equal(total, out[3])
        assert np.array_equal(plain, same)
        if what is not None:
            assert out[4].shape == (N_STEPS, len(what.get("surface", ())))
            assert set(np.unique(out[4])) <= {0.0, 1.0}
    assert (out[4] == 1.0).any() and (out[4] == 0.0).any()
    # shades == NULL through the new entry point: the series without shades
    null = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(null)
        s, keep = binding.make_series(w, n_sub, **{k: v for k, v in kw.items() if k not in ("sky", "gains")})
        k, kkeep = binding.make_sky(**kw["sky"])
        g, gkeep = binding.make_solar_gains(**kw["gains"])
        t1, p1, f1, lit = np.zeros_like(trace), np.zeros_like(p), C.c_int32(5), np.full((N_STEPS, 3), 7.0)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert b._L.heat_batch_march_series_shaded(b._h, C.byref(s), C.byref(k), None, C.byref(g), None, None, None, None, dp(t1), None, None,
                                                   dp(p1), None, dp(lit), C.byref(f1)) == 0
        b.download_state(null)
    assert f1.value == -1 and np.array_equal(trace, t1) and np.array_equal(p, p1) and np.array_equal(plain, null) and np.all(lit == 7.0)
    # a plain series after a shaded one: the bits of a fresh batch
    after = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        shaded = b.march_series(w, n_sub, shades=shades, **kw)
        assert not np.array_equal(shaded[0], trace) and not np.array_equal(shaded[2], p)
        b.upload_state(after)
        t2, _, p2, total2 = b.march_series(w, n_sub, **kw)
        b.download_state(after)
    assert np.array_equal(trace, t2) and np.array_equal(p, p2) and np.array_equal(total, total2) and np.array_equal(plain, after)


# ---- 5. with loads, air paths, ideal loads and a report in the same call ----
def test_shades_with_loads_air_paths_ideal_loads_and_a_report(oracle, monkeypatch):
    """The reference is ideal_loads_ref.cpu_series, whose zone terms of a step come from test_zone_loads_gpu.host_rule; the air
    paths' rule (heat_amd.air_paths.apply) is applied behind it on the same zone temperatures — the order of the device."""
    model, n_sub = "ragged_mixed", 2
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case(model, N_STEPS, n_sub, 300 + n_sub)
    rng = np.random.default_rng(241)
    channel, call, ref_drives, args, gains, shades = sc.shades_case(md, rng, N_STEPS, channel, drives)
    channel, air, _ = random_air(md, st, rng, N_STEPS, channel)
    P = len(probes)
    groups = [(probes[rng.integers(0, P, n)], rng.uniform(-2.0, 3.0, n)) for n in (5, 0, 40)]
    report = dict(stats=("min", "step_min", "max", "step_max", "sum"), group_trace=True, groups=groups)
    ref_channel, ref_drives, ref_f, ref_p, ref_sum = sc.reference(md, channel, ref_drives, args, gains, shades)
    air_state = np.zeros(len(air["target"]), np.uint8)
    ref_q = []
    host_rule = ideal_loads_ref.host_rule

    def with_paths(T, row, za, zb, lds, modes):
        za, zb, applied = host_rule(T, row, za, zb, lds, modes)
        za, zb, q = air_paths.apply(T, row, za, zb, air, air_state)
        ref_q.append(q)
        return za, zb, applied

    monkeypatch.setattr(ideal_loads_ref, "host_rule", with_paths)
    ref_state = st.copy()
    ref = cpu_series(oracle, md, ref_state, w, n_sub, ref_channel, ref_drives, probes, loads, ideal, a0, b0)
    monkeypatch.undo()
    ref_q = np.array(ref_q)
    assert ref["n_heat"] > 0 and ref["n_cool"] > 0 and ref["n_free"] > 0 and (ref["applied"] != 0).any() and (ref_q != 0).any()
    assert ref["margin"] > 1e-7                           # (test_ideal_loads_gpu: the counts cannot depend on rounding)

    def kwargs(steps=slice(None), ap_sum=None):
        return sc.shaded_kwargs(channel, call, probes, a0, b0, args, gains, shades, steps, ap_sum)

    got = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(got)
        out = b.march_series(w, n_sub, loads=loads, ideal=ideal, report=report, air=air, **kwargs())
        b.download_state(got)
    assert out["failed_step"] == -1
    assert np.array_equal(ref_f, out["sunlit"]) and np.array_equal(ref_p, out["transmitted"]) and np.array_equal(ref_sum, out["ap_sum"])
    # at test_ideal_loads_gpu's tolerances
    assert_close(ref["trace"], out["trace"], "shades + ideal trace")
    own = owned_slots(md)
    assert_close(ref_state[own], got[own], "shades + ideal final state")
    assert_close(ref["applied"], out["applied"], "shades + ideal applied")
    assert_close(ref_q, out["air"]["path_q"], "shades + ideal path_q")
    assert np.array_equal(ref["modes"], out["modes"]) and np.array_equal(air_state, out["air"]["state"])
    dq = np.abs(out["ideal_q"] - ref["ideal_q"]) / ref["scale"]
    print("ideal_q: worst |dq| / S = %.3e (bound %.1e)" % (dq.max(), 1e-9 * n_sub))
    assert np.all(np.isfinite(out["ideal_q"])) and dq.max() <= 1e-9 * n_sub
    for k in SAT:
        assert np.array_equal(ref[k], out["ideal"][k]), k
    # the report: exactly the rules over this call's own rows, and the group sums within sum |w| tol of the reference's
    where = {int(s): i for i, s in enumerate(probes)}
    tol = RTOL * (1.0 + np.abs(ref["trace"]))
    gcols = [np.array([where[int(s)] for s in slots], dtype=np.int64) for slots, _ in groups]
    ref_groups = np.stack([(wt * ref["trace"][:, c]).sum(axis=1) for c, (_, wt) in zip(gcols, groups)], axis=1)
    gtol = np.stack([(np.abs(wt) * tol[:, c]).sum(axis=1) + 1e-12 for c, (_, wt) in zip(gcols, groups)], axis=1)
    rep = out["report"]
    assert np.all(np.abs(rep["group_trace"] - ref_groups) <= gtol)
    mine = replay(np.concatenate([out["trace"], rep["group_trace"]], axis=1))
    assert_same(mine, rep, ("q_min", "q_step_min", "q_max", "q_step_max", "q_sum"), "shades + ideal report")
    assert_same(accumulate(out["ideal_q"]), out["ideal"], ACC, "shades + ideal accumulators")
    # one call and two: the same bits
    cut = 6
    two = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(two)
        first = b.march_series(w[:cut], n_sub, loads=loads, ideal=ideal, report=report, air=air, **kwargs(slice(0, cut)))
        loads2 = dict(loads, thermostats=dict(loads["thermostats"], mode=first["modes"]))
        air2 = dict(air, **{k: first["air"][k] for k in ("state", "sum_q", "steps_open", "switches")})
        second = b.march_series(w[cut:], n_sub, loads=loads2, ideal=dict(ideal, resume=first["ideal"], step_base=cut),
                                report=dict(report, resume=first["report"], step_base=cut), air=air2,
                                **kwargs(slice(cut, None), first["ap_sum"]))
        b.download_state(two)
    for k in ("trace", "ideal_q", "applied", "transmitted", "sunlit"):
        assert np.array_equal(out[k], np.concatenate([first[k], second[k]])), k
    assert np.array_equal(out["air"]["path_q"], np.concatenate([first["air"]["path_q"], second["air"]["path_q"]]))
    for k in ("state", "sum_q", "steps_open", "switches"):
        assert np.array_equal(out["air"][k], second["air"][k]), k
    assert np.array_equal(out["report"]["group_trace"], np.concatenate([first["report"]["group_trace"], second["report"]["group_trace"]]))
    assert np.array_equal(out["modes"], second["modes"]) and np.array_equal(out["ap_sum"], second["ap_sum"])
    assert_same(out["ideal"], second["ideal"], ACC + SAT, "cut at %d" % cut)
    assert_same(out["report"], second["report"], ("q_min", "q_step_min", "q_max", "q_step_max", "q_sum"), "cut at %d" % cut)
    assert np.array_equal(got, two)


# ---- 6. refusals through the batch ----
def test_bad_shades_and_sharded_batches_are_refused_by_the_march():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    S = int(md["n_surfaces"])
    rng = np.random.default_rng(229)
    n_steps, n_sub = 3, 1
    w = np.zeros((n_steps, n_sub, 3))
    mode = np.zeros(S, np.uint8)
    mode[::2] = 1                                                            # the fronts of the even surfaces are sky-driven
    sky = dict(record=np.abs(rng.normal(size=(n_steps, 1, 8))), mode=mode)
    normal = (np.zeros(10), -np.ones(10), np.zeros(10))
    right, up = sc.shading.frame_of(normal)
    front = np.full(S, -1, np.int32)
    front[::2] = np.arange(0, S, 2) % 10
    shades = dict(surface=np.arange(10) * 17, normal=normal, right=right, up=up, width=np.full(10, 1.2), height=np.full(10, 1.5),
                  overhang_depth=np.full(10, 0.6), overhang_gap=np.full(10, 0.2), front_shade=front)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        bad = front.copy()
        bad[131] = 4
        with pytest.raises(HeatError) as e:                                  # a shade on a side without a sky bit
            b.march_series(w, n_sub, sky=sky, shades=dict(shades, front_shade=bad))
        assert e.value.code == -4 and "surface 131:" in str(e.value)
        back = np.full(S, -1, np.int32)
        back[130] = 4
        with pytest.raises(HeatError) as e:                                  # ... the back of a surface whose front has one
            b.march_series(w, n_sub, sky=sky, shades=dict(shades, back_shade=back))
        assert e.value.code == -4 and "surface 130:" in str(e.value)
        depth = shades["overhang_depth"].copy()
        depth[6] = np.nan
        with pytest.raises(HeatError) as e:                                  # a depth that is not finite
            b.march_series(w, n_sub, sky=sky, shades=dict(shades, overhang_depth=depth))
        assert e.value.code == -1 and "shade 6:" in str(e.value)
        with pytest.raises(HeatError) as e:                                  # shades without records
            b.march_series(w, n_sub, shades=dict(shades, front_shade=None))
        assert e.value.code == -1 and "shade 0" in str(e.value)
        # refused before any device work: every slot the batch owns is what was uploaded, to the bit
        own = owned_slots(md)
        behind = st.copy()
        behind[own] = np.nan
        b.download_state(behind)
        assert np.array_equal(behind[own], st[own])
        # ... and the batch marches good shades afterwards
        trace, failed, sunlit = b.march_series(w, n_sub, probes=md["zone_slot"], sky=sky, shades=shades)
        assert failed == -1 and np.all(np.isfinite(trace)) and sunlit.shape == (n_steps, 10) and np.all((sunlit >= 0) & (sunlit <= 1))
        b.download_state(behind)
        assert not np.array_equal(behind[own], st[own])                      # (a series that runs does move them)
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, n_sub, sky=sky, shades=shades)
        assert e.value.code == -1 and "sharded" in str(e.value)
