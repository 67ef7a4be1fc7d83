"""Blinds of a series on the GPU (include/heat_amd.h, heat_blinds / heat_batch_march_series_blinds): movable solar protection
that rides on shades — closed by the irradiance on the shade's plane and a zone temperature only the device holds, or following
a position channel — formed on the device at every step between the shades and their consumers.

The rule is this library's own contract; its reference is heat_amd/blinds.py (incident_on(), apply(): the rule in numpy, line
for line) inside a LOOP WITH FEEDBACK (blinds_cases.loop): before march call k the host reads the zone temperatures the state
holds, applies the rule, forms the shaded inputs of the step from the effective factors with sky.incident(..., shade=) and
solar_gains.transmitted(..., shade=) / received, writes them and marches once. Against that loop through the library's own
per-call path the series must be equal bit for bit; against the same loop through the oracle at the project's
rtol = atol = 1e-9, with positions and states equal exactly (the loop records how far its comparisons were from a tie).
tests/test_blinds_host.py asserts the cases' coverage on the CPU."""
import ctypes as C

import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, binding, modeldict as mdl
import blinds_cases as bc
import shades_cases as sc
from air_paths_cases import random_air
from test_ideal_loads_gpu import ideal_case
from test_series_gpu import MODELS, assert_close, owned_slots, probes_of_every_kind, zone_terms, _id
from test_sky_gpu import OPTIONS, SKY_MODELS

pytestmark = pytest.mark.gpu

N_STEPS = bc.N_STEPS
SMALL = sorted(name for name in SKY_MODELS if not name.endswith("_large"))     # a few hundred surfaces each
MARGIN = 1e-6      # how far every comparison of the oracle loop must be from a tie for positions to be compared exactly


def weather_of(md, n_sub):
    return mdl.weather_series(N_STEPS * n_sub, md["dt"]).reshape(N_STEPS, n_sub, 3)


def same_series(ref, want_state, c, out, got_state, own, what):
    """A loop's result against (trace, failed, transmitted, ap_sum, sunlit, blinds) of a series, bit for bit."""
    trace, failed, transmitted, ap_sum, sunlit, blinds = out
    assert failed == -1
    bc.same_blinds(ref, blinds, what + ": ")
    assert np.array_equal(c.f, sunlit), "%s: sunlit keeps the geometric fraction" % what
    assert np.array_equal(ref["transmitted"], transmitted), "%s: %d transmitted powers differ" % (what, int((ref["transmitted"] != transmitted).sum()))
    assert np.array_equal(ref["ap_sum"], ap_sum), "%s: aperture sums differ" % what
    assert np.array_equal(ref["trace"], trace), "%s: %d trace values differ, worst %.3e" % (
        what, int((ref["trace"] != trace).sum()), np.abs(ref["trace"] - trace).max())
    assert np.array_equal(want_state[own], got_state[own]), "%s: %d state slots differ" % (what, int((want_state[own] != got_state[own]).sum()))


# ---- 1. bit for bit against the per-call loop with feedback ----
@pytest.mark.parametrize("opts", OPTIONS + [dict(fuse_always=True)], ids=_id)
@pytest.mark.parametrize("model", SMALL)
def test_blinded_series_equals_the_per_call_loop_bit_for_bit(model, opts):
    md, st = SKY_MODELS[model]()
    own = owned_slots(md)
    for form, n_sub in enumerate((1, 2, 5)):
        rng = np.random.default_rng(470 + n_sub)
        c = bc.blinds_case(md, st, rng)
        probes = probes_of_every_kind(md, rng)
        a0, b0 = zone_terms(md, rng, N_STEPS, form)
        w = weather_of(md, n_sub)
        want = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(want)
            ref = bc.loop(c, want, bc.marcher(b, c, w, a0, b0), probes)
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(got)
            out = b.march_series(w, n_sub, **bc.blinded_kwargs(c, probes, a0, b0))
            b.download_state(got)
        same_series(ref, want, c, out, got, own, "n_sub=%d" % n_sub)
        # the run itself took the rule's branches: blinds closed, reopened, held by hysteresis; positions in between and clamped
        cov = bc.coverage(c, ref)
        print("n_sub=%d: %s, margins %s" % (n_sub, cov, ref["margin"]))
        assert cov["closed"] > 0 and cov["reopened"] > 0 and cov["both"] > 0 and cov["held"] > 0 and cov["fractional"] > 0 and cov["clamped"] > 0, cov
        gated = c.kind >= 4
        assert ref["carry"]["switches"][gated].any() and out[5]["steps_closed"][gated].any()


# ---- 2. against the oracle loop, with sites ----
def sites_case(seed=418):
    """The four-part model of test_shades_gpu, each site with its own weather, channels, sky records, windows, shades and
    blinds. Returns the joined model and call, and per part the case, its probes and zone terms."""
    parts = [mdl.clustered_massive(240, Z=10, seed=31), mdl.rooms_with_windows(200, Z=10, seed=32),
             mdl.glazing_cavity(80, Z=2, seed=33), mdl.ragged_mixed(150, Z=6, seed=34)]
    K = len(parts)
    md, site = mdl.concat([m for m, _ in parts])
    rng = np.random.default_rng(seed)
    cases = []
    for m, st in parts:
        c = bc.blinds_case(m, st, rng)
        cases.append((c, probes_of_every_kind(m, rng, 40), zone_terms(m, rng, N_STEPS, 2)))
    S_all, Z_all = md["n_surfaces"], md["n_zones"]
    width = [c.channel.shape[1] for c, _, _ in cases]
    base = np.concatenate([[0], np.cumsum(width)])
    channel = np.concatenate([c.channel for c, _, _ in cases], axis=1)
    call = {name: (np.full(S_all, -1, np.int32), np.ones(S_all) if name in ("solar_front", "ir_back") else None)
            for name in ("solar_front", "solar_back", "ir_front", "ir_back")}
    record, mode = np.zeros((N_STEPS, K, 8)), np.zeros(S_all, np.uint8)
    normals = tuple(np.zeros(S_all) for _ in range(3))
    a0, b0 = np.zeros((N_STEPS, Z_all)), np.zeros((N_STEPS, Z_all))
    probes, all_gains, all_shades, all_blinds = [], [], [], []
    s0 = slot0 = z0 = ap0 = sh0 = hz0 = 0
    moved = lambda a, by: np.where(a >= 0, a + by, -1).astype(np.int32)
    for k, (c, pr, (ta, tb)) in enumerate(cases):
        m, S = c.md, c.md["n_surfaces"]
        for name in call:
            call[name][0][s0:s0 + S] = moved(c.call[name][0], base[k])
            if call[name][1] is not None:
                call[name][1][s0:s0 + S] = c.call[name][1]
        record[:, k] = c.args["record"][:, 0]
        mode[s0:s0 + S] = c.args["mode"]
        for a in range(3):
            normals[a][s0:s0 + S] = c.args["normals"][a]
        a0[:, z0:z0 + m["n_zones"]], b0[:, z0:z0 + m["n_zones"]] = ta, tb
        g, h, bl = c.gains, c.shades, c.blinds
        all_gains.append(dict(g, ap_surface=g["ap_surface"] + s0, en_surface=g["en_surface"] + s0, en_aperture=g["en_aperture"] + ap0))
        all_shades.append(dict(h, surface=h["surface"] + s0, horizon=moved(h["horizon"], hz0), front_shade=moved(h["front_shade"], sh0),
                               back_shade=moved(h["back_shade"], sh0), aperture_shade=moved(h["aperture_shade"], sh0)))
        all_blinds.append(dict(bl, shade=bl["shade"] + sh0, zone=moved(bl["zone"], z0), pos_chan=moved(bl["pos_chan"], base[k]),
                               set_chan=moved(bl["set_chan"], base[k]), enable_chan=moved(bl["enable_chan"], base[k])))
        probes.append(pr + slot0)
        s0, slot0, z0, ap0 = s0 + S, slot0 + m["n_state"], z0 + m["n_zones"], ap0 + len(g["ap_surface"])
        sh0, hz0 = sh0 + len(h["surface"]), hz0 + len(h["horizon_tan2"])
    gains = {k: np.concatenate([g[k] for g in all_gains]) for k in all_gains[0] if k != "ap_normal"}
    gains["ap_normal"] = tuple(np.concatenate([g["ap_normal"][a] for g in all_gains]) for a in range(3))
    shades = {k: np.concatenate([h[k] for h in all_shades]) for k in all_shades[0] if k not in ("normal", "right", "up")}
    for key in ("normal", "right", "up"):
        shades[key] = tuple(np.concatenate([h[key][a] for h in all_shades]) for a in range(3))
    blinds = {k: np.concatenate([x[k] for x in all_blinds]) for k in all_blinds[0]}
    kw = dict(sc.shaded_kwargs(channel, call, np.concatenate(probes), a0, b0, dict(record=record, mode=mode, normals=normals), gains, shades),
              blinds=blinds)
    return md, site, np.concatenate([s for _, s in parts]), cases, kw


def sites_reference(oracle, cases, w):
    """One oracle loop with feedback per site. Returns the joined results and the smallest margins."""
    refs, states, iters = [], [], []
    for k, (c, pr, (ta, tb)) in enumerate(cases):
        state = c.state.copy()
        refs.append(bc.loop(c, state, bc.oracle_marcher(oracle.OracleModel(c.md), w[:, :, k, :], ta, tb, iters), pr))
        states.append(state)
    ref = {key: np.concatenate([r[key] for r in refs], axis=-1) for key in ("trace", "position", "incident", "transmitted", "ap_sum")}
    ref["carry"] = {key: np.concatenate([r["carry"][key] for r in refs]) for key in refs[0]["carry"]}
    ref["f"] = np.concatenate([c.f for c, _, _ in cases], axis=1)
    margin = {key: min(r["margin"][key] for r in refs) for key in ("I", "T")}
    return ref, np.concatenate(states), sum(iters), margin


def test_blinded_series_of_weather_sites_matches_the_oracle_loop(oracle):
    md, site, state, cases, kw = sites_case()
    n_sub, K = 3, len(cases)
    w = mdl.weather_sites(N_STEPS * n_sub, 45.0, K, seed=2).reshape(N_STEPS, n_sub, K, 3)
    ref, ref_state, iters, margin = sites_reference(oracle, cases, w)
    print("margins of the oracle loop: |I - threshold| >= %.3e, |T - (set +- d)| >= %.3e" % (margin["I"], margin["T"]))
    # no comparison of the reference is within rounding of a tie: the decisions cannot differ between device and oracle
    assert margin["I"] > MARGIN and margin["T"] > MARGIN, margin
    cov = [bc.coverage(c, dict(position=ref["position"][:, k * bc.N_BLINDS:(k + 1) * bc.N_BLINDS],
                               incident=ref["incident"][:, k * bc.N_BLINDS:(k + 1) * bc.N_BLINDS])) for k, (c, _, _) in enumerate(cases)]
    assert all(v["closed"] > 0 and v["reopened"] > 0 for v in cov), cov
    assert len(set(tuple(np.nan_to_num(kw["sky"]["record"][:, k, 0], nan=9.0)) for k in range(K))) == K       # every site has suns of its own
    own = owned_slots(md)
    for opts in (dict(), dict(no_fusion=True), dict(use_graph=True), dict(fuse_always=True)):
        got = state.copy()
        with HeatBatch(md, sites=site, **opts) as b:
            b.upload_state(got)
            trace, failed, transmitted, ap_sum, sunlit, blinds = b.march_series(w, n_sub, **kw)
            b.download_state(got)
            assert b.nomass_iterations() == iters
        assert failed == -1
        # exactly: the sunlit fractions, the irradiance on the shades' planes (neither depends on a zone), every position and state
        assert np.array_equal(ref["f"], sunlit) and np.array_equal(ref["incident"], blinds["incident"])
        bc.same_blinds(ref, blinds, "sites %s: " % _id(opts))
        assert_close(ref["transmitted"], transmitted, "blinded sites transmitted %s" % _id(opts))
        assert_close(ref["ap_sum"], ap_sum, "blinded sites ap_sum %s" % _id(opts))
        assert_close(ref["trace"], trace, "blinded sites trace %s" % _id(opts))
        assert_close(ref_state[own], got[own], "blinded sites final state %s" % _id(opts))


# ---- 3. a cut carries state and accumulators; arrays not asked for ----
@pytest.mark.parametrize("opts", [dict(), dict(use_graph=True), dict(no_fusion=True)], ids=_id)
def test_blinded_series_cut_in_two_equals_the_series_in_one(opts):
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(412)
    n_sub, cut = 3, 7
    c = bc.blinds_case(md, st, rng)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, N_STEPS, 2)
    w = weather_of(md, n_sub)
    one, two, bare = st.copy(), st.copy(), st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(one)
        t1, _, p1, sum1, f1, bl1 = b.march_series(w, n_sub, **bc.blinded_kwargs(c, probes, a0, b0))
        b.download_state(one)
    with HeatBatch(md, **opts) as b:
        b.upload_state(two)
        ta, _, pa, sum_a, fa, bla = b.march_series(w[:cut], n_sub, **bc.blinded_kwargs(c, probes, a0, b0, slice(0, cut)))
        tb, _, pb, sum_b, fb, blb = b.march_series(w[cut:], n_sub, **bc.blinded_kwargs(c, probes, a0, b0, slice(cut, None), sum_a, carry=bla))
        b.download_state(two)
    assert np.array_equal(t1, np.concatenate([ta, tb])) and np.array_equal(p1, np.concatenate([pa, pb])) and np.array_equal(f1, np.concatenate([fa, fb]))
    for key in ("position", "incident"):
        both = np.concatenate([bla[key], blb[key]])
        assert np.array_equal(bl1[key], both, equal_nan=True), key
    for key in ("state",) + bc.ACC:
        assert np.array_equal(bl1[key], blb[key]), key
    assert np.array_equal(sum1, sum_b) and np.array_equal(one, two)
    assert bla["state"].any() and not np.array_equal(bla["switches"], blb["switches"])       # (the cut does carry something)
    # neither array of rows and no accumulator asked for: no other bit changes
    with HeatBatch(md, **opts) as b:
        b.upload_state(bare)
        t0, f0, p0, sum0, s0, bl0 = b.march_series(w, n_sub, position=False, blind_incident=False,
                                                   **bc.blinded_kwargs(c, probes, a0, b0, blinds=dict(c.blinds, stats=())))
        b.download_state(bare)
    assert f0 == -1 and bl0["position"].shape == (0, bc.N_BLINDS) and bl0["incident"].shape == (0, bc.N_BLINDS) and set(bl0) == {"position", "incident", "state"}
    assert np.array_equal(t0, t1) and np.array_equal(p0, p1) and np.array_equal(sum0, sum1) and np.array_equal(bl0["state"], bl1["state"])
    assert np.array_equal(bare, one)


# ---- 4. no blinds is the call without blinds ----
def test_no_blinds_and_blinds_that_never_close_are_the_call_without_blinds():
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(423)
    n_sub = 2
    c = bc.blinds_case(md, st, rng)
    probes = probes_of_every_kind(md, rng)
    w = weather_of(md, n_sub)
    kw = sc.shaded_kwargs(c.channel, c.call, probes, None, None, c.args, c.gains, c.shades)     # the shades of the case, and no blinds
    plain = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(plain)
        trace, failed, p, total, sunlit = b.march_series(w, n_sub, **kw)
        b.download_state(plain)
    assert failed == -1
    # blinds that never close: every blind controlled, its closing threshold the largest finite double (an infinite one is
    # refused: the thresholds of a controlled blind are finite), with zones, setpoints and enable channels as the case has them
    never = dict(c.blinds, pos_chan=None, irr_close=np.full(bc.N_BLINDS, np.finfo(np.float64).max))
    for what in (None, {}, never):
        same = st.copy()
        with HeatBatch(md) as b:
            b.upload_state(same)
            out = b.march_series(w, n_sub, blinds=what, **kw)
            b.download_state(same)
        assert np.array_equal(trace, out[0]) and out[1] == -1 and np.array_equal(p, out[2]) and np.array_equal(total, out[3])
        assert np.array_equal(sunlit, out[4]) and np.array_equal(plain, same)
        if what is not None:
            n = len(what.get("shade", ()))
            assert out[5]["position"].shape == (N_STEPS, n) and not out[5]["position"].any() and not out[5]["state"].any()
            assert not out[5]["switches"].any() and not out[5]["steps_closed"].any()
    assert np.array_equal(out[5]["incident"], c.I[:, c.blinds["shade"]])
    # blinds == NULL through the new entry point: the series without blinds
    null = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(null)
        s, keep = binding.make_series(w, n_sub, **{k: v for k, v in kw.items() if k not in ("sky", "gains", "shades")})
        k, kkeep = binding.make_sky(**kw["sky"])
        g, gkeep = binding.make_solar_gains(**kw["gains"])
        h, hkeep = binding.make_shades(**kw["shades"])
        t1, p1, f1, lit = np.zeros_like(trace), np.zeros_like(p), C.c_int32(5), np.zeros_like(sunlit)
        pos, inc = np.full((N_STEPS, 3), 7.0), np.full((N_STEPS, 3), 8.0)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert b._L.heat_batch_march_series_blinds(b._h, C.byref(s), C.byref(k), C.byref(h), C.byref(g), None, None, None, None, dp(t1), None,
                                                   None, dp(p1), None, dp(lit), None, None, None, None, None, dp(pos), dp(inc),
                                                   C.byref(f1)) == 0
        b.download_state(null)
    assert f1.value == -1 and np.array_equal(trace, t1) and np.array_equal(p, p1) and np.array_equal(sunlit, lit) and np.array_equal(plain, null)
    assert np.all(pos == 7.0) and np.all(inc == 8.0)
    # a plain series after a blinded one: the bits of a fresh batch
    after = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        blinded = b.march_series(w, n_sub, blinds=c.blinds, **kw)
        assert blinded[5]["position"].any() and not np.array_equal(blinded[0], trace) and not np.array_equal(blinded[2], p)
        assert np.array_equal(blinded[4], sunlit)                                           # (sunlit keeps the geometric fraction)
        b.upload_state(after)
        t2, _, p2, total2, f2 = b.march_series(w, n_sub, **kw)
        b.download_state(after)
    assert np.array_equal(trace, t2) and np.array_equal(p, p2) and np.array_equal(total, total2) and np.array_equal(plain, after)


# ---- 5. n_sub == 0 ----
def test_no_sub_timestep_still_evaluates_the_blinds():
    md, st = MODELS["ragged_mixed"]()
    rng = np.random.default_rng(420)
    c = bc.blinds_case(md, st, rng)
    probes = probes_of_every_kind(md, rng)
    ref = bc.loop(c, st.copy(), lambda state, k: None, probes)                               # (nothing marches: the zones stay)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, transmitted, ap_sum, sunlit, blinds = b.march_series(None, 0, n_steps=N_STEPS, **bc.blinded_kwargs(c, probes))
    assert failed == -1 and np.array_equal(trace, np.tile(st[probes], (N_STEPS, 1)))
    bc.same_blinds(ref, blinds)
    assert np.array_equal(c.f, sunlit) and np.array_equal(ref["transmitted"], transmitted) and np.array_equal(ref["ap_sum"], ap_sum)
    assert blinds["switches"].any() and blinds["steps_closed"].any()


# ---- 6. with loads, an ideal load, air paths and a report in the same call ----
def test_blinds_with_loads_air_paths_ideal_loads_and_a_report_lower_the_cooling():
    """A physical sanity check without a tolerance: with the blinds, which only ever lower what a consumer receives (no factor
    of a closed blind is above 1, no record holds a negative diffuse or ground value), the ideal loads remove less heat."""
    model, n_sub = "ragged_mixed", 2
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case(model, N_STEPS, n_sub, 300 + n_sub)
    rng = np.random.default_rng(441)
    c = bc.blinds_case(md, st, rng, N_STEPS, channel, drives, sunny=True)
    c.channel, air, _ = random_air(md, st, rng, N_STEPS, c.channel)
    assert all(np.all(c.blinds[k] <= 1.0) for k in ("beam_closed", "diffuse_closed", "ground_closed"))
    P = len(probes)
    groups = [(probes[rng.integers(0, P, n)], rng.uniform(-2.0, 3.0, n)) for n in (5, 0, 40)]
    report = dict(stats=("min", "step_min", "max", "step_max", "sum"), group_trace=True, groups=groups)
    out = {}
    for name, blinds in (("blinded", c.blinds), ("plain", None)):
        with HeatBatch(md) as b:
            b.upload_state(st.copy())
            kw = bc.blinded_kwargs(c, probes, a0, b0)
            kw["blinds"] = blinds
            out[name] = b.march_series(w, n_sub, loads=loads, ideal=ideal, report=report, air=air, **kw)
        assert out[name]["failed_step"] == -1 and np.all(np.isfinite(out[name]["ideal_q"]))
    got, plain = out["blinded"], out["plain"]
    assert "blinds" in got and "blinds" not in plain and np.array_equal(got["sunlit"], plain["sunlit"])
    pos = got["blinds"]["position"]
    assert (pos == 1).any() and (pos == 0).any() and got["blinds"]["switches"].any()
    assert got["transmitted"].sum() < plain["transmitted"].sum()
    cooling = lambda o: -np.minimum(o["ideal_q"], 0.0).sum()
    print("cooling over the series: %.6e with the blinds, %.6e without" % (cooling(got), cooling(plain)))
    assert cooling(plain) > 0 and cooling(got) < cooling(plain)
    # one call and two: the same bits, every term's state carried
    cut = 6
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        common = dict(loads=loads, ideal=ideal, report=report, air=air)
        first = b.march_series(w[:cut], n_sub, **common, **bc.blinded_kwargs(c, probes, a0, b0, slice(0, cut)))
        common = dict(loads=dict(loads, thermostats=dict(loads["thermostats"], mode=first["modes"])),
                      ideal=dict(ideal, resume=first["ideal"], step_base=cut), report=dict(report, resume=first["report"], step_base=cut),
                      air=dict(air, **{k: first["air"][k] for k in ("state", "sum_q", "steps_open", "switches")}))
        second = b.march_series(w[cut:], n_sub, **common, **bc.blinded_kwargs(c, probes, a0, b0, slice(cut, None), first["ap_sum"], carry=first["blinds"]))
    for k in ("trace", "ideal_q", "applied", "transmitted", "sunlit"):
        assert np.array_equal(got[k], np.concatenate([first[k], second[k]])), k
    assert np.array_equal(pos, np.concatenate([first["blinds"]["position"], second["blinds"]["position"]]), equal_nan=True)
    for k in ("state",) + bc.ACC:
        assert np.array_equal(got["blinds"][k], second["blinds"][k]), k


# ---- 7. refusals through the batch ----
def test_bad_blinds_and_sharded_batches_are_refused_by_the_march():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    S = int(md["n_surfaces"])
    rng = np.random.default_rng(429)
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
    blinds = dict(shade=np.array([7, 2, 9, 0]), beam_closed=np.full(4, 0.1), diffuse_closed=np.full(4, 0.3), ground_closed=np.full(4, 0.3),
                  irr_close=np.full(4, 0.2), irr_open=np.full(4, 0.1), zone=np.array([-1, 3, -1, 7]), set_chan=np.array([-1, 0, -1, 0]),
                  band=np.full(4, 0.5))
    channel = np.full((n_steps, 1), 10.0)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        for damage, code, who in ((dict(shade=np.array([7, 2, 9, 10])), -4, "blind 3:"), (dict(shade=np.array([7, 2, 7, 0])), -4, "blind 2:"),
                                  (dict(zone=np.array([-1, 8, -1, 7])), -4, "blind 1:"), (dict(set_chan=np.array([-1, 0, -1, 1])), -4, "blind 3:"),
                                  (dict(beam_closed=np.array([0.1, np.nan, 0.1, 0.1])), -1, "blind 1:"),
                                  (dict(irr_open=np.array([0.1, 0.1, 0.3, 0.1])), -1, "blind 2:"),
                                  (dict(irr_close=np.array([np.inf, 0.2, 0.2, 0.2])), -1, "blind 0:"),
                                  (dict(band=np.array([0.5, 0.5, 0.5, -0.5])), -1, "blind 3:"),
                                  (dict(state=np.array([0, 0, 2, 0], np.uint8)), -1, "blind 2:")):
            with pytest.raises(HeatError) as e:
                b.march_series(w, n_sub, channel=channel, sky=sky, shades=shades, blinds=dict(blinds, **damage))
            assert e.value.code == code and who in str(e.value), (damage, str(e.value))
        with pytest.raises(HeatError) as e:                                  # blinds without shades
            b.march_series(w, n_sub, channel=channel, sky=sky, blinds=blinds)
        assert e.value.code == -1 and "blind 0" in str(e.value)
        # refused before any device work: every slot the batch owns is what was uploaded, to the bit
        own = owned_slots(md)
        behind = st.copy()
        behind[own] = np.nan
        b.download_state(behind)
        assert np.array_equal(behind[own], st[own])
        # ... and the batch marches good blinds afterwards
        trace, failed, sunlit, out = b.march_series(w, n_sub, probes=md["zone_slot"], channel=channel, sky=sky, shades=shades, blinds=blinds)
        assert failed == -1 and np.all(np.isfinite(trace)) and out["position"].shape == (n_steps, 4) and set(np.unique(out["position"])) <= {0.0, 1.0}
        assert np.all(np.isfinite(out["incident"])) and out["state"].shape == (4,)
        b.download_state(behind)
        assert not np.array_equal(behind[own], st[own])                      # (a series that runs does move them)
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, n_sub, channel=channel, sky=sky, shades=shades, blinds=blinds)
        assert e.value.code == -1 and "sharded" in str(e.value)
