"""Comfort of a series on the GPU (include/heat_amd.h, heat_comfort / heat_batch_march_series_comfort): the operative
temperature of rooms from the face and zone temperatures only the device holds at the start of a step — reported, accumulated
against limits that are channels, and sensed by thermostats, air paths and blinds where a sensor is its zone's control
temperature.

The rule is this library's own contract; its reference is heat_amd/comfort.py (operative(), control_temperatures(),
accumulate(): the rule in numpy, line for line) inside a LOOP WITH FEEDBACK (comfort_cases.loop): before march call k the host
reads the state, applies the rule, runs the thermostat rule, air_paths.apply(control_T=) and blinds.apply on the control
temperatures, writes the inputs and marches once. Against that loop through the library's own per-call path the series must
be equal bit for bit; against the same loop through the oracle at the project's rtol = atol = 1e-9, with every decision,
count and step equal exactly (tests/test_comfort_host.py asserts on the CPU that no comparison of that loop is within 1e-6
of a tie, and the cases' coverage).

The shapes: 300 sensors (past one 256-lane block, not a multiple of 64), a sensor without entries and one with 130, entries
in shuffled order, a zone with two sensors of which one controls, zones without a sensor, no-mass and two-node walls as
faces (comfort_cases.sensors_of asserts them); one sensor alone in the n_sub == 0 and refusal tests."""
import ctypes as C

import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, binding, comfort as cf, modeldict as mdl
import comfort_cases as cc
from test_series_gpu import MODELS, assert_close, owned_slots, probes_of_every_kind, zone_terms, _id

pytestmark = pytest.mark.gpu

N_STEPS = cc.N_STEPS
CASE_MODELS = {"ragged_mixed": MODELS["ragged_mixed"], "rooms_with_windows": MODELS["rooms_with_windows"],
               "ragged_mixed_28": lambda: mdl.ragged_mixed(700, Z=28, seed=1)}       # a few hundred surfaces each
OPTIONS = [dict(), dict(use_graph=True), dict(no_fusion=True), dict(fuse_always=True)]
MARGIN = 1e-6


def weather_of(md, n_sub, n_steps=N_STEPS):
    return mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)


def run_series(md, st, opts, calls):
    """A fresh batch, the state uploaded, the calls (weather, n_sub, kwargs) made one after the other; each may be a function
    of the named result before. Returns (the named results, the final state)."""
    state, outs = st.copy(), []
    with HeatBatch(md, **opts) as b:
        b.upload_state(state)
        for call in calls:
            w, n_sub, kw = call(outs[-1] if outs else None) if callable(call) else call
            outs.append(cc.named(b.march_series(w, n_sub, **kw)))
            assert outs[-1]["failed_step"] == -1
        b.download_state(state)
    return outs, state


# ---- 1. bit for bit against the per-call loop with feedback ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model", sorted(CASE_MODELS))
def test_series_with_comfort_equals_the_per_call_loop_bit_for_bit(model, opts):
    md, st = CASE_MODELS[model]()
    own = owned_slots(md)
    for form, n_sub in enumerate((1, 2, 5)):
        rng = np.random.default_rng(540 + n_sub)
        c = cc.comfort_case(md, st, rng)
        probes = probes_of_every_kind(md, rng)
        a0, b0 = zone_terms(md, rng, N_STEPS, form)
        w = weather_of(md, n_sub)
        want = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(want)
            ref = cc.loop(c, want, cc.marcher(b, w), probes, a0, b0)
        (got,), state = run_series(md, st, opts, [(w, n_sub, cc.series_kwargs(c, probes, a0, b0))])
        what = "n_sub=%d: " % n_sub
        cc.same_as_loop(ref, got, what)
        assert np.array_equal(c.f, got["sunlit"])
        assert np.array_equal(want[own], state[own]), "%s%d state slots differ" % (what, int((want[own] != state[own]).sum()))
        # the run itself took the rule's branches, and its control sensors are not the air: the controls acted on them
        cov = cc.coverage(c, ref)
        print("%s%s, margins %s" % (what, cov, ref["margin"]))
        assert cov["occupied"] > 0 and cov["unoccupied"] > 0 and cov["below"] + cov["above"] > 0 and cov["min_twice"] + cov["max_twice"] > 0, cov
        ctl = c.comfort["control"] == 1
        assert np.array_equal(ref["Tc"][:, c.comfort["zone"][ctl]], ref["operative"][:, ctl]) and not np.array_equal(ref["Tc"], ref["Tz"])
        assert ref["applied"].any() and ref["carry"]["air"]["switches"].any()


# ---- 2. against the same loop through the oracle ----
def test_series_with_comfort_matches_the_oracle_loop(oracle):
    c, w, probes, a0, b0 = cc.oracle_case()
    ref, ref_state = cc.oracle_loop(oracle, c, w, probes, a0, b0)
    print("margins of the oracle loop: %s" % ref["margin"])
    # no comparison of the reference is within rounding of a tie: the decisions cannot differ between device and oracle
    assert all(v > MARGIN for v in ref["margin"].values()), ref["margin"]
    own = owned_slots(c.md)
    for opts in OPTIONS:
        state = c.state.copy()
        with HeatBatch(c.md, **opts) as b:
            b.upload_state(state)
            got = cc.named(b.march_series(w, cc.ORACLE_N_SUB, **cc.series_kwargs(c, probes, a0, b0)))
            b.download_state(state)
            assert b.nomass_iterations() == ref["iters"]
        cc.same_as_loop(ref, got, "oracle %s: " % _id(opts), close=assert_close)
        assert_close(ref_state[own], state[own], "oracle final state %s" % _id(opts))


# ---- 3. a cut carries every accumulator ----
@pytest.mark.parametrize("opts", [dict(), dict(use_graph=True)], ids=_id)
def test_series_with_comfort_cut_in_two_equals_the_series_in_one(opts):
    md, st = CASE_MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(512)
    n_sub, cut = 3, 7
    c = cc.comfort_case(md, st, rng)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, N_STEPS, 2)
    w = weather_of(md, n_sub)
    (one,), state1 = run_series(md, st, opts, [(w, n_sub, cc.series_kwargs(c, probes, a0, b0))])
    (first, second), state2 = run_series(md, st, opts, [
        (w[:cut], n_sub, cc.series_kwargs(c, probes, a0, b0, slice(0, cut))),
        lambda before: (w[cut:], n_sub, cc.series_kwargs(c, probes, a0, b0, slice(cut, None), carry=cc.carried(before), step_base=cut))])
    for key in ("trace", "applied", "transmitted", "sunlit"):
        assert cc.same_bits(one[key], np.concatenate([first[key], second[key]])), key
    for key in ("operative", "mrt"):
        assert cc.same_bits(one["comfort"][key], np.concatenate([first["comfort"][key], second["comfort"][key]])), key
    assert cc.same_bits(one["air"]["path_q"], np.concatenate([first["air"]["path_q"], second["air"]["path_q"]]))
    assert cc.same_bits(one["blinds"]["position"], np.concatenate([first["blinds"]["position"], second["blinds"]["position"]]))
    for key in cf.ACC:
        assert cc.same_bits(one["comfort"][key], second["comfort"][key]), key
    assert np.array_equal(one["modes"], second["modes"]) and np.array_equal(one["air"]["state"], second["air"]["state"])
    assert np.array_equal(state1, state2)
    # (the cut does carry something, and the steps are numbered through)
    assert first["comfort"]["n_occupied"].any() and not np.array_equal(first["comfort"]["n_occupied"], second["comfort"]["n_occupied"])
    assert (second["comfort"]["step_max"] >= cut).any() and (second["comfort"]["step_max"] < cut).any()


# ---- 4. NULL and inert terms ----
def test_no_comfort_and_sensors_without_a_control_bit_change_no_other_bit():
    md, st = CASE_MODELS["ragged_mixed_28"]()
    rng = np.random.default_rng(523)
    n_sub = 2
    c = cc.comfort_case(md, st, rng)
    probes = probes_of_every_kind(md, rng)
    w = weather_of(md, n_sub)
    others = ("trace", "applied", "modes", "transmitted", "ap_sum", "sunlit")

    def same_others(a, b, what):
        for key in others:
            assert cc.same_bits(a[key], b[key]), (what, key)
        for key in ("path_q",) + cc.AIR_ACC:
            assert cc.same_bits(a["air"][key], b["air"][key]), (what, key)
        for key in a["blinds"]:
            assert cc.same_bits(a["blinds"][key], b["blinds"][key]), (what, key)

    (plain,), state0 = run_series(md, st, {}, [(w, n_sub, cc.series_kwargs(c, probes, comfort=None))])           # the positional entry point
    assert "comfort" not in plain
    (call,), state_call = run_series(md, st, {}, [(w, n_sub, cc.series_kwargs(c, probes, comfort=None, aniso={}))])   # heat_batch_march_series_call
    same_others(plain, call, "series_call")
    inert = dict(c.comfort, control=np.zeros(cc.N_SENSORS, np.uint8))
    for what, sensors in (("no sensor", {}), ("no control bit", inert), ("control NULL", {k: v for k, v in c.comfort.items() if k != "control"})):
        (got,), state = run_series(md, st, {}, [(w, n_sub, cc.series_kwargs(c, probes, comfort=sensors))])
        same_others(plain, got, what)
        assert np.array_equal(state0, state), what
        assert got["comfort"]["operative"].shape == (N_STEPS, cf.n_sensors(sensors))
    # ... the inert sensors still report: the operative temperatures of the state the plain series went through
    assert np.all(np.isfinite(got["comfort"]["operative"])) and got["comfort"]["n_occupied"].any() and not cc.same_bits(got["comfort"]["operative"][0], got["comfort"]["operative"][-1])
    # sensors WITH control bits do change the others (the case discriminates)
    (full,), state_full = run_series(md, st, {}, [(w, n_sub, cc.series_kwargs(c, probes))])
    assert not cc.same_bits(plain["applied"], full["applied"]) or not cc.same_bits(plain["air"]["path_q"], full["air"]["path_q"])
    assert cc.same_bits(got["comfort"]["operative"][0], full["comfort"]["operative"][0])                 # (step 0: the uploaded state)
    # rows and accumulators not asked for change no bit of the others
    (bare,), state_bare = run_series(md, st, {}, [(w, n_sub, cc.series_kwargs(c, probes, comfort=dict(c.comfort, stats=()), operative=False, mrt=False))])
    same_others(full, bare, "nothing asked for")
    assert np.array_equal(state_full, state_bare) and bare["comfort"]["operative"].shape == (0, cc.N_SENSORS) and set(bare["comfort"]) == {"operative", "mrt"}
    (some,), _ = run_series(md, st, {}, [(w, n_sub, cc.series_kwargs(c, probes, comfort=dict(c.comfort, stats=("max_above", "n_below")), mrt=False))])
    assert cc.same_bits(some["comfort"]["operative"], full["comfort"]["operative"]) and cc.same_bits(some["comfort"]["max_above"], full["comfort"]["max_above"])
    assert np.array_equal(some["comfort"]["n_below"], full["comfort"]["n_below"]) and some["comfort"]["mrt"].size == 0
    # c == NULL through the new entry point: heat_batch_march_series_call, and the two arrays of rows are not written
    null = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(null)
        kw = cc.series_kwargs(c, probes, comfort=None)
        s, keep = binding.make_series(w, n_sub, channel=kw["channel"], probes=probes)
        trace, failed = np.zeros((N_STEPS, len(probes))), C.c_int32(5)
        top, mrt = np.full((N_STEPS, 3), 7.0), np.full((N_STEPS, 3), 8.0)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        struct = binding.SeriesCall(size=C.sizeof(binding.SeriesCall), s=C.pointer(s), trace=dp(trace), failed_step=C.pointer(failed))
        assert b._L.heat_batch_march_series_comfort(b._h, C.byref(struct), None, dp(top), dp(mrt)) == 0
        b.download_state(null)
        again = st.copy()
        b.upload_state(again)
        t2 = np.zeros_like(trace)
        struct.trace = dp(t2)
        assert b._L.heat_batch_march_series_call(b._h, C.byref(struct)) == 0
        b.download_state(again)
    assert failed.value == -1 and np.all(top == 7.0) and np.all(mrt == 8.0) and cc.same_bits(trace, t2) and np.array_equal(null, again)
    assert np.all(np.isfinite(trace)) and not cc.same_bits(trace[0], trace[-1])


# ---- 5. n_sub == 0 ----
def test_no_sub_timestep_still_evaluates_every_step_on_the_unchanged_state():
    md, st = CASE_MODELS["ragged_mixed"]()
    st = st.copy()
    rng = np.random.default_rng(520)
    st[mdl.node_slots(md)] += rng.uniform(-2.0, 2.0, len(mdl.node_slots(md)))             # (faces that are not the air)
    st[md["zone_slot"]] += rng.uniform(-1.0, 1.0, int(md["n_zones"]))
    own = owned_slots(md)
    for n_sensors in (cc.N_SENSORS, 1):
        c = cc.comfort_case(md, st, np.random.default_rng(521), n_sensors=n_sensors)
        probes = probes_of_every_kind(md, np.random.default_rng(522))
        ref = cc.loop(c, st.copy(), lambda state, k, za, zb: None, probes)                   # (nothing marches: the state stays)
        got_state = st.copy()
        with HeatBatch(md) as b:
            b.upload_state(got_state)
            got = cc.named(b.march_series(None, 0, n_steps=N_STEPS, **cc.series_kwargs(c, probes)))
            b.download_state(got_state)
        cc.same_as_loop(ref, got, "n_sub=0, %d sensors: " % n_sensors)
        assert np.array_equal(got_state[own], st[own])
        top = got["comfort"]["operative"]
        assert top.shape == (N_STEPS, n_sensors) and np.all(top == top[0]) and np.array_equal(got["trace"], np.tile(st[probes], (N_STEPS, 1)))
        assert got["comfort"]["n_occupied"].any() and (got["comfort"]["n_occupied"] < N_STEPS).any() == (n_sensors > 1)
        assert np.all(got["comfort"]["step_min"][got["comfort"]["n_occupied"] > 0] >= 0)


# ---- 6. all terms together ----
def test_every_term_with_comfort_in_one_call_equals_the_call_cut_in_two():
    import ambient_cases as ac
    from test_series_all_terms_gpu import accumulators_of, everything, rows_of, same
    name, cut = "ragged_mixed-planned", 2
    c, kwargs = ac.case(name), everything(name, True)
    md, n_steps = c.md, c.n_steps
    rng = np.random.default_rng(607)
    base = kwargs()
    NS, nc, Z = len(base["shades"]["surface"]), base["channel"].shape[1], int(md["n_zones"])
    shade = rng.permutation(NS)[:40].astype(np.int32)
    t_mid = float(np.median(c.state[md["zone_slot"]]))
    blinds = dict(shade=shade, beam_closed=rng.uniform(0.05, 0.5, 40), diffuse_closed=rng.uniform(0.2, 0.6, 40), ground_closed=rng.uniform(0.2, 0.6, 40),
                  irr_close=rng.uniform(20.0, 200.0, 40), irr_open=rng.uniform(0.0, 20.0, 40), zone=np.where(np.arange(40) % 2 == 0, rng.integers(0, Z, 40), -1).astype(np.int32),
                  set_chan=np.where(np.arange(40) % 2 == 0, nc - 2, -1).astype(np.int32), band=rng.uniform(0.0, 0.5, 40))
    coef = rng.uniform(0.0, 0.4, (n_steps, 1, 2))
    aniso = dict(shade_band=rng.uniform(0.0, 0.3, NS), front_band=rng.uniform(0.0, 0.3, int(md["n_surfaces"])))
    sensors = cf.by_area(md, air_weight=0.1, control=True)
    sensors = dict(sensors, lo_chan=np.full(Z, nc - 2, np.int32), hi_chan=np.full(Z, nc - 1, np.int32))       # (the ideal loads' setpoints as the band)
    assert abs(base["channel"][0, nc - 2] - (t_mid + 0.7)) < 1e-12

    def widened(steps=slice(None), carried=None):
        kw = kwargs(steps, carried)
        kw.update(blinds=blinds, aniso=dict(aniso, coef=coef[steps]), comfort=sensors)
        if carried is not None:
            kw["blinds"] = dict(blinds, **{k: carried["blinds"][k] for k in ("state", "steps_closed", "switches", "sum_position")})
            kw["comfort"] = dict(sensors, resume={k: carried["comfort"][k] for k in cf.ACC}, step_base=steps.start)
        return kw

    def run(calls):
        state, outs = c.state.copy(), []
        with HeatBatch(md, **c.opts) as b:
            b.upload_state(state)
            for call in calls:
                w, kw = call(outs[-1] if outs else None)
                outs.append(b.march_series(w, c.n_sub, **kw))
                assert isinstance(outs[-1], dict) and outs[-1]["failed_step"] == -1
            b.download_state(state)
        return outs, state

    (one,), state1 = run([lambda _: (c.weather, widened())])
    (first, second), state2 = run([lambda _: (c.weather[:cut], widened(slice(0, cut))),
                                   lambda before: (c.weather[cut:], widened(slice(cut, None), before))])
    r1, ra, rb = rows_of(one), rows_of(first), rows_of(second)
    for k, v in r1.items():
        assert same(v, np.concatenate([ra[k], rb[k]])), k
    for k in ("operative", "mrt"):
        assert same(one["comfort"][k], np.concatenate([first["comfort"][k], second["comfort"][k]])) and one["comfort"][k].shape == (n_steps, Z), k
    for k in ("position", "incident"):
        assert same(one["blinds"][k], np.concatenate([first["blinds"][k], second["blinds"][k]])), k
    a1, a2 = accumulators_of(one), accumulators_of(second)
    for k, v in a1.items():
        assert same(v, a2[k]), k
    for k in cf.ACC:
        assert same(one["comfort"][k], second["comfort"][k]), k
    for k in ("state", "steps_closed", "switches", "sum_position"):
        assert same(one["blinds"][k], second["blinds"][k]), k
    own = owned_slots(md)
    assert same(state1[own], state2[own]) and not same(state1[own], c.state[own])
    # the comfort term acts in this company: operative temperatures that move, sensors outside their band, and controls that
    # sense them — the run differs from the same call with sensors that control nothing
    top = one["comfort"]["operative"]
    assert np.all(np.isfinite(top)) and not same(top[0], top[-1]) and (one["comfort"]["n_below"] + one["comfort"]["n_above"]).any()
    (inert,), _ = run([lambda _: (c.weather, dict(widened(), comfort=dict(sensors, control=np.zeros(Z, np.uint8))))])
    moved = [k for k in ("applied", "ideal_q", "trace") if not same(inert[k], one[k])] + [k for k in ("path_q",) if not same(inert["air"][k], one["air"][k])]
    print("sensing the operative temperature moves %s" % moved)
    assert same(inert["comfort"]["operative"][0], top[0]) and moved


# ---- 7. refusals through the batch ----
def test_bad_comfort_terms_and_sharded_batches_are_refused_by_the_march():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    S = int(md["n_surfaces"])
    n_steps, n_sub = 3, 1
    w = np.zeros((n_steps, n_sub, 3))
    channel = np.full((n_steps, 2), 10.0)
    good = dict(zone=np.array([3, 0, 3, 7]), air_weight=np.array([0.5, 0.0, 1.0, 0.25]), control=np.array([1, 1, 0, 0], np.uint8),
                en_sensor=np.array([0, 2, 1, 0, 3]), en_surface=np.array([5, 17, 199, 0, 64]), en_side=np.array([0, 1, 1, 0, 1], np.uint8),
                en_weight=np.array([0.5, 1.0, 1.0, 0.5, 1.0]), occ_chan=np.array([-1, 0, -1, 1]), lo_chan=np.array([0, -1, 1, -1]), hi_chan=np.array([1, 1, -1, -1]))
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        for damage, code, who in ((dict(zone=np.array([3, 0, 8, 7])), -4, "comfort sensor 2:"), (dict(control=np.array([1, 1, 1, 0], np.uint8)), -4, "comfort sensor 2:"),
                                  (dict(hi_chan=np.array([1, 2, -1, -1])), -4, "comfort sensor 1:"), (dict(occ_chan=np.array([-1, 0, -1, -2])), -4, "comfort sensor 3:"),
                                  (dict(en_sensor=np.array([0, 2, 1, 4, 3])), -4, "comfort entry 3:"), (dict(en_surface=np.array([5, 17, S, 0, 64])), -4, "comfort entry 2:"),
                                  (dict(en_side=np.array([0, 1, 1, 0, 2], np.uint8)), -4, "comfort entry 4:"),
                                  (dict(en_weight=np.array([0.5, np.nan, 1.0, 0.5, 1.0])), -1, "comfort entry 1:"),
                                  (dict(air_weight=np.array([0.5, 0.0, 1.5, 0.25])), -1, "comfort sensor 2:"),
                                  (dict(air_weight=np.array([np.inf, 0.0, 1.0, 0.25])), -1, "comfort sensor 0:"),
                                  (dict(control=np.array([1, 2, 0, 0], np.uint8)), -1, "comfort sensor 1:"),
                                  (dict(stats=("step_max",)), -1, "comfort sensor"), (dict(stats=("step_max_above", "max_operative")), -1, "comfort sensor")):
            with pytest.raises(HeatError) as e:
                b.march_series(w, n_sub, channel=channel, comfort=dict(good, **damage))
            assert e.value.code == code and who in str(e.value), (damage, str(e.value))
        # refused before any device work: every slot the batch owns is what was uploaded, to the bit
        own = owned_slots(md)
        behind = st.copy()
        behind[own] = np.nan
        b.download_state(behind)
        assert np.array_equal(behind[own], st[own])
        # ... and the batch marches a good term afterwards, one sensor alone too
        trace, failed, out = b.march_series(w, n_sub, probes=md["zone_slot"], channel=channel, comfort=good)
        assert failed == -1 and np.all(np.isfinite(trace)) and out["operative"].shape == (n_steps, 4) and np.all(np.isfinite(out["operative"]))
        assert out["mrt"].shape == (n_steps, 4) and list(out["n_occupied"]) == [3, 3, 3, 3] and np.all(out["step_min"] >= 0)
        b.download_state(behind)
        assert not np.array_equal(behind[own], st[own])                      # (a series that runs does move them)
        one = dict(zone=[5], en_sensor=[0, 0], en_surface=[9, 9], en_side=[0, 1], en_weight=[0.5, 0.5], control=[1])
        state = behind.copy()
        r, top = cf.operative(state[cf.face_slots(md, one)], state[md["zone_slot"]], one)
        trace, failed, out = b.march_series(w[:1], n_sub, probes=md["zone_slot"], channel=channel[:1], comfort=one)
        assert failed == -1 and out["operative"].shape == (1, 1) and out["operative"][0, 0] == top[0] and out["mrt"][0, 0] == r[0]
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, n_sub, channel=channel, comfort=good)
        assert e.value.code == -1 and "sharded" in str(e.value)
