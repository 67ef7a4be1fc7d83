"""Air species of a series on the GPU (include/heat_amd.h, heat_batch_march_series_species): concentrations per species and
zone carried by every flow of air of a series, and demand vents that follow them, stepped on the device.

The expected result is DEFINED by air_species_cases.loop_with_rules — the zone loads' rule, then heat_amd.air_paths.apply,
heat_amd.air_handlers.apply and heat_amd.air_species.apply (the header's contract in numpy, one rounded operation per line),
applied between per-step march calls to the zone temperatures the call before returned: through heat_batch_march_ex the series
must agree bit for bit, through OracleModel.march (≙ ThermalModel::march, src/model.rs:359-427) at rtol = atol = 1e-9, the
project's parity bound, with the discrete outputs equal. tests/test_air_species_host.py runs the same cases through the oracle
alone and asserts that paths open and close, vents saturate and release and a limit is crossed. The rule is this project's own:
the reference has no counterpart (zone.rs, model.rs:500-597); the air properties are the reference's (gas.rs:49,165-179).

Two species in 20 zones are 40 lanes, less than a wavefront; in 500 zones 1000 lanes: four workgroups of 256 with a ragged last
wavefront (1000 = 15 * 64 + 40), the paths' sources reaching into the lanes of other workgroups."""
import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, air_handlers as ah, air_paths, air_species as asp, binding, comfort as cf, modeldict as mdl
import air_handlers_cases as ahc
import air_species_cases as asc
import comfort_cases as cc
from air_handlers_cases import handlers_with
from test_series_gpu import MODELS, assert_close, owned_slots, probes_of_every_kind, series_kwargs, zone_terms, _id

pytestmark = pytest.mark.gpu

OPTIONS = [dict(), dict(use_graph=True), dict(no_fusion=True)]
SMALL_MODELS = ["ragged_mixed", "rooms_with_windows"]
LARGE = "rooms_with_windows_large"
N_STEPS = asc.N_STEPS


def kwargs(c, steps=slice(None)):
    return series_kwargs(c["channel"], c["drives"], c["probes"], c["a0"], c["b0"], steps=steps)


def named(c, out):
    names = (["trace", "failed_step"] + (["applied", "modes"] if c["loads"] else []) + (["air"] if c["air"] else []) +
             (["handlers"] if c["handlers"] else []) + ["species"])
    assert len(out) == len(names)
    return dict(zip(names, out))


def series(c, opts, species="case", steps=slice(None), state=None, carry=None, step_base=0, **more):
    """One series with the case's loads, air paths, handlers and `species` on a fresh batch, resumed from `carry` (a loop's, or
    carried() of a series). Returns (the named result, the final state)."""
    got = c["st"].copy() if state is None else state.copy()
    species = c["species"] if isinstance(species, str) else species
    loads, air, handlers = c["loads"], c["air"], c["handlers"]
    if carry:
        loads = dict(loads, thermostats=dict(loads["thermostats"], mode=carry["modes"])) if loads else None
        air = dict(air, **{k: carry["air"][k] for k in asc.AIR_ACC}) if air else None
        handlers = handlers_with(handlers, carry["handlers"]) if handlers else None
        species = asc.species_with(species, carry["species"], step_base)
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(got)
        out = named(c, b.march_series(c["w"][steps], c["n_sub"], loads=loads, air=air, handlers=handlers, species=species,
                                      **dict(kwargs(c, steps), **more)))
        b.download_state(got)
    assert out["failed_step"] == -1
    return out, got


def carried(got):
    return dict(modes=got["modes"], air={k: got["air"][k] for k in asc.AIR_ACC},
                handlers={k: v for k, v in got["handlers"].items() if v.ndim == 1}, species={k: got["species"][k] for k in ("conc",) + asp.ACC})


def same(ref, got, what, close=None):
    """A loop's result against a series': the discrete outputs exactly; the rows and sums bit for bit, or through close."""
    def value(r, g, name):
        if close is None:
            assert np.array_equal(r, g, equal_nan=True), "%s %s: %d differ, worst %.3e" % (what, name, int((r != g).sum()), np.nanmax(np.abs(r - g)))
        else:
            close(r, g, "%s %s" % (what, name))

    acc = ref["carry"]["species"]
    for key in asc.DISCRETE:
        assert np.array_equal(acc[key], got["species"][key]), "%s %s: %d differ" % (what, key, int((acc[key] != got["species"][key]).sum()))
    if "modes" in got:
        assert np.array_equal(ref["carry"]["modes"], got["modes"]), what
        value(ref["applied"], got["applied"], "applied")
    if "air" in got:
        for key in ("state", "steps_open", "switches"):
            assert np.array_equal(ref["carry"]["air"][key], got["air"][key]), "%s air %s" % (what, key)
        value(ref["path_q"], got["air"]["path_q"], "path_q")
    if "handlers" in got:
        value(ref["branch_q"], got["handlers"]["branch_q"], "branch_q")
    for key in asp.ROWS:
        value(ref[key], got["species"][key], key)
    for key in asc.REAL:
        value(acc[key], got["species"][key], key)
    value(ref["trace"], got["trace"], "trace")


# ---- 1. bit for bit against the per-call loop ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", [(m, n) for m in SMALL_MODELS for n in (2, 5)] + [(LARGE, 2)])
def test_series_with_air_species_equals_the_per_call_path_bit_for_bit(model, n_sub, opts):
    c = asc.case(model, N_STEPS, n_sub, 2, asc.SEED)
    lanes = asc.N_SPECIES * int(c["md"]["n_zones"])
    assert lanes < 64 or model != "ragged_mixed"
    assert (lanes > 256 and lanes % 64 != 0) or model != LARGE
    own = owned_slots(c["md"])
    ref_state = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(ref_state)
        ref = asc.loop_with_rules(lambda s, wk, za, zb: b.march(s, wk, za, zb, outputs=b.OUT_ALL), c, ref_state)
    # the inputs exercise the vents and the paths (tests/test_air_species_host.py asserts it of the oracle loop alone)
    asc.assert_coverage(asc.coverage(c, ref), "%s n_sub=%d (per-call path)" % (model, n_sub))
    got, state = series(c, opts)
    same(ref, got, model)
    assert np.array_equal(ref_state[own], state[own]), "%d state slots differ" % int((ref_state[own] != state[own]).sum())


# ---- 2. the oracle loop ----
_ORACLE_LOOPS = {}


def oracle_loop(oracle, model, n_sub):
    c = asc.case(model, N_STEPS, n_sub, 2, asc.SEED)
    if (model, n_sub) not in _ORACLE_LOOPS:  # (the same for every option set; left unchanged)
        big = c["md"]["n_surfaces"] > 8192
        m = oracle.OracleModel(c["md"])

        def march(s, wk, za, zb):
            assert m.march(s, wk, za, zb, threads=16 if big else 1)[0] == 0

        state = c["st"].copy()
        _ORACLE_LOOPS[(model, n_sub)] = (asc.loop_with_rules(march, c, state), state)
    return (c,) + _ORACLE_LOOPS[(model, n_sub)]


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", [("ragged_mixed", 2), ("ragged_mixed", 5), ("rooms_with_windows", 2), ("rooms_with_windows", 5), (LARGE, 5)])
def test_series_with_air_species_matches_the_oracle_loop(oracle, model, n_sub, opts):
    c, ref, ref_state = oracle_loop(oracle, model, n_sub)
    asc.assert_coverage(asc.coverage(c, ref), "%s n_sub=%d (oracle loop)" % (model, n_sub))
    got, state = series(c, opts)
    same(ref, got, model, close=assert_close)
    own = owned_slots(c["md"])
    assert_close(ref_state[own], state[own], "%s final state" % model)


# ---- 3. cut ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("cut", [7, 16])
def test_series_with_air_species_cut_in_two_equals_the_series_in_one(cut, opts):
    c = asc.case("rooms_with_windows", N_STEPS, 2, 2, asc.SEED)
    one, state1 = series(c, opts)
    first, mid = series(c, opts, steps=slice(0, cut))
    second, state2 = series(c, opts, steps=slice(cut, None), state=mid, carry=carried(first), step_base=cut)
    assert first["species"]["steps_saturated"].any() and first["species"]["n_above"].any() and first["air"]["state"].any()
    assert (one["species"]["step_max"] >= cut).any() and (one["species"]["step_max"] < cut).any()
    assert np.array_equal(one["trace"], np.concatenate([first["trace"], second["trace"]]))
    for key in asp.ROWS:
        assert np.array_equal(one["species"][key], np.concatenate([first["species"][key], second["species"][key]])), key
    for key in ("conc",) + asp.ACC:
        assert np.array_equal(one["species"][key], second["species"][key]), key
    assert np.array_equal(one["modes"], second["modes"]) and np.array_equal(one["air"]["state"], second["air"]["state"])
    assert np.array_equal(state1, state2)


# ---- 4. every concentration is read as it was at the start of the step ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_a_path_carries_the_concentration_its_source_had_at_the_start_of_the_step(opts):
    c = asc.case("rooms_with_windows", N_STEPS, 2, 2, asc.SEED, with_loads=False, with_air=False, with_handlers=False)
    Z, vol = int(c["md"]["n_zones"]), c["md"]["zone_volume"]
    A, B, D = 50, 3, 51                                               # a chain A -> B -> D: B's lane runs before A's and D's
    vc = c["channel"].shape[1]
    c["channel"] = np.concatenate([c["channel"], np.full((N_STEPS, 1), 0.5)], axis=1)
    c["air"] = dict(target=[B, D], source=[A, B], volume_chan=[vc, vc])
    conc = np.zeros((1, Z))
    conc[0, A] = 1000.0
    species = dict(outdoor_chan=asp.per_zone([-1], Z), conc=conc)
    got, _ = series(c, opts, species=species)
    rows = got["species"]["conc_rows"][:, 0, :]
    h = 2.0 * c["md"]["dt"]
    assert np.array_equal(rows[0], conc[0]) and np.array_equal(rows[:, A], np.full(N_STEPS, 1000.0))
    assert rows[1, B] == (vol[B] * 0.0 + h * (0.0 + 0.5 * 1000.0)) / (vol[B] + h * 0.5)
    assert rows[1, D] == 0.0 and rows[2, D] == (vol[D] * 0.0 + h * (0.0 + 0.5 * rows[1, B])) / (vol[D] + h * 0.5)   # not within a step
    want = np.zeros((N_STEPS, Z))
    C = conc.copy()
    for k in range(N_STEPS):
        want[k] = asp.apply(np.zeros(Z), C, c["channel"][k], None, None, species, vol, h, air=c["air"], air_state=np.zeros(2, np.uint8))[2]["conc"][0]
    assert np.array_equal(want, rows) and np.array_equal(C, got["species"]["conc"])


# ---- 5. with ideal loads: they see the vents' terms in every sub-timestep ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", [("rooms_with_windows", 2), ("rooms_with_windows", 5)])
def test_ideal_loads_see_the_demand_vents(model, n_sub, opts):
    c = asc.case(model, N_STEPS, n_sub, 0, asc.SEED, with_loads=False, with_air=False, with_handlers=False)
    md, Z = c["md"], int(c["md"]["n_zones"])
    t_mid = float(np.median(c["st"][md["zone_slot"]]))
    c0 = c["channel"].shape[1]
    channel = np.concatenate([c["channel"], np.tile([t_mid + 0.7, t_mid + 1.7], (N_STEPS, 1))], axis=1)
    zone = np.flatnonzero(np.arange(Z) % 2 == 0).astype(np.int32)
    ideal = dict(zone=zone, heat_chan=np.full(len(zone), c0, np.int32), cool_chan=np.full(len(zone), c0 + 1, np.int32),
                 heat_cap=np.where(np.arange(len(zone)) % 3 == 0, 500.0, np.inf))
    probes = md["zone_slot"].astype(np.int64)
    kw = series_kwargs(channel, c["drives"], probes)
    first, second = c["st"].copy(), c["st"].copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(first)
        out1 = b.march_series(c["w"], n_sub, ideal=ideal, species=c["species"], **kw)
        b.download_state(first)
    assert out1["failed_step"] == -1 and (out1["ideal_q"] > 0).any() and (out1["ideal_q"] < 0).any()
    # the terms the vents formed, from the first run's zone trace; the concentrations replayed on the way
    start = np.concatenate([c["st"][md["zone_slot"]][None, :], out1["trace"][:-1]])
    C = np.array(c["species"]["conc"])
    rule = asc.rule_args(c["species"])
    rows = [asp.apply(start[k], C, channel[k], None, None, rule, md["zone_volume"], float(n_sub) * md["dt"]) for k in range(N_STEPS)]
    assert np.array_equal(np.array([r[2]["vent_v"] for r in rows]), out1["species"]["vent_v"])
    assert np.array_equal(np.array([r[2]["vent_q"] for r in rows]), out1["species"]["vent_q"]) and out1["species"]["vent_q"].any()
    assert np.array_equal(C, out1["species"]["conc"])
    with HeatBatch(md, **opts) as b:
        b.upload_state(second)
        out2 = b.march_series(c["w"], n_sub, ideal=ideal, zone_a0=np.array([r[0] for r in rows]), zone_b0=np.array([r[1] for r in rows]), **kw)
        b.download_state(second)
    assert np.array_equal(out1["trace"], out2["trace"]) and np.array_equal(out1["ideal_q"], out2["ideal_q"])
    assert np.array_equal(first, second)
    for key in out1["ideal"]:
        assert np.array_equal(out1["ideal"][key], out2["ideal"][key]), key


# ---- 6. beside comfort control sensors, blinds, air paths, zone loads and handlers ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("n_sub", [2, 5])
def test_air_species_beside_every_other_term_equal_the_per_call_loop_bit_for_bit(n_sub, opts):
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(asc.SEED + n_sub)
    c = cc.comfort_case(md, st, rng)
    c.channel, handlers, _ = ahc.random_handlers(md, np.asarray(st), rng, c.n_steps, c.channel)
    c.channel, species, _ = asc.random_species(md, np.asarray(st), rng, c.n_steps, n_sub, c.channel)
    rule = asc.rule_args(species)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, c.n_steps, 2)
    w = mdl.weather_series(c.n_steps * n_sub, md["dt"]).reshape(c.n_steps, n_sub, 3)
    h_acc, acc, rows = ah.fresh(handlers), asp.fresh(rule, int(md["n_zones"]), species["conc"]), []
    path_state = np.zeros(air_paths.n_paths(c.air), np.uint8)

    def with_species(march):
        # comfort_cases.loop hands over the zone terms behind the loads' and the paths' rules; the inputs it has written by then
        # are neither zone nor face temperatures: the state still holds those of the start of the step. The paths' state bytes
        # stay inside that loop, so the step replays the paths' rule on a copy of its own, sensing what the loop senses.
        def step(state, k, za, zb):
            T = state[md["zone_slot"]].copy()
            _, top = cf.operative(state[c.face], T, c.comfort)
            air_paths.apply(T, c.channel[k], None, None, c.air, path_state, control_T=cf.control_temperatures(T, top, c.comfort))
            za, zb, r = ah.apply(T, c.channel[k], za, zb, handlers, h_acc["bypass"])
            ah.accumulate(r, h_acc)
            za, zb, r = asp.apply(T, acc["conc"], c.channel[k], za, zb, rule, md["zone_volume"], float(n_sub) * md["dt"], loads=c.loads, air=c.air,
                                  air_state=path_state, handlers=handlers)
            asp.accumulate(r, acc, rule, c.channel[k], k)
            rows.append(r)
            march(state, k, za, zb)
        return step

    want = st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(want)
        ref = cc.loop(c, want, with_species(cc.marcher(b, w)), probes, a0, b0)
    assert np.array_equal(path_state, ref["carry"]["air"]["state"]) and path_state.any()
    state = st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(state)
        out = b.march_series(w, n_sub, **cc.series_kwargs(c, probes, a0, b0, handlers=handlers, species=species))
        b.download_state(state)
    got = dict(zip(cc.NAMES + ("handlers", "species"), out))
    assert len(out) == len(cc.NAMES) + 2
    cc.same_as_loop(ref, got, "n_sub=%d: " % n_sub)
    assert np.array_equal(np.array([r["conc"] for r in rows]), got["species"]["conc_rows"])
    assert np.array_equal(np.array([r["vent_v"] for r in rows]), got["species"]["vent_v"])
    assert np.array_equal(np.array([r["vent_q"] for r in rows]), got["species"]["vent_q"])
    for key in ("conc",) + asp.ACC:
        assert np.array_equal(acc[key], got["species"][key]), key
    for key in ("bypass",) + ah.ACC:
        assert np.array_equal(h_acc[key], got["handlers"][key]), key
    own = owned_slots(md)
    assert np.array_equal(want[own], state[own])
    assert acc["steps_saturated"].any() and acc["n_above"].any()


# ---- 7. NULL cases ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_no_air_species_is_the_series_without_them_bit_for_bit(opts):
    c = asc.case("rooms_with_windows", 12, 3, 2, 5)
    C = binding.C
    results = []
    for how in ("plain", "empty", "null"):
        state = c["st"].copy()
        with HeatBatch(c["md"], **opts) as b:
            b.upload_state(state)
            if how == "plain":
                trace, failed, applied, modes, air, hd = b.march_series(c["w"], 3, loads=c["loads"], air=c["air"], handlers=c["handlers"], **kwargs(c))
            elif how == "empty":
                trace, failed, applied, modes, air, hd, sp = b.march_series(c["w"], 3, loads=c["loads"], air=c["air"], handlers=c["handlers"],
                                                                            species={}, **kwargs(c))
                assert sp["conc_rows"].shape == (12, 0, 0) and sp["vent_v"].shape == (12, 0) and sp["conc"].size == 0
            else:  # sp == NULL through the C ABI
                s, keep = binding.make_series(c["w"], 3, **kwargs(c))
                l, lkeep = binding.make_zone_loads(**c["loads"])
                a, akeep = binding.make_air_paths(**c["air"])
                h, hkeep = binding.make_air_handlers(**c["handlers"])
                trace, applied, f = np.zeros((12, len(c["probes"]))), np.zeros((12, l.n_thermostats)), C.c_int32(7)
                path_q, branch_q = np.zeros((12, a.n_paths)), np.zeros((12, h.n_branches))
                call = binding.SeriesCall(size=C.sizeof(binding.SeriesCall), s=C.pointer(s), l=C.pointer(l), air=C.pointer(a), failed_step=C.pointer(f),
                                          trace=trace.ctypes.data_as(binding._dp), applied=applied.ctypes.data_as(binding._dp),
                                          path_q=path_q.ctypes.data_as(binding._dp))
                assert b._L.heat_batch_march_series_species(b._h, C.byref(call), None, None, None, C.byref(h), None, None, None,
                                                            branch_q.ctypes.data_as(binding._dp), None, None, None, None) == 0
                failed, modes = f.value, lkeep["th_mode"]
                air = dict(path_q=path_q, **{k: akeep[k] for k in asc.AIR_ACC})
                hd = dict(branch_q=branch_q, bypass=hkeep["bypass"], sum_recovered=hkeep["sum_recovered"])
            b.download_state(state)
        assert failed == -1
        results.append((trace, applied, modes, state, hd["branch_q"], hd["bypass"], hd["sum_recovered"]) + tuple(air[k] for k in ("path_q",) + asc.AIR_ACC))
    for other in results[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(results[0], other))


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_an_array_that_is_not_asked_for_changes_no_bit_of_the_others(opts):
    c = asc.case("ragged_mixed", N_STEPS, 2, 2, asc.SEED)
    full, state = series(c, opts)
    S, Z, V = asc.N_SPECIES, int(c["md"]["n_zones"]), asp.n_vents(c["species"])
    # (step_max follows max_conc: it is kept where max_conc is)
    for stats, rows in ([((s,), ()) for s in binding.SPECIES_STATS if s != "step_max"] + [(("max_conc", "step_max"), ())] +
                        [((), (r,)) for r in asp.ROWS] + [((), ()), ((), asp.ROWS)]):
        got, st = series(c, opts, species=dict(c["species"], stats=stats), **{r: r in rows for r in asp.ROWS})
        assert set(got["species"]) == set(asp.ROWS) | {"conc"} | set(stats)
        assert got["species"]["conc_rows"].shape == ((N_STEPS if "conc_rows" in rows else 0), S, Z)
        for r in ("vent_v", "vent_q"):
            assert got["species"][r].shape == ((N_STEPS if r in rows else 0), V)
        for key, v in got["species"].items():
            if v.size:
                assert np.array_equal(v, full["species"][key]), (stats, rows, key)
        assert np.array_equal(got["trace"], full["trace"]) and np.array_equal(got["applied"], full["applied"]) and np.array_equal(st, state)
        assert np.array_equal(got["air"]["path_q"], full["air"]["path_q"])
    # no vent, no source, no loads, no paths, no handlers: the concentrations stay where they are, up to the rounding of
    # (vol * c) / vol — one ulp a step at the most
    bare = asc.case("ragged_mixed", 4, 2, 2, asc.SEED, with_loads=False, with_air=False, with_handlers=False)
    conc = np.arange(1.0, 1.0 + S * Z).reshape(S, Z)
    alone = dict(outdoor_chan=asp.per_zone([-1, -1], Z), conc=conc)
    got, _ = series(bare, opts, species=alone)
    C = conc.copy()
    want = np.array([asp.apply(np.zeros(Z), C, bare["channel"][k], None, None, alone, bare["md"]["zone_volume"], 2.0 * bare["md"]["dt"])[2]["conc"]
                     for k in range(4)])
    assert np.array_equal(got["species"]["conc"], C) and np.array_equal(got["species"]["conc_rows"], want)
    assert np.array_equal(want[0], conc) and np.allclose(C, conc, rtol=4 * 2.3e-16, atol=0.0)
    assert got["species"]["vent_v"].shape == (4, 0) and (got["species"]["n_occupied"] == 4).all() and (got["species"]["step_max"] == 0).all()


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_a_plain_series_after_one_with_air_species_is_the_plain_series_of_a_fresh_batch(opts):
    c = asc.case("rooms_with_windows", 12, 2, 2, 9)
    fresh = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(fresh)
        want = b.march_series(c["w"], 2, **kwargs(c))
        b.download_state(fresh)
    after = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(c["st"].copy())
        b.march_series(c["w"], 2, loads=c["loads"], air=c["air"], handlers=c["handlers"], species=c["species"], **kwargs(c))
        b.upload_state(after)
        got = b.march_series(c["w"], 2, **kwargs(c))
        b.download_state(after)
    assert np.array_equal(want[0], got[0]) and want[1] == got[1] == -1 and np.array_equal(fresh, after)


def test_a_series_of_no_sub_timestep_still_evaluates_the_species_with_h_zero():
    c = asc.case("ragged_mixed", 6, 0, 2, 21)
    # nothing marches: every step sees the zone temperatures of the start, and with h = 0 no concentration moves
    ref = asc.loop_with_rules(lambda s, wk, za, zb: None, c, c["st"].copy())
    state = c["st"].copy()
    with HeatBatch(c["md"]) as b:
        b.upload_state(state)
        got = named(c, b.march_series(None, 0, n_steps=6, loads=c["loads"], air=c["air"], handlers=c["handlers"], species=c["species"], **kwargs(c)))
        b.download_state(state)
    assert got["failed_step"] == -1 and np.array_equal(state, c["st"])
    assert (ref["vent_v"] != 0).any() and (ref["vent_q"] != 0).any()
    # (h = 0: c_new = (vol * c + 0) / (vol + 0), the concentration it had up to one ulp)
    assert np.allclose(got["species"]["conc"], c["species"]["conc"], rtol=6 * 2.3e-16, atol=0.0) and np.array_equal(got["species"]["conc_rows"][0], c["species"]["conc"])
    for key in asp.ROWS:
        assert np.array_equal(ref[key], got["species"][key]), key
    for key in asc.DISCRETE + asc.REAL:
        assert np.array_equal(ref["carry"]["species"][key], got["species"][key]), key


# ---- 8. NaN ----
def test_a_nan_concentration_at_a_vent_is_reported_as_the_zone_failure_and_elsewhere_it_is_data():
    """A NaN concentration makes a vent's f, V and m NaN, and with them the zone's a0 and b0; the zone update itself would hide
    that (model.rs:662-668), so the vents report it as the air paths do: HEAT_N_NAN_ZONE, at the step whose row holds the NaN. In
    a zone without a vent the NaN is data: it stays in its rows and fails nothing."""
    md, st = mdl.clustered_massive(700, Z=28, dt=45.0, seed=3)
    Z, n_steps, j = 28, 9, 5
    good = np.tile([400.0, 1.0, 5.0], (n_steps, 1))                  # the outdoor level, a source strength, the outdoor temperature
    channel = good.copy()
    channel[j, 1] = np.nan                                           # the source of zone 13 at step j: its concentration is NaN from j + 1 on
    species = dict(outdoor_chan=asp.per_zone([0], Z), conc=np.full((1, Z), 500.0), src_zone=[13, 7], src_species=[0, 0], src_chan=[1, 1],
                   src_factor=[3.0, 3.0], vent_zone=[13, 2], vent_species=[0, 0], vent_temp_chan=[2, 2], vent_v_min=[0.01, 0.01],
                   vent_v_max=[0.2, 0.2], vent_c_lo=[450.0, 450.0], vent_c_hi=[900.0, 900.0])
    for opts, n_sub in [(o, 2) for o in OPTIONS]:
        w = mdl.weather_series(n_steps * n_sub, 45.0).reshape(n_steps, n_sub, 3)
        with HeatBatch(md, **opts) as b:
            b.upload_state(st.copy())
            with pytest.raises(HeatError) as e:
                b.march_series(w, n_sub, species=species, channel=channel, probes=md["zone_slot"], n_steps=n_steps)
            assert e.value.failed_step == j + 1 and e.value.code == 3, str(e.value)   # HEAT_N_NAN_ZONE
            assert b.failed_surface() == (13, 3) and "zone 13" in str(e.value)
            assert np.all(np.isfinite(e.value.trace[:j + 1]))
            # the process and the batch survive: a healthy series afterwards
            b.upload_state(st.copy())
            trace, failed, got = b.march_series(w, n_sub, species=species, channel=good, probes=md["zone_slot"], n_steps=n_steps)
            assert failed == -1 and np.all(np.isfinite(trace)) and np.all(np.isfinite(got["conc_rows"])) and got["sum_volume"].all()
    # the same NaN in a zone without a vent (7 has a source, no vent) fails nothing and stays in its rows
    no_vent = dict(species, src_zone=[7, 7], vent_zone=[13, 2])
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, got = b.march_series(mdl.weather_series(n_steps * 2, 45.0).reshape(n_steps, 2, 3), 2, species=no_vent, channel=channel,
                                            probes=md["zone_slot"])
    assert failed == -1 and np.all(np.isfinite(trace))
    rows = got["conc_rows"][:, 0, :]
    assert np.isnan(rows[j + 1:, 7]).all() and np.isfinite(rows[:j + 1, 7]).all() and np.isfinite(np.delete(rows, 7, axis=1)).all()
    assert np.isnan(got["conc"][0, 7]) and np.isnan(got["sum_conc"][0, 7]) and np.isfinite(got["vent_v"]).all()


# ---- 9. the closed form, and one physical sanity check ----
def test_one_zone_with_constant_source_flow_and_outdoor_level_follows_the_closed_form():
    """vol dc/dt = S + V (co - c), backward Euler: c_n - c* = (c_0 - c*) (vol / (vol + h V))^n with c* = co + S / V. Held at
    rtol 1e-12: about six rounded operations a step, each 1.1e-16, over 100 steps of a map that contracts."""
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    Z, n_steps, n_sub, z = 8, 100, 1, 5
    S, V, co, c0 = 0.004, 0.03, 410.0, 2000.0
    channel = np.tile([S, V, co, 10.0], (n_steps, 1))
    loads = dict(flows=dict(zone=[z], volume_chan=[1], temp_chan=[3]))
    conc = np.zeros((1, Z))
    conc[0, z] = c0
    species = dict(outdoor_chan=asp.per_zone([2], Z), conc=conc, src_zone=[z], src_species=[0], src_chan=[0], src_factor=[1000.0])
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, applied, modes, got = b.march_series(w, n_sub, loads=loads, species=species, channel=channel, probes=md["zone_slot"])
    assert failed == -1
    vol, h = float(md["zone_volume"][z]), float(n_sub) * float(md["dt"])
    star = co + 1000.0 * S / V
    r = vol / (vol + h * V)
    n = np.arange(n_steps + 1)
    want = star + (c0 - star) * r ** n
    have = np.concatenate([got["conc_rows"][:, 0, z], got["conc"][0, [z]]])
    print("closed form: worst relative deviation %.3e over %d steps" % (np.max(np.abs(have - want) / np.abs(want)), n_steps))
    assert np.allclose(have, want, rtol=1e-12, atol=0.0)
    assert have[-1] < 0.5 * (c0 + star)                              # (it moved: r^100 is small)
    # the other zones: no inflow, no source — they keep what they had
    assert not np.delete(got["conc_rows"][:, 0, :], z, axis=1).any()


def test_a_demand_vent_settles_the_concentration_lower_and_cold_outside_air_cools_the_room():
    md, st = mdl.partitioned_buildings(960, 12, seed=8)
    Z, n_steps, n_sub, room = int(md["n_zones"]), 60, 2, 1
    t0 = float(st[md["zone_slot"]][room])
    # 800 W and a CO2 source in the room (100 units a second: about 30 ppm a step in a room of 300 m3); infiltration of
    # 0.005 m3/s; outside air at t0 - 15 C with 400 ppm
    channel = np.tile([800.0, 0.005, t0 - 15.0, 400.0, 1.0], (n_steps, 1))
    loads = dict(gains=dict(zone=[room], chan=[0]), flows=dict(zone=[room], volume_chan=[1], temp_chan=[2]))
    conc = np.full((1, Z), 400.0)
    base = dict(outdoor_chan=asp.per_zone([3], Z), conc=conc, src_zone=[room], src_species=[0], src_chan=[4], src_factor=[100.0])
    vent = dict(base, vent_zone=[room], vent_species=[0], vent_temp_chan=[2], vent_v_min=[0.0], vent_v_max=[0.1], vent_c_lo=[600.0], vent_c_hi=[1200.0])
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    probes = md["zone_slot"][[room]]
    runs = {}
    with HeatBatch(md) as b:
        for name, species in (("closed", base), ("vented", vent)):
            b.upload_state(st.copy())
            trace, failed, _, _, got = b.march_series(w, n_sub, loads=loads, species=species, channel=channel, probes=probes)
            assert failed == -1
            runs[name] = (trace, got)
    c_closed, c_vented = runs["closed"][1]["conc"][0, room], runs["vented"][1]["conc"][0, room]
    t_closed, t_vented = runs["closed"][0][-1, 0], runs["vented"][0][-1, 0]
    print("after %d steps: %.1f / %.1f ppm and %.3f / %.3f C without / with the demand vent; sum_volume %s m3/s-steps" % (
        n_steps, c_closed, c_vented, t_closed, t_vented, runs["vented"][1]["sum_volume"]))
    assert c_vented < c_closed - 100.0 and t_vented < t_closed - 0.1
    assert runs["vented"][1]["sum_volume"][0] > 0.0 and runs["vented"][1]["sum_q"][0] < 0.0 and np.all(runs["vented"][1]["vent_q"] <= 0.0)
    # until the concentration reaches c_lo the vent stays shut and the two runs are one
    shut = runs["vented"][1]["vent_v"][:, 0] == 0.0
    assert shut[0] and not shut[-1] and np.array_equal(runs["closed"][0][:shut.sum()], runs["vented"][0][:shut.sum()])


# ---- 10. refusals ----
def test_bad_species_and_sharded_batches_are_refused_by_the_march():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    Z = 8
    w, channel = np.zeros((2, 1, 3)), np.zeros((2, 2))
    ok = dict(outdoor_chan=asp.per_zone([0], Z), src_zone=[1], src_species=[0], src_chan=[1], vent_zone=[2], vent_species=[0], vent_temp_chan=[1],
              vent_v_min=[0.0], vent_v_max=[0.1], vent_c_lo=[1.0], vent_c_hi=[2.0])
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        for bad, code, needle in ((dict(ok, src_zone=[8]), -4, "species source 0:"),
                                  (dict(ok, src_species=[1]), -4, "species source 0:"),
                                  (dict(ok, outdoor_chan=asp.per_zone([2], Z)), -4, "air species 0:"),
                                  (dict(ok, vent_zone=[-1]), -4, "demand vent 0:"),
                                  (dict(ok, vent_temp_chan=[2]), -4, "demand vent 0:"),
                                  (dict(ok, vent_v_min=[-0.1]), -1, "demand vent 0:"),
                                  (dict(ok, vent_v_max=[np.inf]), -1, "demand vent 0:"),
                                  (dict(ok, vent_c_hi=[1.0]), -1, "demand vent 0:"),
                                  (dict(ok, src_factor=[np.nan]), -1, "species source 0:")):
            with pytest.raises(HeatError) as e:
                b.march_series(w, 1, channel=channel, species=bad)
            assert e.value.code == code and needle in str(e.value), str(e.value)
        got = st.copy()
        b.download_state(got)
        assert np.array_equal(got, st)
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, 1, channel=channel, species=ok)
        assert e.value.code == -1 and "sharded" in str(e.value)
