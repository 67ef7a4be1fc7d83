"""Air handlers of a series on the GPU (include/heat_amd.h, heat_batch_march_series_handlers): ventilation units with heat
recovery, a summer bypass and supply-air coils, formed on the device at every step of a series from the zone air temperatures
it holds.

The expected result is DEFINED by air_handlers_cases.loop_with_rules — the zone loads' rule, then heat_amd.air_paths.apply, then
heat_amd.air_handlers.apply (the header's contract in numpy, one rounded operation per line), applied between per-step march
calls to the zone temperatures the call before returned: through heat_batch_march_ex the series must agree bit for bit, through
OracleModel.march (≙ ThermalModel::march, src/model.rs:359-427) at rtol = atol = 1e-9, the project's parity bound, with the
discrete outputs equal. tests/test_air_handlers_host.py runs the same cases through the oracle alone and asserts that the
bypass and the coils move. The rule is this project's own: the reference has no plant (heating_cooling.rs is a todo!(),
model.rs:522-544 knows scheduled flows only); the air properties are the reference's (gas.rs:49,165-179).

5 units are less than a wavefront; 300 units are two workgroups of 256 lanes with a ragged tail, their branches reaching into
zones of the other one."""
import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, air_handlers as ah, binding, modeldict as mdl
import air_handlers_cases as ahc
import comfort_cases as cc
from test_series_gpu import MODELS, assert_close, owned_slots, probes_of_every_kind, series_kwargs, zone_terms, _id

pytestmark = pytest.mark.gpu

OPTIONS = [dict(), dict(use_graph=True), dict(no_fusion=True)]
ALL_MODELS = ["ragged_mixed", "rooms_with_windows", "partitioned_buildings_large", "rooms_with_windows_large"]
N_STEPS = ahc.N_STEPS
DISCRETE = ("bypass", "steps_bypass", "switches", "steps_heat_saturated", "steps_cool_saturated")
REAL = ("sum_recovered", "sum_heating", "sum_cooling", "sum_branch_q")


def kwargs(c, steps=slice(None)):
    return series_kwargs(c["channel"], c["drives"], c["probes"], c["a0"], c["b0"], steps=steps)


def named(c, out):
    names = ["trace", "failed_step"] + (["applied", "modes"] if c["loads"] else []) + (["air"] if c["air"] else []) + ["handlers"]
    assert len(out) == len(names)
    return dict(zip(names, out))


def series(c, opts, handlers="case", steps=slice(None), state=None, carry=None, **more):
    """One series with the case's loads, air paths and `handlers` on a fresh batch, resumed from `carry` (a loop's, or
    carried() of a series). Returns (the named result, the final state)."""
    got = c["st"].copy() if state is None else state.copy()
    handlers = c["handlers"] if isinstance(handlers, str) else handlers
    loads, air = c["loads"], c["air"]
    if carry:
        loads = dict(loads, thermostats=dict(loads["thermostats"], mode=carry["modes"])) if loads else None
        air = dict(air, **{k: carry["air"][k] for k in ahc.AIR_ACC}) if air else None
        handlers = ahc.handlers_with(handlers, carry["handlers"])
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(got)
        out = named(c, b.march_series(c["w"][steps], c["n_sub"], loads=loads, air=air, handlers=handlers, **dict(kwargs(c, steps), **more)))
        b.download_state(got)
    assert out["failed_step"] == -1
    return out, got


def carried(got):
    return dict(modes=got["modes"], air={k: got["air"][k] for k in ahc.AIR_ACC}, handlers={k: got["handlers"][k] for k in ("bypass",) + ah.ACC})


def same(ref, got, what, close=None):
    """A loop's result against a series': the discrete outputs exactly; the rows and sums bit for bit, or through close."""
    def value(r, g, name):
        if close is None:
            assert np.array_equal(r, g), "%s %s: %d differ, worst %.3e" % (what, name, int((r != g).sum()), np.abs(r - g).max())
        else:
            close(r, g, "%s %s" % (what, name))

    acc = ref["carry"]["handlers"]
    for key in DISCRETE:
        assert np.array_equal(acc[key], got["handlers"][key]), "%s %s: %d differ" % (what, key, int((acc[key] != got["handlers"][key]).sum()))
    if "modes" in got:
        assert np.array_equal(ref["carry"]["modes"], got["modes"]), what
        value(ref["applied"], got["applied"], "applied")
    if "air" in got:
        for key in ("state", "steps_open", "switches"):
            assert np.array_equal(ref["carry"]["air"][key], got["air"][key]), "%s air %s" % (what, key)
        value(ref["path_q"], got["air"]["path_q"], "path_q")
        value(ref["carry"]["air"]["sum_q"], got["air"]["sum_q"], "sum_q")
    for key in ah.ROWS:
        value(ref[key], got["handlers"][key], key)
    for key in REAL:
        value(acc[key], got["handlers"][key], key)
    value(ref["trace"], got["trace"], "trace")


# ---- 1. bit for bit against the per-call loop ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("n_sub", [2, 5])
@pytest.mark.parametrize("model", ALL_MODELS)
def test_series_with_air_handlers_equals_the_per_call_path_bit_for_bit(model, n_sub, opts):
    c = ahc.case(model, N_STEPS, n_sub, 2, ahc.SEED)
    own = owned_slots(c["md"])
    ref_state = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(ref_state)
        ref = ahc.loop_with_rules(lambda s, wk, za, zb: b.march(s, wk, za, zb, outputs=b.OUT_ALL), c, ref_state)
    # the inputs exercise the controllers (tests/test_air_handlers_host.py asserts it of the oracle loop alone)
    ahc.assert_coverage(ahc.coverage(c["handlers"], ref), "%s n_sub=%d (per-call path)" % (model, n_sub))
    got, state = series(c, opts)
    same(ref, got, model)
    assert np.array_equal(ref_state[own], state[own]), "%d state slots differ" % int((ref_state[own] != state[own]).sum())


# ---- 2. the oracle loop ----
_ORACLE_LOOPS = {}


def oracle_loop(oracle, model, n_sub):
    c = ahc.case(model, N_STEPS, n_sub, 2, ahc.SEED)
    if (model, n_sub) not in _ORACLE_LOOPS:  # (the same for every option set; left unchanged)
        big = c["md"]["n_surfaces"] > 8192
        m = oracle.OracleModel(c["md"])

        def march(s, wk, za, zb):
            assert m.march(s, wk, za, zb, threads=16 if big else 1)[0] == 0

        state = c["st"].copy()
        _ORACLE_LOOPS[(model, n_sub)] = (ahc.loop_with_rules(march, c, state), state)
    return (c,) + _ORACLE_LOOPS[(model, n_sub)]


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", [("ragged_mixed", 2), ("ragged_mixed", 5), ("rooms_with_windows", 2), ("rooms_with_windows", 5),
                                         ("partitioned_buildings_large", 2), ("rooms_with_windows_large", 5)])
def test_series_with_air_handlers_matches_the_oracle_loop(oracle, model, n_sub, opts):
    c, ref, ref_state = oracle_loop(oracle, model, n_sub)
    ahc.assert_coverage(ahc.coverage(c["handlers"], ref), "%s n_sub=%d (oracle loop)" % (model, n_sub))
    got, state = series(c, opts)
    same(ref, got, model, close=assert_close)
    own = owned_slots(c["md"])
    assert_close(ref_state[own], state[own], "%s final state" % model)


# ---- 3. cut ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("cut", [7, 16])
def test_series_with_air_handlers_cut_in_two_equals_the_series_in_one(cut, opts):
    c = ahc.case("rooms_with_windows", N_STEPS, 2, 2, ahc.SEED)
    one, state1 = series(c, opts)
    first, mid = series(c, opts, steps=slice(0, cut))
    second, state2 = series(c, opts, steps=slice(cut, None), state=mid, carry=carried(first))
    ctl = c["handlers"]["bypass_chan"] >= 0
    assert first["handlers"]["bypass"][ctl].any(), "no unit is bypassed at the cut: the bytes carry nothing over it"
    assert first["handlers"]["switches"].any() and first["handlers"]["sum_recovered"].any() and first["handlers"]["sum_branch_q"].any()
    assert np.array_equal(one["trace"], np.concatenate([first["trace"], second["trace"]]))
    assert np.array_equal(one["applied"], np.concatenate([first["applied"], second["applied"]]))
    for key in ah.ROWS:
        assert np.array_equal(one["handlers"][key], np.concatenate([first["handlers"][key], second["handlers"][key]])), key
    for key in DISCRETE + REAL:
        assert np.array_equal(one["handlers"][key], second["handlers"][key]), key
    assert np.array_equal(one["modes"], second["modes"]) and np.array_equal(state1, state2)


# ---- 4. every temperature is read as it was at the start of the step ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_a_unit_reads_the_zone_it_extracts_from_as_it_was_at_the_start_of_the_step(opts):
    c = ahc.case("rooms_with_windows", N_STEPS, 2, 2, ahc.SEED, with_loads=False, with_air=False)
    Z = int(c["md"]["n_zones"])
    A, B = 50, 3                                                     # zone A's lane runs behind zone B's; one unit, lane 0
    h = c["handlers"]
    one = dict(outdoor_chan=h["outdoor_chan"][:1], eff_gain=[0.8], br_unit=[0, 0], br_zone=[B, A], br_volume_chan=h["br_volume_chan"][:2],
               br_kind=[1, 2])
    got, _ = series(c, opts, handlers=one)
    zones = got["trace"][:, -Z:]                                     # (the case probes every zone last)
    start = np.concatenate([c["st"][c["md"]["zone_slot"]][None, :], zones[:-1]])   # what step k - 1 left
    want = [ah.apply(start[k], c["channel"][k], None, None, one, np.zeros(1, np.uint8))[2] for k in range(N_STEPS)]
    own = [ah.apply(zones[k], c["channel"][k], None, None, one, np.zeros(1, np.uint8))[2] for k in range(N_STEPS)]
    for key in ah.ROWS:
        assert np.array_equal(np.array([r[key] for r in want]), got["handlers"][key]), key
    assert (np.array([r["supply_t"][0] for r in own]) != got["handlers"]["supply_t"][:, 0]).sum() >= N_STEPS - 2   # ... not step k's own
    assert not got["handlers"]["branch_q"][:, 1].any() and got["handlers"]["branch_q"][:, 0].all()             # the extract branch: 0.0


# ---- 5. with ideal loads: they see the handlers' terms in every sub-timestep ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", [("rooms_with_windows", 2), ("rooms_with_windows_large", 5)])
def test_ideal_loads_see_the_air_handlers(model, n_sub, opts):
    c = ahc.case(model, N_STEPS, n_sub, 0, ahc.SEED, with_loads=False, with_air=False)
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
        out1 = b.march_series(c["w"], n_sub, ideal=ideal, handlers=c["handlers"], **kw)
        b.download_state(first)
    assert out1["failed_step"] == -1 and (out1["ideal_q"] > 0).any() and (out1["ideal_q"] < 0).any()
    # the rows the handlers formed, from the first run's zone trace; the bypass replayed on the way
    start = np.concatenate([c["st"][md["zone_slot"]][None, :], out1["trace"][:-1]])
    bypass = np.zeros(ah.n_units(c["handlers"]), np.uint8)
    rows = [ah.apply(start[k], channel[k], None, None, c["handlers"], bypass) for k in range(N_STEPS)]
    for key in ah.ROWS:
        assert np.array_equal(np.array([r[2][key] for r in rows]), out1["handlers"][key]), key
    assert np.array_equal(bypass, out1["handlers"]["bypass"])
    with HeatBatch(md, **opts) as b:
        b.upload_state(second)
        out2 = b.march_series(c["w"], n_sub, ideal=ideal, zone_a0=np.array([r[0] for r in rows]), zone_b0=np.array([r[1] for r in rows]), **kw)
        b.download_state(second)
    assert np.array_equal(out1["trace"], out2["trace"]) and np.array_equal(out1["ideal_q"], out2["ideal_q"])
    assert np.array_equal(first, second)
    for key in out1["ideal"]:
        assert np.array_equal(out1["ideal"][key], out2["ideal"][key]), key


# ---- 6. beside comfort control sensors, air paths, zone loads and blinds ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("n_sub", [2, 5])
def test_air_handlers_beside_every_other_term_equal_the_per_call_loop_bit_for_bit(n_sub, opts):
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(ahc.SEED + n_sub)
    c = cc.comfort_case(md, st, rng)
    c.channel, handlers, _ = ahc.random_handlers(md, np.asarray(st), rng, c.n_steps, c.channel)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, c.n_steps, 2)
    w = mdl.weather_series(c.n_steps * n_sub, md["dt"]).reshape(c.n_steps, n_sub, 3)
    acc, rows, sensed = ah.fresh(handlers), [], []

    def with_handlers(march):
        # comfort_cases.loop hands over the zone terms behind the loads' and the paths' rules; the inputs it has written by
        # then are no zone temperatures: the state still holds the air of the start of the step
        def step(state, k, za, zb):
            T = state[md["zone_slot"]].copy()
            za, zb, r = ah.apply(T, c.channel[k], za, zb, handlers, acc["bypass"])
            ah.accumulate(r, acc)
            rows.append(r), sensed.append(T)
            march(state, k, za, zb)
        return step

    want = st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(want)
        ref = cc.loop(c, want, with_handlers(cc.marcher(b, w)), probes, a0, b0)
    state = st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(state)
        out = b.march_series(w, n_sub, **cc.series_kwargs(c, probes, a0, b0, handlers=handlers))
        b.download_state(state)
    got = dict(zip(cc.NAMES + ("handlers",), out))
    assert len(out) == len(cc.NAMES) + 1
    cc.same_as_loop(ref, got, "n_sub=%d: " % n_sub)
    for key in ah.ROWS:
        assert np.array_equal(np.array([r[key] for r in rows]), got["handlers"][key]), key
    for key in ("bypass",) + ah.ACC:
        assert np.array_equal(acc[key], got["handlers"][key]), key
    own = owned_slots(md)
    assert np.array_equal(want[own], state[own])
    # the units sensed air where the controls sensed the operative temperature
    assert np.array_equal(np.array(sensed), ref["Tz"]) and not np.array_equal(ref["Tc"], ref["Tz"])
    assert acc["switches"].any() and acc["sum_heating"].any() and acc["sum_cooling"].any()


# ---- 7. NULL cases ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_no_air_handlers_is_the_series_without_them_bit_for_bit(opts):
    c = ahc.case("rooms_with_windows", 12, 3, 2, 5)
    C = binding.C
    results = []
    for how in ("plain", "empty", "null"):
        state = c["st"].copy()
        with HeatBatch(c["md"], **opts) as b:
            b.upload_state(state)
            if how == "plain":
                trace, failed, applied, modes, air = b.march_series(c["w"], 3, loads=c["loads"], air=c["air"], **kwargs(c))
            elif how == "empty":
                trace, failed, applied, modes, air, h = b.march_series(c["w"], 3, loads=c["loads"], air=c["air"], handlers={}, **kwargs(c))
                assert h["supply_t"].shape == (12, 0) and h["branch_q"].shape == (12, 0) and len(h["bypass"]) == 0
            else:  # h == NULL through the C ABI
                s, keep = binding.make_series(c["w"], 3, **kwargs(c))
                l, lkeep = binding.make_zone_loads(**c["loads"])
                a, akeep = binding.make_air_paths(**c["air"])
                trace, applied, f = np.zeros((12, len(c["probes"]))), np.zeros((12, l.n_thermostats)), C.c_int32(7)
                path_q = np.zeros((12, a.n_paths))
                call = binding.SeriesCall(size=C.sizeof(binding.SeriesCall), s=C.pointer(s), l=C.pointer(l), air=C.pointer(a), failed_step=C.pointer(f),
                                          trace=trace.ctypes.data_as(binding._dp), applied=applied.ctypes.data_as(binding._dp),
                                          path_q=path_q.ctypes.data_as(binding._dp))
                assert b._L.heat_batch_march_series_handlers(b._h, C.byref(call), None, None, None, None, None, None, None, None) == 0
                failed, modes = f.value, lkeep["th_mode"]
                air = dict(path_q=path_q, **{k: akeep[k] for k in ahc.AIR_ACC})
            b.download_state(state)
        assert failed == -1
        results.append((trace, applied, modes, state) + tuple(air[k] for k in ("path_q",) + ahc.AIR_ACC))
    for other in results[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(results[0], other))


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_an_array_that_is_not_asked_for_changes_no_bit_of_the_others(opts):
    c = ahc.case("ragged_mixed", N_STEPS, 2, 2, ahc.SEED)
    full, state = series(c, opts)
    U, B = ah.n_units(c["handlers"]), ah.n_branches(c["handlers"])
    for stats, rows in ([((s,), ()) for s in binding.HANDLER_STATS] + [((), (r,)) for r in ah.ROWS] + [((), ()), ((), ah.ROWS)]):
        got, st = series(c, opts, handlers=dict(c["handlers"], stats=stats), **{r: r in rows for r in ah.ROWS})
        assert set(got["handlers"]) == set(ah.ROWS) | {"bypass"} | set(stats)
        for r in ah.ROWS:
            assert got["handlers"][r].shape == ((N_STEPS if r in rows else 0), B if r == "branch_q" else U)
        for key, v in got["handlers"].items():
            if v.size:
                assert np.array_equal(v, full["handlers"][key]), (stats, rows, key)
        assert np.array_equal(got["trace"], full["trace"]) and np.array_equal(got["applied"], full["applied"]) and np.array_equal(st, state)
        assert np.array_equal(got["air"]["path_q"], full["air"]["path_q"])
    # bypass == NULL through the C ABI: every unit starts recovering, nothing is returned — the same series
    C = binding.C
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(c["st"].copy())
        s, keep = binding.make_series(c["w"], 2, **kwargs(c))
        l, lkeep = binding.make_zone_loads(**c["loads"])
        a, akeep = binding.make_air_paths(**c["air"])
        h, hkeep = binding.make_air_handlers(**c["handlers"])
        h.bypass = None
        t, q, f = np.zeros_like(full["trace"]), np.zeros_like(full["handlers"]["coil_q"]), C.c_int32(7)
        call = binding.SeriesCall(size=C.sizeof(binding.SeriesCall), s=C.pointer(s), l=C.pointer(l), air=C.pointer(a), failed_step=C.pointer(f),
                                  trace=t.ctypes.data_as(binding._dp))
        rc = b._L.heat_batch_march_series_handlers(b._h, C.byref(call), None, None, None, C.byref(h), None, None, q.ctypes.data_as(binding._dp), None)
    assert rc == 0 and f.value == -1
    assert np.array_equal(t, full["trace"]) and np.array_equal(q, full["handlers"]["coil_q"])
    assert np.array_equal(hkeep["sum_recovered"], full["handlers"]["sum_recovered"]) and np.array_equal(hkeep["switches"], full["handlers"]["switches"])
    assert full["handlers"]["steps_bypass"].any() and not hkeep["bypass"].any()  # (not written)


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_a_plain_series_after_one_with_air_handlers_is_the_plain_series_of_a_fresh_batch(opts):
    c = ahc.case("rooms_with_windows", 12, 2, 2, 9)
    fresh = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(fresh)
        want = b.march_series(c["w"], 2, **kwargs(c))
        b.download_state(fresh)
    after = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(c["st"].copy())
        b.march_series(c["w"], 2, loads=c["loads"], air=c["air"], handlers=c["handlers"], **kwargs(c))
        b.upload_state(after)
        got = b.march_series(c["w"], 2, **kwargs(c))
        b.download_state(after)
    assert np.array_equal(want[0], got[0]) and want[1] == got[1] == -1 and np.array_equal(fresh, after)


def test_a_series_of_no_sub_timestep_still_evaluates_the_units():
    c = ahc.case("ragged_mixed", 6, 1, 2, 21)
    # nothing marches: every step sees the zone temperatures of the start
    ref = ahc.loop_with_rules(lambda s, wk, za, zb: None, c, c["st"].copy())
    state = c["st"].copy()
    with HeatBatch(c["md"]) as b:
        b.upload_state(state)
        got = named(c, b.march_series(None, 0, n_steps=6, loads=c["loads"], air=c["air"], handlers=c["handlers"], **kwargs(c)))
        b.download_state(state)
    assert got["failed_step"] == -1 and np.array_equal(state, c["st"])
    assert (ref["branch_q"] != 0).any() and (ref["coil_q"] != 0).any()
    for key in ah.ROWS:
        assert np.array_equal(ref[key], got["handlers"][key]), key
    for key in DISCRETE + REAL:
        assert np.array_equal(ref["carry"]["handlers"][key], got["handlers"][key]), key


# ---- 8. NaN ----
def test_a_nan_volume_on_a_supply_branch_is_reported_as_the_zone_failure():
    """A NaN volume makes the branch's m NaN, and with it the zone's a0 and b0; the zone update itself would hide that
    (model.rs:662-668), so the handlers report it as the air paths do: HEAT_N_NAN_ZONE, at the step whose row holds the NaN."""
    md, st = mdl.clustered_massive(700, Z=28, dt=45.0, seed=3)
    n_steps, j = 9, 5
    good = np.tile([0.02, 0.01, 5.0], (n_steps, 1))                  # two volumes, the outdoor temperature
    channel = good.copy()
    channel[j, 0] = np.nan
    handlers = dict(outdoor_chan=[2, 2], eff_gain=[0.7, 0.7], br_unit=[0, 0, 1], br_zone=[13, 7, 2], br_volume_chan=[0, 1, 1], br_kind=[1, 2, 3])
    for opts, n_sub in [(o, n) for o in OPTIONS for n in (0, 2)]:
        w = mdl.weather_series(n_steps * n_sub, 45.0).reshape(n_steps, n_sub, 3) if n_sub else None
        with HeatBatch(md, **opts) as b:
            b.upload_state(st.copy())
            with pytest.raises(HeatError) as e:
                b.march_series(w, n_sub, handlers=handlers, channel=channel, probes=md["zone_slot"], n_steps=n_steps)
            assert e.value.failed_step == j and e.value.code == 3, str(e.value)   # HEAT_N_NAN_ZONE
            assert b.failed_surface() == (13, 3) and "zone 13" in str(e.value)
            assert np.all(np.isfinite(e.value.trace[:j]))
            # the process and the batch survive: a healthy series afterwards
            b.upload_state(st.copy())
            trace, failed, got = b.march_series(w, n_sub, handlers=handlers, channel=good, probes=md["zone_slot"], n_steps=n_steps)
            assert failed == -1 and np.all(np.isfinite(trace)) and np.all(np.isfinite(got["supply_t"])) and got["sum_recovered"].all()
    # the same NaN on a unit that only extracts fails nothing: sv is NaN, sv > 0.0 is false, the unit has nothing to recover from
    extract = dict(handlers, br_kind=[2, 2, 3])
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, got = b.march_series(mdl.weather_series(n_steps * 2, 45.0).reshape(n_steps, 2, 3), 2, handlers=extract, channel=channel,
                                            probes=md["zone_slot"])
    assert failed == -1 and np.all(np.isfinite(trace))
    assert got["supply_t"][j, 0] == 5.0 and got["recovered"][j, 0] == 0.0 and np.all(got["supply_t"][:j, 0] != 5.0)
    assert np.all(np.isfinite(got["supply_t"])) and not got["branch_q"][:, :2].any() and got["branch_q"][:, 2].all()


# ---- 9. one physical sanity check ----
def test_heat_recovery_keeps_a_ventilated_room_warmer_and_a_bypass_gives_it_up():
    md, st = mdl.partitioned_buildings(960, 12, seed=8)
    n_steps, n_sub, room = 40, 2, 1
    # a heater of 800 W in the room; 0.05 m3/s of outdoor air at 0 C through a balanced unit; a bypass setpoint far below
    channel = np.tile([800.0, 0.05, 0.0, -1000.0], (n_steps, 1))
    loads = dict(gains=dict(zone=[room], chan=[0]))
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    probes = md["zone_slot"][[room]]
    runs = {}
    with HeatBatch(md) as b:
        for name, unit in (("recovering", ah.balanced([room], 1, 2, eff_gain=0.8)), ("none", ah.balanced([room], 1, 2, eff_gain=0.0)),
                           ("bypassed", ah.balanced([room], 1, 2, eff_gain=0.8, bypass_chan=3))):
            b.upload_state(st.copy())
            trace, failed, _, _, got = b.march_series(w, n_sub, loads=loads, handlers=unit, channel=channel, probes=probes)
            assert failed == -1
            runs[name] = (trace, got)
    warm, cold, bypassed = runs["recovering"][0][-1, 0], runs["none"][0][-1, 0], runs["bypassed"][0][-1, 0]
    print("the room after %d steps: %.3f C with eta = 0.8, %.3f C with eta = 0; sum_recovered %s W" % (n_steps, warm, cold, runs["recovering"][1]["sum_recovered"]))
    assert warm > cold + 0.3 and runs["recovering"][1]["sum_recovered"][0] > 0.0
    assert not runs["none"][1]["sum_recovered"].any() and np.all(runs["recovering"][1]["branch_q"] < 0.0)
    # the room is warmer than its setpoint and than the air outside from the first step on: the bypass opens and stays open
    assert runs["bypassed"][1]["steps_bypass"][0] == n_steps and runs["bypassed"][1]["switches"][0] == 1 and runs["bypassed"][1]["bypass"][0] == 1
    assert np.array_equal(runs["bypassed"][0], runs["none"][0]) and np.array_equal(runs["bypassed"][1]["supply_t"], runs["none"][1]["supply_t"])
    assert not runs["recovering"][1]["coil_q"].any()


# ---- 10. refusals ----
def test_bad_handlers_and_sharded_batches_are_refused_by_the_march():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    w, channel = np.zeros((2, 1, 3)), np.zeros((2, 2))
    ok = dict(outdoor_chan=[0], br_unit=[0], br_zone=[1], br_volume_chan=[1])
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        for bad, code, needle in ((dict(ok, br_zone=[8]), -4, "air handler branch 0:"),
                                  (dict(ok, br_unit=[1]), -4, "air handler branch 0:"),
                                  (dict(ok, outdoor_chan=[2]), -4, "air handler 0:"),
                                  (dict(ok, br_kind=[0]), -1, "air handler branch 0:"),
                                  (dict(ok, heat_chan=[1], heat_cap=[-1.0]), -1, "air handler 0:"),
                                  (dict(ok, bypass_chan=[1], bypass_band=[np.nan], bypass_min_delta=[0.0]), -1, "air handler 0:"),
                                  (dict(ok, bypass=[2]), -1, "air handler 0:")):
            with pytest.raises(HeatError) as e:
                b.march_series(w, 1, channel=channel, handlers=bad)
            assert e.value.code == code and needle in str(e.value), str(e.value)
        got = st.copy()
        b.download_state(got)
        assert np.array_equal(got, st)
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, 1, channel=channel, handlers=ok)
        assert e.value.code == -1 and "sharded" in str(e.value)
