"""Controllers of a series on the GPU (include/heat_amd.h, heat_batch_march_series_controllers): modulating control loops evaluated
as the first kernel of every step from the zone and node temperatures the device holds, written into derived channels of the
device's copy of the channel table and read from there by the zone loads' gains, the room radiation, the openings' fractions,
the air paths and the driven inputs of the embedded slabs.

The expected result is DEFINED by controllers_cases.loop_with_rules — heat_amd.controllers.apply (the header's contract in numpy,
one rounded operation per line), then the openings' and the existing terms' rules on the row with its derived columns, applied
between per-step march calls to the temperatures the call before returned: through heat_batch_march_ex the series must agree bit
for bit, through OracleModel.march (≙ ThermalModel::march, src/model.rs:359-427) at rtol = atol = 1e-9, the project's parity
bound, with the discrete outputs equal. tests/test_controllers_host.py runs the same cases through the oracle alone and asserts
that the loops respond, that limits trip and release and that no decision comes within 1e-6 K of its threshold. The rule is this
project's own: the reference has no counterpart.

20 zones are 40 controllers, less than a wavefront; 500 zones 1 000: three full workgroups of 256 and a tail of 232 = 3 * 64 +
40."""
import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, air_species as asp, binding, controllers as ctl, modeldict as mdl, openings as opn
import air_species_cases as asc
import controllers_cases as cc
import openings_cases as oc
from air_handlers_cases import handlers_with
from test_series_gpu import assert_close, owned_slots, series_kwargs, _id

pytestmark = pytest.mark.gpu

OPTIONS = [dict(), dict(use_graph=True), dict(no_fusion=True)]
LARGE = "rooms_with_windows_large"
N_STEPS = cc.N_STEPS
NAMES = ("trace", "failed_step", "applied", "modes", "air", "irradiance", "sum_irradiance", "handlers", "species", "openings", "controllers")
DISCRETE = ("tripped", "steps_on", "steps_sat", "trips")


def kwargs(c, steps=slice(None)):
    return series_kwargs(c["channel"], c["drives"], c["probes"], c["a0"], c["b0"], steps=steps)


def series(c, opts, controllers="case", steps=slice(None), state=None, carry=None, step_base=0, **more):
    """One series with the case's loads, air paths, radiation, handlers, species, openings and `controllers` on a fresh batch,
    resumed from `carry` (a loop's, or carried() of a series). Returns (the named result, the final state)."""
    got = c["st"].copy() if state is None else state.copy()
    controllers = c["controllers"] if isinstance(controllers, str) else controllers
    loads, air, handlers, species, openings, radiation = c["loads"], c["air"], c["handlers"], c["species"], c["openings"], c["radiation"]
    if carry:
        loads = dict(loads, thermostats=dict(loads["thermostats"], mode=carry["modes"]))
        air = dict(air, **{k: carry["air"][k] for k in asc.AIR_ACC})
        handlers = handlers_with(handlers, carry["handlers"])
        species = asc.species_with(species, carry["species"], step_base)
        openings = oc.openings_with(openings, carry["openings"], step_base)
        radiation = dict(radiation, sum_irradiance=carry["sum_irradiance"])
        if controllers is not None:
            controllers = cc.controllers_with(controllers, carry["controllers"])
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(got)
        out = b.march_series(c["w"][steps], c["n_sub"], loads=loads, air=air, radiation=radiation, handlers=handlers, species=species,
                             openings=openings, controllers=controllers, **dict(kwargs(c, steps), **more))
        b.download_state(got)
        counts = b.class_counts()
    names = NAMES if controllers is not None else NAMES[:-1]
    assert len(out) == len(names)
    out = dict(zip(names, out))
    assert out["failed_step"] == -1
    out["class_counts"] = counts
    return out, got


def carried(got):
    return dict(modes=got["modes"], air={k: got["air"][k] for k in asc.AIR_ACC}, handlers={k: v for k, v in got["handlers"].items() if v.ndim == 1},
                species={k: got["species"][k] for k in ("conc",) + asp.ACC}, openings={k: got["openings"][k] for k in opn.ACC},
                sum_irradiance=got["sum_irradiance"], controllers={k: got["controllers"][k] for k in ctl.STATE + ctl.ACC})


def same(ref, got, what, close=None):
    """A loop's result against a series': the discrete outputs exactly; the rows, sums and state bit for bit, or through close."""
    def value(r, g, name):
        if close is None:
            assert np.array_equal(r, g, equal_nan=True), "%s %s: %d differ, worst %.3e" % (what, name, int((r != g).sum()), np.nanmax(np.abs(r - g)))
        else:
            close(r, g, "%s %s" % (what, name))

    acc = ref["carry"]
    for key in DISCRETE:
        assert np.array_equal(acc["controllers"][key], got["controllers"][key]), "%s %s: %d differ" % (
            what, key, int((acc["controllers"][key] != got["controllers"][key]).sum()))
    assert np.array_equal(acc["openings"]["step_max"], got["openings"]["step_max"]), "%s step_max" % what
    for key in asc.DISCRETE:
        assert np.array_equal(acc["species"][key], got["species"][key]), "%s %s" % (what, key)
    assert np.array_equal(acc["modes"], got["modes"]), "%s modes" % what
    for key in ("state", "steps_open", "switches"):
        assert np.array_equal(acc["air"][key], got["air"][key]), "%s air %s" % (what, key)
    if close is not None:      # where a signal sits on a clamp in the loop it does in the series
        assert np.array_equal(ref["control_u"] == 0.0, got["controllers"]["control_u"] == 0.0), "%s u == 0" % what
        assert np.array_equal(ref["control_u"] == 1.0, got["controllers"]["control_u"] == 1.0), "%s u == 1" % what
    value(ref["control_u"], got["controllers"]["control_u"], "control_u")
    value(ref["control_out"], got["controllers"]["control_out"], "control_out")
    for key in ("integral", "sum_u", "sum_out"):
        value(acc["controllers"][key], got["controllers"][key], key)
    value(ref["opening_v"], got["openings"]["opening_v"], "opening_v")
    value(acc["openings"]["sum_v"], got["openings"]["sum_v"], "sum_v")
    value(ref["irradiance"], got["irradiance"], "irradiance")
    value(acc["sum_irradiance"], got["sum_irradiance"], "sum_irradiance")
    value(ref["path_q"], got["air"]["path_q"], "path_q")
    value(ref["applied"], got["applied"], "applied")
    value(ref["branch_q"], got["handlers"]["branch_q"], "branch_q")
    for key in asp.ROWS:
        value(ref[key], got["species"][key], key)
    for key in asc.REAL:
        value(acc["species"][key], got["species"][key], key)
    value(ref["trace"], got["trace"], "trace")


# ---- 1. bit for bit against the per-call loop ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", [("ragged_mixed", 2), ("ragged_mixed", 5), (LARGE, 2), (LARGE, 5)])
def test_series_with_controllers_equals_the_per_call_path_bit_for_bit(model, n_sub, opts):
    c = cc.case(model, N_STEPS, n_sub, 2, cc.SEED, floor=False)
    n, info = ctl.n_controllers(c["controllers"]), c["controllers_info"]
    assert (n == 40 and model == "ragged_mixed") or (n == 1000 and model == LARGE)
    own = owned_slots(c["md"])
    ref_state = c["st"].copy()
    with HeatBatch(c["md_plain"], **opts) as b:
        plain_counts = b.class_counts()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(ref_state)
        ref = cc.loop_with_rules(lambda s, wk, za, zb: b.march(s, wk, za, zb, outputs=b.OUT_ALL), c, ref_state)
    cc.assert_coverage(cc.coverage(c, ref), "%s n_sub=%d (per-call path)" % (model, n_sub))
    got, state = series(c, opts)
    # a wall that absorbs inside marches in the general class, which applies its whole alpha row (controllers.embed)
    assert got["class_counts"][4] == plain_counts[4] + info["general"] and sum(got["class_counts"]) == sum(plain_counts)
    same(ref, got, model)
    assert np.array_equal(ref_state[own], state[own]), "%d state slots differ" % int((ref_state[own] != state[own]).sum())


# ---- 2. the oracle loop ----
_ORACLE_LOOPS = {}


def oracle_loop(oracle, model, n_sub):
    c = cc.case(model, N_STEPS, n_sub, 2, cc.SEED)
    if (model, n_sub) not in _ORACLE_LOOPS:  # (the same for every option set; left unchanged)
        m = oracle.OracleModel(c["md"])

        def march(s, wk, za, zb):
            assert m.march(s, wk, za, zb, threads=1)[0] == 0

        state = c["st"].copy()
        _ORACLE_LOOPS[(model, n_sub)] = (cc.loop_with_rules(march, c, state), state)
    return (c,) + _ORACLE_LOOPS[(model, n_sub)]


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", cc.ORACLE_CASES)
def test_series_with_controllers_matches_the_oracle_loop(oracle, model, n_sub, opts):
    """rtol = atol = 1e-9 on the cases whose decisions — limits, clamps' edges, the openings' and paths' thresholds — keep 1e-6 K
    from their thresholds in the oracle loop (tests/test_controllers_host.py asserts it; the assertion is repeated here on the
    loop this test compares against). u is Lipschitz in the temperatures with constant kp + ki <= 1 / 2 K + 1 / 8 K per step."""
    c, ref, ref_state = oracle_loop(oracle, model, n_sub)
    assert cc.margin(c, ref) >= cc.MARGIN
    cc.assert_coverage(cc.coverage(c, ref), "%s n_sub=%d (oracle loop)" % (model, n_sub))
    got, state = series(c, opts)
    same(ref, got, model, close=assert_close)
    own = owned_slots(c["md"])
    assert_close(ref_state[own], state[own], "%s final state" % model)


# ---- 3. cut ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("cut", [7, 15])
def test_series_with_controllers_cut_in_two_equals_the_series_in_one(cut, opts):
    c = cc.case("ragged_mixed", N_STEPS, 2, 2, cc.SEED, floor=False)
    one, state1 = series(c, opts)
    first, mid = series(c, opts, steps=slice(0, cut))
    second, state2 = series(c, opts, steps=slice(cut, None), state=mid, carry=carried(first), step_base=cut)
    at_cut = first["controllers"]
    assert at_cut["tripped"].any() and (at_cut["integral"] > 0).any() and (at_cut["trips"] < one["controllers"]["trips"]).any()
    assert np.array_equal(one["trace"], np.concatenate([first["trace"], second["trace"]]))
    for key in ("control_u", "control_out"):
        assert np.array_equal(one["controllers"][key], np.concatenate([first["controllers"][key], second["controllers"][key]])), key
    assert np.array_equal(one["openings"]["opening_v"], np.concatenate([first["openings"]["opening_v"], second["openings"]["opening_v"]]))
    assert np.array_equal(one["irradiance"], np.concatenate([first["irradiance"], second["irradiance"]]))
    for key in ctl.STATE + ctl.ACC:
        assert np.array_equal(one["controllers"][key], second["controllers"][key]), key
    for key in opn.ACC:
        assert np.array_equal(one["openings"][key], second["openings"][key]), key
    assert np.array_equal(one["sum_irradiance"], second["sum_irradiance"]) and np.array_equal(one["modes"], second["modes"])
    assert np.array_equal(state1, state2)


# ---- 4. no controllers ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_no_controllers_is_the_series_with_openings_bit_for_bit(opts):
    c = oc.case("rooms_with_windows", 12, 3, 2, 5, floor=False)
    C, dp = binding.C, binding._dp
    results = []
    for how in ("plain", "empty", "null"):
        state = c["st"].copy()
        with HeatBatch(c["md"], **opts) as b:
            b.upload_state(state)
            terms = dict(loads=c["loads"], air=c["air"], handlers=c["handlers"], species=c["species"], openings=c["openings"])
            if how == "plain":
                trace, failed, applied, modes, air, hd, sp, op = b.march_series(c["w"], 3, **terms, **kwargs(c))
            elif how == "empty":
                trace, failed, applied, modes, air, hd, sp, op, ct = b.march_series(c["w"], 3, controllers={}, **terms, **kwargs(c))
                assert ct["control_u"].shape == (12, 0) and ct["control_out"].shape == (12, 0) and ct["integral"].size == 0
            else:  # ct == NULL through the C ABI
                s, keep = binding.make_series(c["w"], 3, **kwargs(c))
                l, lkeep = binding.make_zone_loads(**c["loads"])
                a, akeep = binding.make_air_paths(**c["air"])
                h, hkeep = binding.make_air_handlers(**c["handlers"])
                spc, spkeep = binding.make_air_species(**c["species"])
                opc, opkeep = binding.make_openings(**c["openings"])
                Z = int(c["md"]["n_zones"])
                trace, applied, f = np.zeros((12, len(c["probes"]))), np.zeros((12, l.n_thermostats)), C.c_int32(7)
                path_q, branch_q, conc_rows = np.zeros((12, a.n_paths)), np.zeros((12, h.n_branches)), np.zeros((12, spc.n_species, Z))
                opening_v = np.zeros((12, opc.n_openings))
                call = binding.SeriesCall(size=C.sizeof(binding.SeriesCall), s=C.pointer(s), l=C.pointer(l), air=C.pointer(a), failed_step=C.pointer(f),
                                          trace=trace.ctypes.data_as(dp), applied=applied.ctypes.data_as(dp), path_q=path_q.ctypes.data_as(dp))
                assert b._L.heat_batch_march_series_controllers(b._h, C.byref(call), None, None, None, C.byref(h), None, None, None,
                                                                branch_q.ctypes.data_as(dp), C.byref(spc), conc_rows.ctypes.data_as(dp), None, None,
                                                                C.byref(opc), opening_v.ctypes.data_as(dp), None, None, None) == 0
                failed, modes = f.value, lkeep["th_mode"]
                air = dict(path_q=path_q, **{k: akeep[k] for k in asc.AIR_ACC})
                hd = dict(branch_q=branch_q, bypass=hkeep["bypass"])
                sp = dict(conc_rows=conc_rows, **{k: spkeep[k] for k in ("conc",) + asp.ACC})
                op = dict(opening_v=opening_v, **{k: opkeep[k] for k in opn.ACC})
            b.download_state(state)
        assert failed == -1
        results.append((trace, applied, modes, state, hd["branch_q"], hd["bypass"], sp["conc_rows"], op["opening_v"]) +
                       tuple(sp[k] for k in ("conc",) + asp.ACC) + tuple(op[k] for k in opn.ACC) + tuple(air[k] for k in ("path_q",) + asc.AIR_ACC))
    for other in results[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(results[0], other))


# ---- 5. nullable outputs ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_an_array_that_is_not_asked_for_changes_no_bit_of_the_others(opts):
    c = cc.case("ragged_mixed", N_STEPS, 2, 2, cc.SEED, floor=False)
    full, state = series(c, opts)
    n = ctl.n_controllers(c["controllers"])
    every = binding.CONTROLLER_STATS
    for state_names, stats, u_rows, out_rows in (((), (), False, False), (("integral",), ("sum_u",), True, False), (("tripped",), ("trips", "sum_out"), False, True),
                                                 ((), ("steps_on", "steps_sat"), True, True), (binding.CONTROLLER_STATE, every, False, False),
                                                 (binding.CONTROLLER_STATE, (), True, True)):
        got, st = series(c, opts, controllers=dict(c["controllers"], state=state_names, stats=stats), control_u=u_rows, control_out=out_rows)
        assert set(got["controllers"]) == {"control_u", "control_out"} | set(state_names) | set(stats)
        assert got["controllers"]["control_u"].shape == ((N_STEPS if u_rows else 0), n)
        assert got["controllers"]["control_out"].shape == ((N_STEPS if out_rows else 0), n)
        for key, v in got["controllers"].items():
            if v.size:
                assert np.array_equal(v, full["controllers"][key]), (state_names, stats, key)
        assert np.array_equal(got["trace"], full["trace"]) and np.array_equal(got["applied"], full["applied"]) and np.array_equal(st, state)
        assert np.array_equal(got["air"]["path_q"], full["air"]["path_q"]) and np.array_equal(got["openings"]["opening_v"], full["openings"]["opening_v"])
        assert np.array_equal(got["irradiance"], full["irradiance"])


# ---- 6. refusals ----
def test_bad_controllers_and_sharded_batches_are_refused_and_leave_the_device_untouched():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    w, channel = np.zeros((2, 1, 3)), np.zeros((2, 8))
    channel[:, 0] = 30.0
    ok = dict(sense_kind=[0, 1], sense_index=[1, 17], sense_node=[-1, 2], set_chan=[0, 0], en_chan=[-1, 1], lim_kind=[-1, 1], lim_index=[-1, 17],
              out_chan=[6, 7], kp=[0.5, 0.25], ki=[0.0, 0.1], out_hi=[500.0, 1.0], lim_hi=[0.0, 29.0], lim_lo=[0.0, 27.0])
    op = dict(zone_a=[1], zone_b=[-1], temp_chan=[2], frac_chan=[7], out_chan=[5], area=[0.5], cs=[9.0], c0=[0.01])
    n_nodes = int(np.diff(md["node_offset"])[17])
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        for bad, code, needle in ((dict(ok, sense_index=[8, 17]), -4, "controller 0:"),
                                  (dict(ok, sense_node=[-1, n_nodes]), -4, "controller 1:"),
                                  (dict(ok, sense_kind=[0, 3]), -1, "controller 1:"),
                                  (dict(ok, set_chan=[0, -1]), -4, "controller 1:"),
                                  (dict(ok, out_chan=[6, 6]), -4, "controller 1:"),
                                  (dict(ok, out_chan=[6, 5]), -4, "controller 1:"),            # the opening's
                                  (dict(ok, set_chan=[7, 0]), -4, "controller 0:"),            # a controller's
                                  (dict(ok, en_chan=[5, 1]), -4, "controller 0:"),             # the opening's: openings run behind
                                  (dict(ok, kp=[0.5, -0.25]), -1, "controller 1:"),
                                  (dict(ok, out_hi=[np.nan, 1.0]), -1, "controller 0:"),
                                  (dict(ok, lim_lo=[0.0, 29.5]), -1, "controller 1:"),
                                  (dict(ok, resume=dict(ctl.fresh(ok), tripped=[0, 2])), -1, "controller 1:"),
                                  (dict(ok, resume=dict(ctl.fresh(ok), integral=[1.5, 0.0])), -1, "controller 0:")):
            with pytest.raises(HeatError) as e:
                b.march_series(w, 1, channel=channel, openings=op, controllers=bad)
            assert e.value.code == code and needle in str(e.value), str(e.value)
        got = st.copy()
        own = owned_slots(md)
        got[own] = np.nan                                             # (a download writes the slots the device owns, and only those)
        b.download_state(got)
        assert np.array_equal(got, st)
        # the batch marches on: a good term afterwards
        trace, failed, o, ct = b.march_series(w, 1, channel=channel, openings=op, controllers=ok, probes=md["zone_slot"])
        assert failed == -1 and np.isfinite(ct["control_u"]).all() and (ct["control_u"][:, 0] == 1.0).all() and (ct["control_u"][:, 1] == 0.0).all()
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, 1, channel=channel, controllers=ok)
        assert e.value.code == -1 and "sharded" in str(e.value)


# ---- 7. a sensed node, alone ----
def test_a_controller_senses_the_node_the_descriptor_names_wherever_the_device_keeps_it():
    """One controller per surface of a ragged model, each sensing a node of its own wall, with kp so small that u = kp (100 - Tn)
    stays inside (0, 1): u of step 0 gives back the node temperatures of the uploaded state, whose places in the device's packed
    buffer follow no descriptor numbering."""
    md, st = mdl.ragged_mixed(300, Z=6, seed=5)
    S = int(md["n_surfaces"])
    count = np.diff(md["node_offset"])
    rng = np.random.default_rng(9)
    node = np.where(np.arange(S) % 3 == 0, -1, rng.integers(0, 1 << 30, S) % count)
    ct = dict(sense_kind=np.ones(S, np.int32), sense_index=np.arange(S), sense_node=node, set_chan=np.zeros(S, np.int32), out_chan=1 + np.arange(S),
              kp=np.full(S, 1.0 / 256.0), out_hi=np.ones(S))
    channel = np.full((1, 1 + S), np.nan)
    channel[:, 0] = 100.0
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, got = b.march_series(None, 0, n_steps=1, channel=channel, controllers=ct)
    Tn = st[md["first_node_slot"] + np.where(node < 0, count - 1, node)]
    assert failed == -1 and np.array_equal(got["control_u"][0], (100.0 - Tn) * (1.0 / 256.0)) and len(np.unique(Tn)) > S // 2


# ---- 8. no sub-timestep; NaN ----
def test_a_series_of_no_sub_timestep_still_evaluates_the_controllers():
    c = cc.case("ragged_mixed", 6, 0, 2, 21, floor=False)
    ref = cc.loop_with_rules(lambda s, wk, za, zb: None, c, c["st"].copy())          # nothing marches: every step sees the start
    state = c["st"].copy()
    with HeatBatch(c["md"]) as b:
        b.upload_state(state)
        got = dict(zip(NAMES, b.march_series(None, 0, n_steps=6, loads=c["loads"], air=c["air"], radiation=c["radiation"], handlers=c["handlers"],
                                             species=c["species"], openings=c["openings"], controllers=c["controllers"], **kwargs(c))))
        b.download_state(state)
    own = owned_slots(c["md"])
    assert got["failed_step"] == -1 and np.array_equal(state[own], c["st"][own]) and (ref["control_u"] > 0).any() and (ref["control_u"] < 1).any()
    assert np.array_equal(ref["control_u"], got["controllers"]["control_u"]) and np.array_equal(ref["control_out"], got["controllers"]["control_out"])
    assert np.array_equal(ref["opening_v"], got["openings"]["opening_v"]) and np.array_equal(ref["path_q"], got["air"]["path_q"])
    for key in ctl.STATE + ctl.ACC:
        assert np.array_equal(ref["carry"]["controllers"][key], got["controllers"][key]), key


def test_a_nan_setpoint_is_data_until_a_gain_adds_it_to_a_zone():
    """A NaN setpoint makes u and out NaN, and the integral with them (0 * NaN, whatever ki is): the signal stays NaN until the
    controller is disabled, which zeroes the integral. Read by nothing the NaNs stay in their rows and fail nothing; read by a
    gain of the zone loads they make the zone's a0 NaN, which the loads report as HEAT_N_NAN_ZONE at that step, as they do for a
    NaN in an ordinary channel."""
    md, st = mdl.clustered_massive(700, Z=28, dt=45.0, seed=3)
    n_steps, j = 9, 4
    channel = np.tile([30.0, np.nan, 1.0], (n_steps, 1))                 # the setpoint, the derived channel, the enable
    channel[j, 0] = np.nan
    channel[j + 2, 2] = 0.0
    ct = dict(sense_index=[13], set_chan=[0], en_chan=[2], out_chan=[1], kp=[0.05], out_hi=[800.0])
    w = mdl.weather_series(n_steps * 2, 45.0).reshape(n_steps, 2, 3)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, got = b.march_series(w, 2, controllers=ct, channel=channel, probes=md["zone_slot"])
        assert failed == -1 and np.isfinite(trace).all()
        u, out = got["control_u"][:, 0], got["control_out"][:, 0]
        assert np.isnan(u[j:j + 2]).all() and np.isnan(out[j:j + 2]).all() and u[j + 2] == 0.0 and out[j + 2] == 0.0
        assert np.isfinite(np.delete(u, [j, j + 1])).all() and (np.delete(u, [j, j + 1, j + 2]) > 0).all()
        assert np.isnan(got["sum_u"][0]) and got["steps_on"][0] == n_steps - 3 and got["integral"][0] == 0.0 and got["trips"][0] == 0
        # The gain makes a0 of zone 13 NaN: the loads flag the zone at step j, and heat_batch_failed_surface names it with
        # HEAT_N_NAN_ZONE. That is the call's status too where the step ends before a wall has seen the zone's NaN temperature
        # (no sub-timestep, or one: the zone balance closes it); with two, the walls of zone 13 meet it in the second and
        # heat_batch_synchronize, which has always ranked a NaN convection coefficient first, returns HEAT_N_NAN_HS.
        for n_sub in (0, 1, 2):
            b.upload_state(st.copy())
            with pytest.raises(HeatError) as e:
                b.march_series(w[:, :n_sub] if n_sub else None, n_sub, controllers=ct, loads=dict(gains=dict(zone=[13], chan=[1])), channel=channel,
                               probes=md["zone_slot"], **(dict(n_steps=n_steps) if n_sub == 0 else {}))
            assert e.value.failed_step == j and e.value.code == (3 if n_sub < 2 else 1), (n_sub, str(e.value))
            assert b.failed_surface() == (13, 3) and np.all(np.isfinite(e.value.trace[:j])) and "zone 13" in str(e.value)
