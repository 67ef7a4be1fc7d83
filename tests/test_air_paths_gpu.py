"""Air paths of a series on the GPU (include/heat_amd.h, heat_batch_march_series_air): air that moves between zones and vents
controlled on both of their ends, formed on the device at every step of a series.

The expected result is DEFINED by air_paths_cases.loop_with_rules — the zone loads' rule, then heat_amd.air_paths.apply (the
header's contract in numpy, one rounded operation per product and sum), applied between per-step march calls to the zone
temperatures the call before returned: through heat_batch_march_ex the series must agree bit for bit, through
OracleModel.march (≙ ThermalModel::march, src/model.rs:359-427) at rtol = atol = 1e-9, the project's parity bound, with the
discrete outputs equal. tests/test_air_paths_host.py runs the same cases through the oracle alone and asserts that the vents
move. The rule is this project's own: the reference leaves the mixing of air between zones unimplemented
(model.rs:546,592-593); the air properties are the reference's (gas.rs:49,165-179).

Z = 20 is less than a wavefront; Z = 500 is two workgroups of 256 lanes with a ragged tail and sources in the other one."""
import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, air_paths, binding, modeldict as mdl
import air_paths_cases as apc
from test_series_gpu import assert_close, owned_slots, series_kwargs, _id

pytestmark = pytest.mark.gpu

OPTIONS = [dict(), dict(use_graph=True), dict(no_fusion=True)]
ALL_MODELS = ["ragged_mixed", "rooms_with_windows", "partitioned_buildings_large", "rooms_with_windows_large"]
N_STEPS = 24
DISCRETE = ("state", "steps_open", "switches")


def kwargs(c, steps=slice(None)):
    return series_kwargs(c["channel"], c["drives"], c["probes"], c["a0"], c["b0"], steps=steps)


def series(c, opts, air="case", steps=slice(None), state=None, batch=None, **more):
    """One series with the case's loads and `air` on a fresh batch. Returns (trace, applied, modes, air dict, state)."""
    got = c["st"].copy() if state is None else state.copy()
    air = c["air"] if isinstance(air, str) else air
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(got)
        out = b.march_series(c["w"][steps], c["n_sub"], loads=c["loads"], air=air, **dict(kwargs(c, steps), **more))
        b.download_state(got)
    assert out[1] == -1
    if c["loads"] is None:
        return out[0], None, None, out[2], got
    return out[0], out[2], out[3], out[4], got


def describe(what, c, ref):
    open_share, switching, senses = apc.coverage(c["air"], ref)
    print("%s: %d paths; %.0f %% of the controlled step-paths open, %.0f %% of the controlled paths switch, senses %s" % (
        what, len(c["air"]["target"]), 100 * open_share, 100 * switching, sorted(senses)))
    return open_share, switching, senses


# ---- 1. bit for bit against the per-call loop ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("n_sub", [2, 5])
@pytest.mark.parametrize("model", ALL_MODELS)
def test_series_with_air_paths_equals_the_per_call_path_bit_for_bit(model, n_sub, opts):
    c = apc.case(model, N_STEPS, n_sub, 2, apc.SEED)
    own = owned_slots(c["md"])
    ref_state = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(ref_state)
        ref = apc.loop_with_rules(lambda s, wk, za, zb: b.march(s, wk, za, zb, outputs=b.OUT_ALL), c, ref_state)
    open_share, switching, senses = describe("%s n_sub=%d (per-call path)" % (model, n_sub), c, ref)
    # the inputs exercise the controllers (tests/test_air_paths_host.py asserts it of the oracle loop alone)
    assert 0.2 < open_share < 0.8 and switching > 0.2 and senses == {1, -1}
    trace, applied, modes, got, state = series(c, opts)
    assert np.array_equal(ref["path_q"], got["path_q"]), "%d path powers differ, worst %.3e" % (
        int((ref["path_q"] != got["path_q"]).sum()), np.abs(ref["path_q"] - got["path_q"]).max())
    for key in DISCRETE + ("sum_q",):
        assert np.array_equal(ref[key], got[key]), "%s: %d differ" % (key, int((ref[key] != got[key]).sum()))
    assert np.array_equal(ref["applied"], applied) and np.array_equal(ref["modes"], modes)
    assert np.array_equal(ref["trace"], trace), "%d trace values differ, worst %.3e" % (
        int((ref["trace"] != trace).sum()), np.abs(ref["trace"] - trace).max())
    assert np.array_equal(ref_state[own], state[own]), "%d state slots differ" % int((ref_state[own] != state[own]).sum())


# ---- 2. the oracle loop ----
_ORACLE_LOOPS = {}


def oracle_loop(oracle, model, n_sub):
    c = apc.case(model, N_STEPS, n_sub, 2, apc.SEED)
    if (model, n_sub) not in _ORACLE_LOOPS:  # (the same for every option set; left unchanged)
        big = c["md"]["n_surfaces"] > 8192
        m = oracle.OracleModel(c["md"])

        def march(s, wk, za, zb):
            assert m.march(s, wk, za, zb, threads=16 if big else 1)[0] == 0

        state = c["st"].copy()
        _ORACLE_LOOPS[(model, n_sub)] = (apc.loop_with_rules(march, c, state), state)
    return (c,) + _ORACLE_LOOPS[(model, n_sub)]


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", [("ragged_mixed", 2), ("ragged_mixed", 5), ("rooms_with_windows", 2), ("rooms_with_windows", 5),
                                         ("partitioned_buildings_large", 2), ("rooms_with_windows_large", 5)])
def test_series_with_air_paths_matches_the_oracle_loop(oracle, model, n_sub, opts):
    c, ref, ref_state = oracle_loop(oracle, model, n_sub)
    describe("%s n_sub=%d (oracle loop)" % (model, n_sub), c, ref)
    trace, applied, modes, got, state = series(c, opts)
    for key in DISCRETE:
        assert np.array_equal(ref[key], got[key]), "%s: %d differ" % (key, int((ref[key] != got[key]).sum()))
    assert np.array_equal(ref["modes"], modes)
    assert_close(ref["trace"], trace, "%s trace" % model)
    assert_close(ref["applied"], applied, "%s applied" % model)
    assert_close(ref["path_q"], got["path_q"], "%s path_q" % model)
    assert_close(ref["sum_q"], got["sum_q"], "%s sum_q" % model)
    own = owned_slots(c["md"])
    assert_close(ref_state[own], state[own], "%s final state" % model)


# ---- 3. cut ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("cut", [7, 16])
def test_series_with_air_paths_cut_in_two_equals_the_series_in_one(cut, opts):
    c = apc.case("rooms_with_windows", N_STEPS, 2, 2, apc.SEED)
    trace1, applied1, modes1, one, state1 = series(c, opts)
    two = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(two)
        ta, _, aa, ma, first = b.march_series(c["w"][:cut], 2, loads=c["loads"], air=c["air"], **kwargs(c, slice(0, cut)))
        loads2 = dict(c["loads"], thermostats=dict(c["loads"]["thermostats"], mode=ma))
        resumed = dict(c["air"], **{k: first[k] for k in DISCRETE + ("sum_q",)})
        tb, _, ab, mb, second = b.march_series(c["w"][cut:], 2, loads=loads2, air=resumed, **kwargs(c, slice(cut, None)))
        b.download_state(two)
    ctl = c["air"]["open_chan"] >= 0
    assert first["state"][ctl].any(), "no controlled path is open at the cut: the states carry nothing over it"
    assert first["switches"].any() and first["sum_q"].any()
    assert np.array_equal(trace1, np.concatenate([ta, tb])) and np.array_equal(applied1, np.concatenate([aa, ab]))
    assert np.array_equal(one["path_q"], np.concatenate([first["path_q"], second["path_q"]]))
    for key in DISCRETE + ("sum_q",):
        assert np.array_equal(one[key], second[key]), key
    assert np.array_equal(modes1, mb) and np.array_equal(state1, two)


# ---- 4. every source is read as it was at the start of the step ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_a_chain_does_not_propagate_within_a_step(opts):
    c = apc.case("rooms_with_windows", N_STEPS, 2, 2, apc.SEED)
    Z = int(c["md"]["n_zones"])
    trace, _, _, got, _ = series(c, opts)
    zones = trace[:, -Z:]                                            # (the case probes every zone last)
    start = np.concatenate([c["st"][c["md"]["zone_slot"]][None, :], zones[:-1]])   # what step k - 1 left
    for i, (src, dst) in zip(c["info"]["chain"], ((4, 5), (5, 6))):
        one = {k: v[i:i + 1] for k, v in c["air"].items()}
        assert (int(one["source"][0]), int(one["target"][0])) == (src, dst) and one["open_chan"][0] < 0
        want = np.array([air_paths.apply(start[k], c["channel"][k], None, None, one, np.zeros(1, np.uint8))[2][0] for k in range(N_STEPS)])
        own = np.array([air_paths.apply(zones[k], c["channel"][k], None, None, one, np.zeros(1, np.uint8))[2][0] for k in range(N_STEPS)])
        assert np.array_equal(want, got["path_q"][:, i])
        assert (own != got["path_q"][:, i]).sum() >= N_STEPS - 2     # ... and not to step k's own values


# ---- 5. with ideal loads: they see the paths' terms in every sub-timestep ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", [("rooms_with_windows", 2), ("rooms_with_windows_large", 5)])
def test_ideal_loads_see_the_air_paths(model, n_sub, opts):
    c = apc.case(model, N_STEPS, n_sub, 0, apc.SEED, with_loads=False)
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
        out1 = b.march_series(c["w"], n_sub, ideal=ideal, air=c["air"], **kw)
        b.download_state(first)
    assert out1["failed_step"] == -1 and (out1["ideal_q"] > 0).any() and (out1["ideal_q"] < 0).any()
    # the rows the paths formed, from the first run's zone trace; the controllers replayed on the way
    start = np.concatenate([c["st"][md["zone_slot"]][None, :], out1["trace"][:-1]])
    state = np.zeros(len(c["air"]["target"]), np.uint8)
    rows = [air_paths.apply(start[k], channel[k], None, None, c["air"], state) for k in range(N_STEPS)]
    assert np.array_equal(np.array([r[2] for r in rows]), out1["air"]["path_q"]) and np.array_equal(state, out1["air"]["state"])
    with HeatBatch(md, **opts) as b:
        b.upload_state(second)
        out2 = b.march_series(c["w"], n_sub, ideal=ideal, zone_a0=np.array([r[0] for r in rows]), zone_b0=np.array([r[1] for r in rows]), **kw)
        b.download_state(second)
    assert np.array_equal(out1["trace"], out2["trace"]) and np.array_equal(out1["ideal_q"], out2["ideal_q"])
    assert np.array_equal(first, second)
    for key in out1["ideal"]:
        assert np.array_equal(out1["ideal"][key], out2["ideal"][key]), key


# ---- 6. NULL cases ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_no_air_paths_is_the_series_without_them_bit_for_bit(opts):
    c = apc.case("rooms_with_windows", 12, 3, 2, 5)
    results = []
    for how in ("plain", "empty", "null"):
        state = c["st"].copy()
        with HeatBatch(c["md"], **opts) as b:
            b.upload_state(state)
            if how == "plain":
                trace, failed, applied, modes = b.march_series(c["w"], 3, loads=c["loads"], **kwargs(c))
            elif how == "empty":
                trace, failed, applied, modes, air = b.march_series(c["w"], 3, loads=c["loads"], air={}, **kwargs(c))
                assert air["path_q"].shape == (12, 0) and len(air["state"]) == 0
            else:  # air == NULL through the C ABI
                s, keep = binding.make_series(c["w"], 3, **kwargs(c))
                l, lkeep = binding.make_zone_loads(**c["loads"])
                trace, applied, f = np.zeros((12, len(c["probes"]))), np.zeros((12, l.n_thermostats)), binding.C.c_int32(7)
                rc = b._L.heat_batch_march_series_air(b._h, binding.C.byref(s), None, None, binding.C.byref(l), None, None, None,
                                                      trace.ctypes.data_as(binding._dp), applied.ctypes.data_as(binding._dp), None, None,
                                                      None, binding.C.byref(f))
                assert rc == 0
                failed, modes = f.value, lkeep["th_mode"]
            b.download_state(state)
        assert failed == -1
        results.append((trace, applied, modes, state))
    for other in results[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(results[0], other))


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_an_array_that_is_not_asked_for_changes_no_bit_of_the_others(opts):
    c = apc.case("ragged_mixed", N_STEPS, 2, 2, apc.SEED)
    trace, applied, modes, full, state = series(c, opts)
    for stats, want_q in ((("sum_q",), False), (("steps_open",), False), (("switches",), False), ((), True), ((), False)):
        t, a, m, got, st = series(c, opts, air=dict(c["air"], stats=stats), path_q=want_q)
        assert set(got) == {"path_q", "state"} | set(stats)
        assert got["path_q"].shape == ((N_STEPS if want_q else 0), len(c["air"]["target"]))
        for key in got:
            if got[key].size:
                assert np.array_equal(got[key], full[key]), (stats, key)
        assert np.array_equal(t, trace) and np.array_equal(a, applied) and np.array_equal(m, modes) and np.array_equal(st, state)
    # state == NULL through the C ABI: every controlled path starts closed, nothing is returned — the same series
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(c["st"].copy())
        s, keep = binding.make_series(c["w"], 2, **kwargs(c))
        l, lkeep = binding.make_zone_loads(**c["loads"])
        a, akeep = binding.make_air_paths(**c["air"])
        a.state = None
        t, q, f = np.zeros_like(trace), np.zeros_like(full["path_q"]), binding.C.c_int32(7)
        rc = b._L.heat_batch_march_series_air(b._h, binding.C.byref(s), None, None, binding.C.byref(l), binding.C.byref(a), None, None,
                                              t.ctypes.data_as(binding._dp), None, None, None, q.ctypes.data_as(binding._dp), binding.C.byref(f))
    assert rc == 0 and f.value == -1
    assert np.array_equal(t, trace) and np.array_equal(q, full["path_q"]) and np.array_equal(akeep["sum_q"], full["sum_q"])
    assert not akeep["state"].any()  # (not written)


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_a_plain_series_after_one_with_air_paths_is_the_plain_series_of_a_fresh_batch(opts):
    c = apc.case("rooms_with_windows", 12, 2, 2, 9)
    fresh = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(fresh)
        want = b.march_series(c["w"], 2, **kwargs(c))
        b.download_state(fresh)
    after = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(c["st"].copy())
        b.march_series(c["w"], 2, loads=c["loads"], air=c["air"], **kwargs(c))
        b.upload_state(after)
        got = b.march_series(c["w"], 2, **kwargs(c))
        b.download_state(after)
    assert np.array_equal(want[0], got[0]) and want[1] == got[1] == -1 and np.array_equal(fresh, after)


def test_a_series_of_no_sub_timestep_still_evaluates_the_paths():
    c = apc.case("ragged_mixed", 6, 1, 2, 21)
    # nothing marches: every step sees the zone temperatures of the start
    ref = apc.loop_with_rules(lambda s, wk, za, zb: None, dict(c, n_steps=6), c["st"].copy())
    state = c["st"].copy()
    with HeatBatch(c["md"]) as b:
        b.upload_state(state)
        trace, failed, applied, modes, got = b.march_series(None, 0, n_steps=6, loads=c["loads"], air=c["air"], **kwargs(c))
        b.download_state(state)
    assert failed == -1 and np.array_equal(state, c["st"])
    assert (ref["path_q"] != 0).any() and np.array_equal(ref["path_q"], got["path_q"])
    for key in DISCRETE + ("sum_q",):
        assert np.array_equal(ref[key], got[key]), key


# ---- 7. NaN ----
def test_a_nan_volume_on_an_open_path_is_reported_as_the_zone_failure():
    """A NaN volume makes the path's m NaN, and with it the target's a0 and b0; the zone update itself would hide that
    (model.rs:662-668), so the paths report it as the zone loads do: HEAT_N_NAN_ZONE, at the step whose row holds the NaN."""
    md, st = mdl.clustered_massive(700, Z=28, dt=45.0, seed=3)
    n_steps, j = 9, 5
    channel = np.tile([0.02, 0.01], (n_steps, 1))
    channel[j, 0] = np.nan
    air = dict(target=[13, 2], source=[7, 3], volume_chan=[0, 1])
    for opts, n_sub in [(o, n) for o in OPTIONS for n in (0, 2)]:
        w = mdl.weather_series(n_steps * n_sub, 45.0).reshape(n_steps, n_sub, 3) if n_sub else None
        with HeatBatch(md, **opts) as b:
            b.upload_state(st.copy())
            with pytest.raises(HeatError) as e:
                b.march_series(w, n_sub, air=air, channel=channel, probes=md["zone_slot"], n_steps=n_steps)
            assert e.value.failed_step == j and e.value.code == 3, str(e.value)   # HEAT_N_NAN_ZONE
            assert b.failed_surface() == (13, 3) and "zone 13" in str(e.value)
            assert np.all(np.isfinite(e.value.trace[:j]))
            # the process and the batch survive: a healthy series afterwards
            b.upload_state(st.copy())
            trace, failed, got = b.march_series(w, n_sub, air=air, channel=np.tile([0.02, 0.01], (n_steps, 1)), probes=md["zone_slot"],
                                                n_steps=n_steps)
            assert failed == -1 and np.all(np.isfinite(trace)) and np.all(got["steps_open"] == n_steps)
    # on a CLOSED path the NaN volume reaches nothing: a cooling vent far below its setpoint
    closed = dict(air, open_chan=[2, -1], sense=[1, 1], band=[0.5, 0.0], min_delta=[0.0, 0.0])
    channel3 = np.concatenate([channel, np.full((n_steps, 1), 1000.0)], axis=1)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, got = b.march_series(mdl.weather_series(n_steps * 2, 45.0).reshape(n_steps, 2, 3), 2, air=closed, channel=channel3,
                                            probes=md["zone_slot"])
    assert failed == -1 and np.all(np.isfinite(trace)) and not got["path_q"][:, 0].any() and got["steps_open"][0] == 0


# ---- 8. one physical sanity check ----
def test_a_doorway_brings_two_rooms_closer():
    md, st = mdl.partitioned_buildings(960, 12, seed=8)
    n_steps, n_sub = 40, 2
    a, b_ = 1, 0                                                     # two rooms of the first building, joined by a partition
    assert (((md["front_zone"] == a) & (md["back_zone"] == b_)) | ((md["front_zone"] == b_) & (md["back_zone"] == a))).any()
    channel = np.tile([800.0, 0.15], (n_steps, 1))                   # a heater of 800 W in room a; 0.15 m3/s through the door
    # (the CPU oracle with the two rules gives 2.83 K between the rooms without the doorway and 1.99 K with it)
    loads = dict(gains=dict(zone=[a], chan=[0]))
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    probes = md["zone_slot"][[a, b_]]
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        closed, failed, _, _ = b.march_series(w, n_sub, loads=loads, channel=channel, probes=probes)
        b.upload_state(st.copy())
        opened, failed2, _, _, got = b.march_series(w, n_sub, loads=loads, air=air_paths.doorway(a, b_, 1), channel=channel, probes=probes)
    assert failed == -1 and failed2 == -1
    gap_closed, gap_open = closed[-1, 0] - closed[-1, 1], opened[-1, 0] - opened[-1, 1]
    print("room a - room b after %d steps: %.3f K without the doorway, %.3f K with it; sum_q %s" % (n_steps, gap_closed, gap_open, got["sum_q"]))
    assert gap_closed > 1.0 and 0.0 < gap_open < gap_closed - 0.3
    assert got["sum_q"][0] > 0.0 > got["sum_q"][1]                   # a -> b warms b, b -> a cools a
    assert np.all(got["steps_open"] == n_steps) and not got["switches"].any() and not got["state"].any()


# ---- refusals ----
def test_bad_paths_and_sharded_batches_are_refused_by_the_march():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    w, channel = np.zeros((2, 1, 3)), np.zeros((2, 2))
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        for bad, code, needle in ((dict(target=[0, 8], source=[1, 0], volume_chan=[0, 0]), -4, "air path 1:"),
                                  (dict(target=[0, 3], source=[1, 3], volume_chan=[0, 0]), -1, "air path 1:"),
                                  (dict(target=[0], source=[-1], volume_chan=[0]), -4, "air path 0:"),
                                  (dict(target=[0], source=[1], volume_chan=[0], open_chan=[1], sense=[0], band=[0.1], min_delta=[0.0]), -1,
                                   "air path 0:")):
            with pytest.raises(HeatError) as e:
                b.march_series(w, 1, channel=channel, air=bad)
            assert e.value.code == code and needle in str(e.value), str(e.value)
        got = st.copy()
        b.download_state(got)
        assert np.array_equal(got, st)
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, 1, channel=channel, air=dict(target=[0], source=[1], volume_chan=[0]))
        assert e.value.code == -1 and "sharded" in str(e.value)
