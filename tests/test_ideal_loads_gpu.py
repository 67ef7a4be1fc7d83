"""Ideal loads of a series on the GPU (include/heat_amd.h, heat_ideal_loads / heat_batch_march_series_ideal): in every
sub-timestep a zone receives exactly the power that brings it to its setpoint, limited by a capacity.

The expected result is DEFINED by tests/ideal_loads_ref.py: OracleModel.iterate_surfaces, OracleModel.zones_abc and the
header's rule in plain Python, per sub-timestep. State and trace are compared at the project's rtol = atol = 1e-9. The
powers are differences of large terms, so they are compared on the scale of those terms:
|dq| <= 1e-9 * n_sub * S with S = |a| + |b| (|setpoint| + |tc|) / D from the reference's own values. The saturation counts
are compared exactly, after asserting that the reference never has `need` within 1e-9 S of a capacity. What the rule makes
exact is tested exactly: the setpoint itself, cut and resume, repeatability, the accumulators against the returned rows."""
import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, binding, modeldict as mdl
from ideal_loads_ref import accumulate, cpu_series
from test_series_gpu import MODELS, assert_close, owned_slots, probes_of_every_kind, random_drives, series_kwargs, zone_terms, _id
from test_series_report_gpu import Q_KEYS, TH_KEYS, assert_same, modes_of, random_groups, replay, replay_thermostats
from test_zone_loads_gpu import closed_form_zone, host_rule, random_loads, start_modes

pytestmark = pytest.mark.gpu

OPTIONS = [dict(), dict(use_graph=True), dict(no_fusion=True)]
ACC = ("sum_heating", "sum_cooling", "peak_heating", "step_peak_heating", "peak_cooling", "step_peak_cooling")
SAT = ("n_sat_heating", "n_sat_cooling")


def ideal_case(model, n_steps, n_sub, seed, caps="mixed"):
    """Model, drives, zone terms and the zone loads of test_zone_loads_gpu (a gain, flows and dead-band thermostats on most
    zones), plus ideal loads on three zones in four, in shuffled order: heating only, cooling only and both; setpoints around
    the zones' temperatures with a night set-back (a step change half way); capacities small enough to saturate in part of
    the sub-timesteps, and unlimited ones."""
    md, st = MODELS[model]()
    rng = np.random.default_rng(seed)
    channel, drives = random_drives(md, rng, n_steps)
    a0, b0 = zone_terms(md, rng, n_steps, 2)
    channel, loads = random_loads(md, st, rng, n_steps, channel)
    Z = int(md["n_zones"])
    t_mid = float(np.median(st[md["zone_slot"]]))
    c0 = channel.shape[1]
    night = np.arange(n_steps) >= n_steps // 2
    # (the zones of these models float up to 30-60 C under their gains: one heating setpoint just around the start
    # temperatures, rarely reached from below, and one far above, which heats most zones; one cooling setpoint 1 K above
    # the first heating one, which cools nearly always, and one high up that only the hot zones reach)
    heat_sp = np.stack([np.where(night, t_mid - 1.5, t_mid + 0.7), np.where(night, t_mid + 14.0, t_mid + 24.0)], axis=1)
    cool_sp = np.stack([heat_sp[:, 0] + 1.0, np.where(night, t_mid + 18.0, t_mid + 30.0)], axis=1)
    channel = np.concatenate([channel, heat_sp, cool_sp], axis=1)
    zone = rng.permutation(np.flatnonzero(np.arange(Z) % 4 != 3)).astype(np.int32)
    n = len(zone)
    kind = np.arange(n) % 3                                      # heating only, cooling only, both
    pick = (np.arange(n) // 3) % 2                               # both setpoint channels of either kind in every model
    heat_chan = np.where(kind != 1, c0 + pick, -1).astype(np.int32)
    # (a load with both setpoints takes the cooling setpoint above its heating one)
    cool_chan = np.where(kind == 1, c0 + 2 + pick, np.where(kind == 2, c0 + 2, -1)).astype(np.int32)
    heat_chan[kind == 2] = c0
    ideal = dict(zone=zone, heat_chan=heat_chan, cool_chan=cool_chan)
    if caps == "mixed":
        # (the powers these zones need span 1e2 .. 1e6 W: capacities spread over that range saturate in part of the run)
        ideal["heat_cap"] = np.where(np.arange(n) % 4 < 2, 10.0 ** rng.uniform(2.0, 5.0, n), np.inf)
        ideal["cool_cap"] = np.where((np.arange(n) + 3) % 4 < 2, 10.0 ** rng.uniform(2.5, 5.5, n), np.inf)
    elif caps == "zero":
        ideal["heat_cap"], ideal["cool_cap"] = np.zeros(n), np.zeros(n)
    probes = np.unique(np.concatenate([probes_of_every_kind(md, rng), md["zone_slot"]])).astype(np.int64)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    return md, st, channel, drives, probes, a0, b0, loads, ideal, w


def run(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts=None, steps=slice(None), state=None, **more):
    """One ideal series on a fresh batch (or on `state`). Returns (result dict, downloaded state)."""
    got = st.copy() if state is None else state.copy()
    with HeatBatch(md, **(opts or {})) as b:
        b.upload_state(got)
        out = b.march_series(w[steps], n_sub, loads=loads, ideal=ideal, **dict(series_kwargs(channel, drives, probes, a0, b0, steps=steps), **more))
        b.download_state(got)
    assert out["failed_step"] == -1
    return out, got


# ---- 1. against the CPU reference ----
_REF = {}


def reference(oracle, model, n_steps, n_sub):
    key = (model, n_steps, n_sub)
    if key not in _REF:
        md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case(model, n_steps, n_sub, 300 + n_sub)
        ref = st.copy()
        _REF[key] = (cpu_series(oracle, md, ref, w, n_sub, channel, drives, probes, loads, ideal, a0, b0), ref)
    return _REF[key]


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("n_sub,n_steps", [(1, 24), (2, 24), (20, 8)])
@pytest.mark.parametrize("model", ["ragged_mixed", "rooms_with_windows", "partitioned_buildings"])
def test_ideal_series_matches_the_cpu_reference(oracle, model, n_sub, n_steps, opts):
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case(model, n_steps, n_sub, 300 + n_sub)
    ref, ref_state = reference(oracle, model, n_steps, n_sub)
    N = len(ideal["zone"])
    print("%s n_sub=%d: %d loads; reference sub-timesteps heating %d, cooling %d, floating %d; saturated %d + %d; smallest "
          "|need - cap| / S = %.3g" % (model, n_sub, N, ref["n_heat"], ref["n_cool"], ref["n_free"], ref["n_sat_heating"].sum(),
                                       ref["n_sat_cooling"].sum(), ref["margin"]))
    # the inputs exercise every branch, and no sub-timestep of the reference sits near a capacity
    assert ref["n_heat"] > 0 and ref["n_cool"] > 0 and ref["n_free"] > 0
    assert 0 < ref["n_sat_heating"].sum() < ref["n_heat"] and 0 < ref["n_sat_cooling"].sum() < ref["n_cool"]
    assert (ref["applied"] != 0).any()
    assert ref["margin"] > 1e-7                           # (a hundred times the 1e-9 S the counts could depend on)
    out, got = run(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts)
    assert_close(ref["trace"], out["trace"], "%s n_sub=%d trace" % (model, n_sub))
    own = owned_slots(md)
    assert_close(ref_state[own], got[own], "%s n_sub=%d final state" % (model, n_sub))
    assert_close(ref["applied"], out["applied"], "%s n_sub=%d applied" % (model, n_sub))
    assert np.array_equal(ref["modes"], out["modes"])
    dq = np.abs(out["ideal_q"] - ref["ideal_q"]) / ref["scale"]
    print("%s n_sub=%d ideal_q: worst |dq| / S = %.3e (bound %.1e)" % (model, n_sub, dq.max(), 1e-9 * n_sub))
    assert np.all(np.isfinite(out["ideal_q"])) and dq.max() <= 1e-9 * n_sub
    for k in SAT:
        assert np.array_equal(ref[k], out["ideal"][k]), k


# ---- 2. exact properties ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("n_sub", [1, 3])
def test_unlimited_loads_on_one_constant_channel_hold_it_bit_for_bit(n_sub, opts):
    n_steps = 12
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case("rooms_with_windows", n_steps, n_sub, 21, caps="none")
    sp = float(np.median(st[md["zone_slot"]])) + 0.3217
    channel = np.concatenate([channel, np.full((n_steps, 1), sp)], axis=1)
    c = channel.shape[1] - 1
    zone = ideal["zone"]
    ideal = dict(zone=zone, heat_chan=np.full(len(zone), c), cool_chan=np.full(len(zone), c))
    out, got = run(md, st, w, n_sub, channel, drives, md["zone_slot"], a0, b0, loads, ideal, opts)
    assert np.array_equal(out["trace"][:, zone], np.full((n_steps, len(zone)), sp))
    assert (out["ideal_q"] != 0).any() and not out["ideal"]["n_sat_heating"].any() and not out["ideal"]["n_sat_cooling"].any()
    others = np.setdiff1d(np.arange(md["n_zones"]), zone)
    assert (out["trace"][:, others] != sp).all()


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model", ["ragged_mixed", "partitioned_buildings"])
def test_a_series_cut_and_resumed_gives_the_bits_of_the_whole(model, opts):
    n_steps, n_sub = 20, 3
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case(model, n_steps, n_sub, 33)
    whole, whole_state = run(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts)
    again, again_state = run(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts)
    for k in ("trace", "ideal_q", "applied", "modes"):
        assert np.array_equal(whole[k], again[k]), k                       # two runs, the same bits
    assert_same(whole["ideal"], again["ideal"], ACC + SAT, "repeat")
    assert np.array_equal(whole_state, again_state)
    cut = int(np.random.default_rng(5).integers(3, n_steps - 3))
    got = st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(got)
        kw = lambda steps: series_kwargs(channel, drives, probes, a0, b0, steps=steps)
        first = b.march_series(w[:cut], n_sub, loads=loads, ideal=ideal, **kw(slice(0, cut)))
        loads2 = dict(loads, thermostats=dict(loads["thermostats"], mode=first["modes"]))
        second = b.march_series(w[cut:], n_sub, loads=loads2, ideal=dict(ideal, resume=first["ideal"], step_base=cut), **kw(slice(cut, None)))
        b.download_state(got)
    assert first["failed_step"] == -1 and second["failed_step"] == -1
    for k in ("trace", "ideal_q", "applied"):
        assert np.array_equal(whole[k], np.concatenate([first[k], second[k]])), k
    assert np.array_equal(whole["modes"], second["modes"])
    assert_same(whole["ideal"], second["ideal"], ACC + SAT, "cut at %d" % cut)
    assert np.array_equal(whole_state, got)
    assert (whole["ideal"]["step_peak_heating"] >= cut).any() or (whole["ideal"]["step_peak_cooling"] >= cut).any()


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_no_sub_timesteps_give_zero_rows_and_an_unchanged_state(opts):
    n_steps = 5
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case("ragged_mixed", n_steps, 1, 44)
    got = st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(got)
        out = b.march_series(np.zeros((0, 3)), 0, loads=loads, ideal=ideal, n_steps=n_steps, **series_kwargs(channel, drives, probes, a0, b0))
        b.download_state(got)
    own = owned_slots(md)
    assert out["failed_step"] == -1 and out["ideal_q"].shape == (n_steps, len(ideal["zone"])) and not out["ideal_q"].any()
    assert np.array_equal(got[own], st[own])
    assert np.array_equal(out["trace"], np.tile(st[probes], (n_steps, 1)))
    assert_same(accumulate(out["ideal_q"]), out["ideal"], ACC, "n_sub = 0")
    assert (out["ideal"]["peak_heating"] == 0.0).all() and (out["ideal"]["step_peak_heating"] == 0).all()


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_a_load_that_never_acts_leaves_everything_as_initialised(opts):
    n_steps, n_sub = 6, 2
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case("ragged_mixed", n_steps, n_sub, 45)
    channel = np.concatenate([channel, np.full((n_steps, 1), -200.0), np.full((n_steps, 1), 300.0)], axis=1)
    c = channel.shape[1]
    n = len(ideal["zone"])
    far = dict(zone=ideal["zone"], heat_chan=np.full(n, c - 2), cool_chan=np.full(n, c - 1))
    out, got = run(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, far, opts)
    assert not out["ideal_q"].any() and not out["ideal"]["n_sat_heating"].any() and not out["ideal"]["n_sat_cooling"].any()
    # peaks: a q-sum of 0.0 enters at step 0 (0 > -inf, 0 < +inf), the sums stay 0
    assert_same(accumulate(out["ideal_q"]), out["ideal"], ACC, "never acts")
    assert not out["ideal"]["sum_heating"].any() and not out["ideal"]["sum_cooling"].any()
    # ... and the march is the one without ideal loads, streamed (the two zone kernels contract differently: 1e-10)
    with HeatBatch(md, no_fusion=True) as b:
        b.upload_state(st.copy())
        trace, failed, applied, modes = b.march_series(w, n_sub, loads=loads, **series_kwargs(channel, drives, probes, a0, b0))
    np.testing.assert_allclose(out["trace"], trace, rtol=1e-10, atol=1e-10)


# ---- 3. against the existing path; the rest of the series on an ideal run ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model", ["ragged_mixed", "rooms_with_windows"])
def test_capacities_of_zero_are_the_streamed_series_and_the_report_replays(model, opts):
    n_steps, n_sub = 16, 3
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case(model, n_steps, n_sub, 51, caps="zero")
    rng = np.random.default_rng(9)
    groups = random_groups(md, rng, (5, 0, 300, 1100))
    P = len(probes)
    kw = series_kwargs(channel, drives, probes, a0, b0)
    with HeatBatch(md, no_fusion=True) as b:
        ref = st.copy()
        b.upload_state(ref)
        trace, failed, applied, modes = b.march_series(w, n_sub, loads=loads, **kw)
        b.download_state(ref)
    assert failed == -1
    lo, hi = trace.min(axis=0) + 0.3 * np.ptp(trace, axis=0), trace.min(axis=0) + 0.7 * np.ptp(trace, axis=0)
    lo, hi = np.concatenate([lo, np.full(len(groups), np.nan)]), np.concatenate([hi, np.full(len(groups), np.nan)])
    report = dict(stats=binding.Q_STATS, thermostat_stats=binding.TH_STATS, group_trace=True, groups=groups, limits=dict(lo=lo, hi=hi))
    out, got = run(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, ideal, opts, report=report)
    assert not out["ideal_q"].any()
    own = owned_slots(md)
    np.testing.assert_allclose(out["trace"], trace, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(got[own], ref[own], rtol=1e-10, atol=1e-10)
    # applied, modes and every report array: the rules replayed over THIS run's trace, bit for bit
    zt = {int(s): i for i, s in enumerate(probes)}
    zcol = np.array([zt[int(s)] for s in md["zone_slot"]])
    T = np.concatenate([st[md["zone_slot"]][None], out["trace"][:-1, zcol]])
    m = start_modes(loads)
    want_applied = np.array([host_rule(T[k], channel[k], a0[k], b0[k], loads, m)[2] for k in range(n_steps)])
    assert np.array_equal(want_applied, out["applied"]) and np.array_equal(m, out["modes"])
    rep = out["report"]
    assert_same(replay(np.concatenate([out["trace"], rep["group_trace"]], axis=1), lo, hi), rep, Q_KEYS, model)
    assert_same(replay_thermostats(out["applied"], start_modes(loads)), rep, TH_KEYS, model)
    assert (rep["q_n_below"][:P] > 0).any() and (rep["th_switches"] > 0).any()


def test_without_ideal_loads_the_call_is_the_report_series():
    n_steps, n_sub = 10, 2
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case("rooms_with_windows", n_steps, n_sub, 52)
    groups = random_groups(md, np.random.default_rng(3), (7, 200))
    Q = len(probes) + len(groups)
    t_mid = float(np.median(st[md["zone_slot"]]))
    report = dict(stats=binding.Q_STATS, thermostat_stats=binding.TH_STATS, group_trace=True, groups=groups,
                  limits=dict(lo=np.full(Q, t_mid), hi=np.full(Q, t_mid + 2.0)))
    kw = series_kwargs(channel, drives, probes, a0, b0)
    with HeatBatch(md) as b:
        ref = st.copy()
        b.upload_state(ref)
        trace, failed, applied, modes, rep = b.march_series(w, n_sub, loads=loads, report=report, **kw)
        b.download_state(ref)
        fused = b.n_fused_launches
    for none in (dict(), None):
        got = st.copy()
        with HeatBatch(md) as b:
            b.upload_state(got)
            if none is None:   # il == NULL through the raw entry point
                s, keep = binding.make_series(w, n_sub, **kw)
                l, lkeep = binding.make_zone_loads(**loads)
                r, rkeep = binding.make_report(n_probes=s.n_probes, n_thermostats=l.n_thermostats, n_steps=s.n_steps, **report)
                import ctypes as C
                t2, a2, f2 = np.zeros_like(trace), np.zeros_like(applied), C.c_int32(7)
                dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
                assert b._L.heat_batch_march_series_ideal(b._h, C.byref(s), C.byref(l), None, C.byref(r), dp(t2), dp(a2), None, C.byref(f2)) == 0
                out = dict(trace=t2, applied=a2, modes=lkeep["th_mode"], report=rkeep, failed_step=f2.value)
            else:
                out = b.march_series(w, n_sub, loads=loads, report=report, ideal=none, **kw)
            b.download_state(got)
            assert b.n_fused_launches == fused                           # the same launches: the cluster-resident march
        assert out["failed_step"] == -1
        assert np.array_equal(trace, out["trace"]) and np.array_equal(applied, out["applied"]) and np.array_equal(modes, out["modes"])
        assert_same(rep, out["report"], Q_KEYS + TH_KEYS + ("group_trace",), "no ideal loads")
        assert np.array_equal(ref, got)


# ---- 4. the accumulators against the returned rows ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_accumulators_equal_a_plain_loop_over_the_returned_rows(opts):
    n_steps, n_sub = 30, 2
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case("rooms_with_windows", n_steps, n_sub, 61)
    out, got = run(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, dict(ideal, step_base=1000), opts)
    acc = out["ideal"]
    assert_same(accumulate(out["ideal_q"], step_base=1000), acc, ACC, "accumulators")
    assert (acc["sum_heating"] > 0).any() and (acc["sum_cooling"] < 0).any()
    assert (acc["step_peak_heating"] > 1000).any() and (acc["step_peak_cooling"] > 1000).any()
    assert (acc["n_sat_heating"] > 0).any() and (acc["n_sat_cooling"] > 0).any()
    # a subset of the accumulators costs nothing else
    some, _ = run(md, st, w, n_sub, channel, drives, probes, a0, b0, loads, dict(ideal, step_base=1000, stats=("sum_heating", "peak_cooling")), opts)
    assert sorted(some["ideal"]) == ["peak_cooling", "sum_heating"]
    assert np.array_equal(some["ideal"]["sum_heating"], acc["sum_heating"]) and np.array_equal(some["ideal"]["peak_cooling"], acc["peak_cooling"])
    assert np.array_equal(some["ideal_q"], out["ideal_q"]) and np.array_equal(some["trace"], out["trace"])


# ---- 5. the physics: once the zone sits on h, q = b h - a ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_the_power_that_holds_a_room_is_its_heat_loss(oracle, opts):
    md, st, n_sub = closed_form_zone(oracle)
    steps, h, t_out, gain = 400, 21.0, 3.0, 35.0
    channel = np.tile([h, gain], (steps, 1))
    loads = dict(gains=dict(zone=[0], chan=[1]))
    w = np.tile([t_out, 0.0, 0.0], (steps, n_sub, 1))
    got = st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(got)
        out = b.march_series(w, n_sub, loads=loads, ideal=dict(zone=[0], heat_chan=[0]), channel=channel, probes=md["zone_slot"])
        b.download_state(got)
    # (the room starts above h and floats down to it in a few steps; from then on it sits on h)
    assert out["failed_step"] == -1 and np.all(out["trace"][50:, 0] == h) and np.all(out["ideal_q"][50:, 0] > 0)
    S, area = int(md["n_surfaces"]), md["area"]
    first = md["first_node_slot"]
    last = first + np.diff(md["node_offset"]) - 1
    loss, b_sum = 0.0, 0.0
    for s in range(S):
        for kind, zslot, hs, face in ((md["front_kind"][s], md["front_zone"][s], md["hs_front_slot"][s], first[s]),
                                      (md["back_kind"][s], md["back_zone"][s], md["hs_back_slot"][s], last[s])):
            if kind == mdl.SPACE and zslot == 0:
                loss += got[hs] * area[s] * (h - got[face])
                b_sum += got[hs] * area[s]
    want = loss - gain                                  # + b0 h - a0 with b0 = 0, a0 = the gain
    E = np.exp(-b_sum * md["dt"] / (md["zone_volume"][0] * 101325. * 28.97 / (8314.46261815324 * (h + 273.15)) * (1002.7370 + 1.2324e-2 * (h + 273.15))))
    scale = abs(loss - b_sum * h) + gain + b_sum * 2 * abs(h) / (1.0 - E)
    mean = out["ideal_q"][-1, 0] / n_sub
    print("holding %.1f C against %.1f C: %.6f W per sub-timestep, heat loss %.6f W, scale %.3g" % (h, t_out, mean, want, scale))
    assert want > 0 and abs(mean - want) <= 1e-9 * scale


# ---- 6. failures ----
def test_a_nan_capacity_is_refused_and_a_nan_gain_is_reported_with_its_zone_and_step():
    # (one sub-timestep per step: the step that fails ends with the zone's own flag alone; in a second sub-timestep the
    # surfaces facing the NaN zone would add theirs, and a NaN coefficient outranks a NaN zone in the return code)
    n_steps, n_sub = 8, 1
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case("ragged_mixed", n_steps, n_sub, 71)
    kw = series_kwargs(channel, drives, probes, a0, b0)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        bad = dict(ideal, heat_cap=np.where(np.arange(len(ideal["zone"])) == 2, np.nan, ideal["heat_cap"]))
        with pytest.raises(HeatError) as e:
            b.march_series(w, n_sub, loads=loads, ideal=bad, **kw)
        assert e.value.code == -1 and "ideal load 2" in str(e.value)
        # a NaN in the gain channel of an ideal zone at step 5
        z = int(ideal["zone"][0])
        ch = np.concatenate([channel, np.zeros((n_steps, 1))], axis=1)
        ch[5, -1] = np.nan
        g = loads["gains"]
        gains = dict(zone=np.append(g["zone"], z), chan=np.append(g["chan"], ch.shape[1] - 1), factor=np.append(g["factor"], 1.0))
        with pytest.raises(HeatError) as e:
            b.march_series(w, n_sub, loads=dict(loads, gains=gains), ideal=ideal, **dict(kw, channel=ch))
        assert e.value.code == 3 and e.value.failed_step == 5                 # HEAT_N_NAN_ZONE
        assert b.failed_surface() == (z, 3)


# ---- 7. nothing of an ideal series stays on the batch ----
@pytest.mark.parametrize("opts", [dict(), dict(use_graph=True)], ids=_id)
def test_a_plain_series_after_an_ideal_one_is_the_plain_series_of_a_fresh_batch(opts):
    n_steps, n_sub = 8, 3
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case("partitioned_buildings", n_steps, n_sub, 81)
    kw = series_kwargs(channel, drives, probes, a0, b0)
    with HeatBatch(md, **opts) as b:
        assert b.n_fused_surfaces > 0
        ref = st.copy()
        b.upload_state(ref)
        trace, failed = b.march_series(w, n_sub, **kw)
        b.download_state(ref)
        fused = b.n_fused_launches
        assert fused > 0
    with HeatBatch(md, **opts) as b:
        b.upload_state(st.copy())
        out = b.march_series(w, n_sub, loads=loads, ideal=ideal, **kw)
        assert out["failed_step"] == -1 and b.n_fused_launches == 0           # the ideal body is streamed
        got = st.copy()
        b.upload_state(got)
        trace2, failed2 = b.march_series(w, n_sub, **kw)
        b.download_state(got)
        assert b.n_fused_launches == fused
    assert failed == -1 and failed2 == -1
    assert np.array_equal(trace, trace2) and np.array_equal(ref, got)
