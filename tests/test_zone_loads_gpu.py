"""Zone loads of a series on the GPU (include/heat_amd.h, heat_batch_march_series_loads): gains, air flows and thermostats
formed on the device at every step of a series.

The expected result is DEFINED by `host_rule` below — the contract of the header in numpy, one rounded operation per
product and sum — applied between per-step march calls to the zone temperatures the call before returned: through
heat_batch_march_ex the series must agree bit for bit, through OracleModel.march (≙ ThermalModel::march,
src/model.rs:359-427) at rtol = atol = 1e-9. The gain and flow terms are the reference's (model.rs:500-544, gas.rs:49,
165-179); the thermostat is this project's own (the reference has no controller)."""
import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, binding, modeldict as mdl
from test_series_gpu import (MODELS, assert_close, owned_slots, probes_of_every_kind, random_drives, series_kwargs, term_row,
                             write_inputs, zone_terms, _id)

pytestmark = pytest.mark.gpu

OPTIONS = [dict(), dict(use_graph=True), dict(no_fusion=True)]


def host_rule(T, row, a0, b0, loads, modes):
    """Step 1-4 of the contract: returns (a0, b0, applied); `modes` is updated in place. T: the zone temperatures at the start
    of the step; row: the step's channel row; a0 / b0: the series' own zone-term row (or None). np.add.at adds unbuffered,
    in the order of its index array: per zone the caller's order, gains, then flows, then thermostats."""
    Z = len(T)
    a0 = np.zeros(Z) if a0 is None else np.array(a0, dtype=np.float64)
    b0 = np.zeros(Z) if b0 is None else np.array(b0, dtype=np.float64)
    g = loads.get("gains")
    if g is not None:
        factor = g.get("factor")
        p = row[g["chan"]] if factor is None else factor * row[g["chan"]]
        np.add.at(a0, g["zone"], p)
    f = loads.get("flows")
    if f is not None:
        gain = f.get("volume_gain")
        v = row[f["volume_chan"]] if gain is None else gain * row[f["volume_chan"]]
        t_in = row[f["temp_chan"]]
        tk = t_in + 273.15
        rho = 101325. * 28.97 / (8314.46261815324 * tk)
        cp = 1002.7370 + 1.2324e-2 * tk
        m = (rho * v) * cp
        np.add.at(a0, f["zone"], m * t_in)
        np.add.at(b0, f["zone"], m)
    th = loads.get("thermostats")
    applied = np.zeros(0)
    if th is not None:
        ts, d = T[th["sensor_zone"]], th["band"] / 2.0
        hc, cc = th["heat_chan"], th["cool_chan"]
        h, c = row[np.maximum(hc, 0)], row[np.maximum(cc, 0)]
        on = (hc >= 0) & (ts < h - d)
        off = (hc >= 0) & ~on & (modes == 1) & (ts > h + d)
        modes[on], modes[off] = 1, 0
        may = (modes != 1) & (cc >= 0)
        on = may & (ts > c + d)
        off = may & ~on & (modes == 2) & (ts < c - d)
        modes[on], modes[off] = 2, 0
        applied = np.where(modes == 1, th["heat_power"], np.where(modes == 2, -th["cool_power"], 0.0))
        np.add.at(a0, th["target_zone"], applied)
    return a0, b0, applied


def n_thermostats(loads):
    return len(loads["thermostats"]["sensor_zone"]) if loads.get("thermostats") is not None else 0


def start_modes(loads):
    th = loads.get("thermostats")
    if th is None:
        return np.zeros(0, np.uint8)
    return np.zeros(n_thermostats(loads), np.uint8) if th.get("mode") is None else np.array(th["mode"], dtype=np.uint8)


def loop_with_host_rule(march, md, state, weather, channel, drives, probes, loads, a0=None, b0=None):
    """The definition: per step, the rule on the zone temperatures the state holds, the inputs written, one march call.
    march(state, weather of the step, a0, b0). Returns (trace, applied, modes)."""
    n_steps = len(channel)
    modes = start_modes(loads)
    trace, applied = np.zeros((n_steps, len(probes))), np.zeros((n_steps, n_thermostats(loads)))
    for k in range(n_steps):
        za, zb, applied[k] = host_rule(state[md["zone_slot"]], channel[k], term_row(a0, k), term_row(b0, k), loads, modes)
        write_inputs(md, state, k, channel, drives)
        march(state, weather[k], za, zb)
        trace[k] = state[probes]
    return trace, applied, modes


def random_loads(md, st, rng, n_steps, channel):
    """Appends the loads' channels to `channel` (gain powers, flow volumes and temperatures, heating and cooling setpoints
    around the zones' temperatures) and returns (channel, loads): about three gains and two flows per zone in shuffled
    order, a thermostat on two zones in three — every third of them sensing another zone — and a second thermostat on some
    targets."""
    Z = int(md["n_zones"])
    t_mid = float(np.median(st[md["zone_slot"]]))
    c0 = channel.shape[1]
    heat_sp = t_mid + rng.uniform(-0.4, 1.0, (n_steps, 2))
    # (one cooling setpoint above the heating ones, one below the zones' temperatures: that one cools from the start)
    cool_sp = np.stack([heat_sp[:, 0] + rng.uniform(0.8, 1.6, n_steps), t_mid - rng.uniform(0.0, 1.0, n_steps)], axis=1)
    extra = np.concatenate([rng.uniform(0.0, 300.0, (n_steps, 4)), rng.uniform(0.0, 0.05, (n_steps, 2)),
                            rng.uniform(-5.0, 35.0, (n_steps, 2)), heat_sp, cool_sp], axis=1)
    channel = np.concatenate([channel, extra], axis=1)
    ng, nf = 3 * Z, 2 * Z
    gains = dict(zone=rng.permutation(np.arange(ng) % Z).astype(np.int32), chan=(c0 + rng.integers(0, 4, ng)).astype(np.int32),
                 factor=rng.uniform(0.2, 1.5, ng))
    flows = dict(zone=rng.permutation(np.arange(nf) % Z).astype(np.int32), volume_chan=(c0 + 4 + rng.integers(0, 2, nf)).astype(np.int32),
                 temp_chan=(c0 + 6 + rng.integers(0, 2, nf)).astype(np.int32), volume_gain=rng.uniform(0.5, 1.5, nf))
    target = np.flatnonzero(np.arange(Z) % 3 != 2)
    target = np.concatenate([target, target[::4]])                   # two thermostats on one target
    target = rng.permutation(target).astype(np.int32)
    nt = len(target)
    sensor = np.where(np.arange(nt) % 3 == 0, (target + 1) % Z, target).astype(np.int32)
    kind = rng.integers(0, 3, nt)                                    # heating only, cooling only, both
    thermostats = dict(sensor_zone=sensor, target_zone=target,
                       heat_chan=np.where(kind != 1, c0 + 8 + rng.integers(0, 2, nt), -1).astype(np.int32),
                       cool_chan=np.where(kind != 0, c0 + 10 + rng.integers(0, 2, nt), -1).astype(np.int32),
                       heat_power=rng.uniform(200.0, 3000.0, nt), cool_power=rng.uniform(200.0, 3000.0, nt),
                       band=rng.uniform(0.0, 0.6, nt))
    return channel, dict(gains=gains, flows=flows, thermostats=thermostats)


def case(model, n_steps, n_sub, form, seed):
    md, st = MODELS[model]()
    rng = np.random.default_rng(seed)
    channel, drives = random_drives(md, rng, n_steps)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, n_steps, form)
    channel, loads = random_loads(md, st, rng, n_steps, channel)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    return md, st, channel, drives, probes, a0, b0, loads, w


def describe(what, applied):
    changes = int((np.diff((applied != 0).astype(int), axis=0) != 0).sum()) if len(applied) > 1 else 0
    print("%s: %d thermostats, %.0f %% of the step-thermostats acting, %d changes of acting" % (
        what, applied.shape[1], 100.0 * float((applied != 0).mean()) if applied.size else 0.0, changes))


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model", ["ragged_mixed", "rooms_with_windows", "partitioned_buildings_large"])
def test_series_with_loads_equals_the_per_call_path_bit_for_bit(model, opts):
    n_steps = 24
    for form, n_sub in enumerate((1, 2, 5)):
        md, st, channel, drives, probes, a0, b0, loads, w = case(model, n_steps, n_sub, form, 40 + n_sub)
        own = owned_slots(md)
        ref = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(ref)
            ref_trace, ref_applied, ref_modes = loop_with_host_rule(
                lambda s, wk, za, zb: b.march(s, wk, za, zb, outputs=b.OUT_ALL), md, ref, w, channel, drives, probes, loads, a0, b0)
        describe("%s n_sub=%d (per-call path)" % (model, n_sub), ref_applied)
        # the inputs exercise the controller: thermostats act, rest, and change between the two during the series
        assert (ref_applied > 0).any() and (ref_applied < 0).any() and (ref_applied == 0).any()
        assert (np.diff(ref_applied != 0, axis=0) != 0).any()
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(got)
            trace, failed, applied, modes = b.march_series(w, n_sub, loads=loads, **series_kwargs(channel, drives, probes, a0, b0))
            b.download_state(got)
        assert failed == -1
        assert np.array_equal(ref_applied, applied), "n_sub=%d: %d applied powers differ" % (n_sub, int((ref_applied != applied).sum()))
        assert np.array_equal(ref_modes, modes)
        assert np.array_equal(ref_trace, trace), "n_sub=%d: %d trace values differ, worst %.3e" % (
            n_sub, int((ref_trace != trace).sum()), np.abs(ref_trace - trace).max())
        assert np.array_equal(ref[own], got[own]), "n_sub=%d: %d state slots differ" % (n_sub, int((ref[own] != got[own]).sum()))


_ORACLE_LOOPS = {}


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model", ["ragged_mixed", "rooms_with_windows", "partitioned_buildings_large"])
def test_series_with_loads_matches_the_oracle_loop(oracle, model, opts):
    n_steps, n_sub = 24, 3
    md, st, channel, drives, probes, a0, b0, loads, w = case(model, n_steps, n_sub, 2, 77)
    if model not in _ORACLE_LOOPS:  # (the same for every option set)
        big = md["n_surfaces"] > 8192
        m = oracle.OracleModel(md)

        def march(s, wk, za, zb):
            assert m.march(s, wk, za, zb, threads=16 if big else 1)[0] == 0

        ref = st.copy()
        _ORACLE_LOOPS[model] = loop_with_host_rule(march, md, ref, w, channel, drives, probes, loads, a0, b0) + (ref,)
    ref_trace, ref_applied, ref_modes, ref = _ORACLE_LOOPS[model]
    describe("%s (oracle loop)" % model, ref_applied)
    assert (ref_applied > 0).any() and (ref_applied < 0).any() and (ref_applied == 0).any()
    got = st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(got)
        trace, failed, applied, modes = b.march_series(w, n_sub, loads=loads, **series_kwargs(channel, drives, probes, a0, b0))
        b.download_state(got)
    assert failed == -1
    assert_close(ref_trace, trace, "%s trace" % model)
    assert_close(ref_applied, applied, "%s applied" % model)
    assert np.array_equal(ref_modes, modes)
    own = owned_slots(md)
    assert_close(ref[own], got[own], "%s final state" % model)


CLOSED_FORM_LOADS = {
    # validate_wall_heat_transfer.rs:752-790; the power as a gain on a constant channel, 0.1 m3/s at 30 C as a flow
    "luminaire_on": dict(lighting_power=100.),
    "heater_on": dict(heating_power=100.),
    "heater_and_infiltration": dict(heating_power=10., infiltration_rate=0.1),
}


def closed_form_zone(oracle, **kw):
    """The closed-form zone of tests/test_energyplus_series.py (40 m3, 4 m2 no-mass wall, 20 steps per hour): model, initial
    state, sub-timesteps per step."""
    from test_energyplus_series import closed_form_case
    md, st, _, _ = closed_form_case(oracle, 20, 0, **kw)
    n_sub = int(round(180.0 / md["dt"]))
    assert abs(n_sub * md["dt"] - 180.0) < 1e-9
    return md, st, n_sub


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("name", sorted(CLOSED_FORM_LOADS))
def test_closed_form_zone_cases_through_loads(oracle, name, opts):
    """Bounds: those of tests/test_energyplus_series.py::test_closed_form_zone_solutions for the same cases (0.35 K
    throughout, 0.05 K at the end); the oracle there forms a0 / b0 from or_gas_density / or_gas_heat_capacity."""
    from test_energyplus_series import closed_form_case
    kw = CLOSED_FORM_LOADS[name]
    steps, t_out = 800, 30.0
    md, st, n_sub = closed_form_zone(oracle, **kw)
    _, ref_state, ref_found, exp = closed_form_case(oracle, 20, steps, **kw)   # (the zone BEFORE each of its marches)
    power = kw.get("heating_power", 0.0) + kw.get("lighting_power", 0.0)
    channel = np.tile([power, kw.get("infiltration_rate", 0.0), t_out], (steps, 1))
    loads = dict(gains=dict(zone=[0], chan=[0]))
    if kw.get("infiltration_rate", 0.0) > 0.0:
        loads["flows"] = dict(zone=[0], volume_chan=[1], temp_chan=[2])
    w = np.tile([t_out, 0.0, 0.0], (steps, n_sub, 1))
    zone = md["zone_slot"]
    with HeatBatch(md, **opts) as b:
        b.upload_state(st.copy())
        trace, failed, applied, modes = b.march_series(w, n_sub, loads=loads, channel=channel, probes=zone)
    assert failed == -1 and applied.shape == (steps, 0) and len(modes) == 0
    found = np.concatenate([st[zone], trace[:-1, 0]])
    err = np.abs(found - exp)
    print("%s: max |found - closed form| = %.4f C, final %.3f vs %.3f" % (name, err.max(), found[-1], exp[-1]))
    assert err.max() < 0.35
    assert abs(found[-1] - exp[-1]) < 0.05
    assert_close(ref_found, found, "%s zone against the oracle with or_gas_* terms" % name)
    assert_close(ref_state[zone], trace[-1], "%s zone after the last step" % name)


CYCLING = {
    # name: (outdoor C, thermostat). The CPU oracle with host_rule gives 119 / 167 mode changes and zone ranges of
    # 19.30-20.61 / 25.37-26.63 C after step 400: the inputs satisfy the conditions below without the code under test.
    "heating": (5.0, dict(heat_chan=[0], cool_chan=[-1], heat_power=[100.0], cool_power=[0.0], band=[1.0]), 20.0),
    "cooling": (38.0, dict(heat_chan=[-1], cool_chan=[0], heat_power=[0.0], cool_power=[150.0], band=[1.0]), 26.0),
}


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("name", sorted(CYCLING))
def test_a_thermostat_that_really_cycles(name, opts, oracle):
    t_out, th, setpoint = CYCLING[name]
    steps = 800
    md, st, n_sub = closed_form_zone(oracle)
    loads = dict(thermostats=dict(sensor_zone=[0], target_zone=[0], **th))
    channel = np.full((steps, 1), setpoint)
    w = np.tile([t_out, 0.0, 0.0], (steps, n_sub, 1))
    zone = md["zone_slot"]
    with HeatBatch(md, **opts) as b:
        b.upload_state(st.copy())
        trace, failed, applied, modes = b.march_series(w, n_sub, loads=loads, channel=channel, probes=zone)
    assert failed == -1 and applied.shape == (steps, 1)
    acting = applied[:, 0] != 0
    changes = int((acting[1:] != acting[:-1]).sum())
    late = trace[400:, 0]
    print("%s: %d mode changes, zone %.2f - %.2f C after step 400" % (name, changes, late.min(), late.max()))
    assert changes >= 50
    assert np.all(np.abs(late - setpoint) <= 1.5)
    # the rule replayed over the traced sensor temperatures gives exactly the applied powers and the final mode
    np_loads = dict(thermostats={k: np.asarray(v) for k, v in loads["thermostats"].items()})
    replay_modes = np.zeros(1, np.uint8)
    sensor = np.concatenate([st[zone], trace[:-1, 0]])
    replay = np.array([host_rule(sensor[k:k + 1], channel[k], None, None, np_loads, replay_modes)[2][0] for k in range(steps)])
    assert np.array_equal(replay, applied[:, 0])
    assert np.array_equal(replay_modes, modes)


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_series_with_loads_cut_in_two_equals_the_series_in_one(opts):
    n_steps, n_sub, cut = 24, 3, 7
    md, st, channel, drives, probes, a0, b0, loads, w = case("rooms_with_windows", n_steps, n_sub, 2, 11)
    one, two = st.copy(), st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(one)
        trace1, _, applied1, modes1 = b.march_series(w, n_sub, loads=loads, **series_kwargs(channel, drives, probes, a0, b0))
        b.download_state(one)
    with HeatBatch(md, **opts) as b:
        b.upload_state(two)
        ta, _, aa, ma = b.march_series(w[:cut], n_sub, loads=loads,
                                       **series_kwargs(channel, drives, probes, a0, b0, steps=slice(0, cut)))
        second = dict(loads, thermostats=dict(loads["thermostats"], mode=ma))
        tb, _, ab, mb = b.march_series(w[cut:], n_sub, loads=second,
                                       **series_kwargs(channel, drives, probes, a0, b0, steps=slice(cut, None)))
        b.download_state(two)
    assert ma.any(), "no thermostat is on at the cut: the modes carry nothing over it"
    assert np.array_equal(trace1, np.concatenate([ta, tb]))
    assert np.array_equal(applied1, np.concatenate([aa, ab]))
    assert np.array_equal(modes1, mb)
    assert np.array_equal(one, two)


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_no_loads_is_the_plain_series_bit_for_bit(opts):
    n_steps, n_sub = 12, 3
    md, st, channel, drives, probes, a0, b0, loads, w = case("rooms_with_windows", n_steps, n_sub, 2, 5)
    kw = series_kwargs(channel, drives, probes, a0, b0)
    results = []
    for how in ("plain", "empty", "null"):
        state = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(state)
            if how == "plain":
                trace, failed = b.march_series(w, n_sub, **kw)
            elif how == "empty":
                trace, failed, applied, modes = b.march_series(w, n_sub, loads={}, **kw)
                assert applied.shape == (n_steps, 0) and len(modes) == 0
            else:  # l == NULL through the C ABI
                s, keep = binding.make_series(w, n_sub, **kw)
                trace, f = np.zeros((n_steps, len(probes))), binding.C.c_int32(7)
                rc = b._L.heat_batch_march_series_loads(b._h, binding.C.byref(s), None, trace.ctypes.data_as(binding._dp), None,
                                                        binding.C.byref(f))
                assert rc == 0
                failed = f.value
            b.download_state(state)
        assert failed == -1
        results.append((trace, state))
    for trace, state in results[1:]:
        assert np.array_equal(results[0][0], trace) and np.array_equal(results[0][1], state)


def test_a_series_of_no_sub_timestep_still_evaluates_the_loads():
    n_steps = 6
    md, st, channel, drives, probes, a0, b0, loads, w = case("ragged_mixed", n_steps, 1, 2, 21)
    # nothing marches: every step sees the zone temperatures of the start
    modes = start_modes(loads)
    want = np.array([host_rule(st[md["zone_slot"]], channel[k], a0[k], b0[k], loads, modes)[2] for k in range(n_steps)])
    state = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(state)
        trace, failed, applied, got_modes = b.march_series(None, 0, n_steps=n_steps, loads=loads,
                                                           **series_kwargs(channel, drives, probes, a0, b0))
        b.download_state(state)
    assert failed == -1 and np.array_equal(trace, np.tile(st[probes], (n_steps, 1)))
    assert (want != 0).any()
    assert np.array_equal(want, applied) and np.array_equal(modes, got_modes)
    assert np.array_equal(state, st)


def test_thermostats_without_a_mode_array_start_off_and_return_nothing():
    """th_mode == NULL through the C ABI: the applied powers are those of modes that start at zero."""
    n_steps, n_sub = 8, 2
    md, st, channel, drives, probes, a0, b0, loads, w = case("ragged_mixed", n_steps, n_sub, 0, 23)
    kw = series_kwargs(channel, drives, probes)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, applied, modes = b.march_series(w, n_sub, loads=loads, **kw)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        s, keep = binding.make_series(w, n_sub, **kw)
        l, lkeep = binding.make_zone_loads(**loads)
        l.th_mode = None
        trace2, applied2, f = np.zeros_like(trace), np.zeros_like(applied), binding.C.c_int32(7)
        rc = b._L.heat_batch_march_series_loads(b._h, binding.C.byref(s), binding.C.byref(l), trace2.ctypes.data_as(binding._dp),
                                                applied2.ctypes.data_as(binding._dp), binding.C.byref(f))
    assert rc == 0 and f.value == -1
    assert np.array_equal(trace, trace2) and np.array_equal(applied, applied2)
    assert not lkeep["th_mode"].any()  # (not written)


def test_a_nan_flow_volume_is_reported_as_the_zone_failure():
    """A NaN volume makes the flow's m NaN, and with it the zone's a0 and b0. The zone update itself would hide that
    (model.rs:662-668: |b| > 1e-9 is false for a NaN b, the zone keeps its temperature), so the loads report it: the zone's
    failure, HEAT_N_NAN_ZONE, at the step whose channel row holds the NaN."""
    md, st = mdl.clustered_massive(700, Z=28, dt=45.0, seed=3)
    n_steps, j, z = 9, 5, 13
    channel = np.tile([0.02, 10.0], (n_steps, 1))
    channel[j, 0] = np.nan
    loads = dict(flows=dict(zone=[z], volume_chan=[0], temp_chan=[1]))
    for opts, n_sub in [(o, n) for o in OPTIONS for n in (0, 1, 2)]:
        w = mdl.weather_series(n_steps * n_sub, 45.0).reshape(n_steps, n_sub, 3) if n_sub else None
        with HeatBatch(md, **opts) as b:
            b.upload_state(st.copy())
            with pytest.raises(HeatError) as e:
                b.march_series(w, n_sub, loads=loads, channel=channel, probes=md["zone_slot"])
            assert e.value.failed_step == j and e.value.code == 3, str(e.value)   # HEAT_N_NAN_ZONE
            assert b.failed_surface() == (z, 3) and "zone %d" % z in str(e.value)
            assert np.all(np.isfinite(e.value.trace[:j]))
            # the process and the batch survive: a healthy series afterwards
            b.upload_state(st.copy())
            healthy = np.tile([0.02, 10.0], (n_steps, 1))
            trace, failed, _, _ = b.march_series(w, n_sub, loads=loads, channel=healthy, probes=md["zone_slot"])
            assert failed == -1 and np.all(np.isfinite(trace))


def test_sharded_batch_is_refused():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(np.zeros((2, 1, 3)), 1, channel=np.zeros((2, 1)), loads=dict(gains=dict(zone=[0], chan=[0])))
        assert e.value.code == -1 and "sharded" in str(e.value)


def test_bad_loads_are_refused_by_the_march_as_by_the_check():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        with pytest.raises(HeatError) as e:
            b.march_series(np.zeros((2, 1, 3)), 1, channel=np.zeros((2, 1)), loads=dict(gains=dict(zone=[0, 8], chan=[0, 0])))
        assert e.value.code == -4 and "gain 1" in str(e.value)
        with pytest.raises(HeatError) as e:
            b.march_series(np.zeros((2, 1, 3)), 1, channel=np.zeros((2, 1)), loads=dict(flows=dict(zone=[0], volume_chan=[0], temp_chan=[1])))
        assert e.value.code == -4 and "flow 0" in str(e.value)
        got = st.copy()
        b.download_state(got)
        assert np.array_equal(got, st)


def test_weather_sites_with_each_sites_dry_bulb_in_a_channel(oracle):
    """Three sites in one batch; every zone is ventilated with its own site's outdoor air (the site's dry bulb of the step's
    first sub-timestep, which the caller puts into a channel) and heated on a thermostat; against one oracle loop per site."""
    parts = [mdl.clustered_massive(240, Z=10, seed=31), mdl.rooms_with_windows(200, Z=10, seed=32), mdl.ragged_mixed(150, Z=6, seed=34)]
    K = len(parts)
    md, site = mdl.concat([m for m, _ in parts])
    state = np.concatenate([s for _, s in parts])
    n_steps, n_sub = 24, 3
    rng = np.random.default_rng(17)
    w = mdl.weather_sites(n_steps * n_sub, 45.0, K, seed=2).reshape(n_steps, n_sub, K, 3)
    # channels: per site [dry bulb, air volume flow, heating setpoint]
    channel = np.zeros((n_steps, 3 * K))
    probes, ref_trace, ref_applied, ref_state = [], [], [], []
    fz, sz = [], []
    z0 = slot0 = 0
    for k, (m, st) in enumerate(parts):
        Z = m["n_zones"]
        channel[:, 3 * k] = w[:, 0, k, 0]
        channel[:, 3 * k + 1] = rng.uniform(0.0, 0.05, n_steps)
        channel[:, 3 * k + 2] = float(np.median(st[m["zone_slot"]])) + rng.uniform(-0.5, 0.5, n_steps)
        local = dict(flows=dict(zone=np.arange(Z, dtype=np.int32), volume_chan=np.full(Z, 3 * k + 1, np.int32),
                                temp_chan=np.full(Z, 3 * k, np.int32), volume_gain=rng.uniform(0.5, 1.5, Z)),
                     thermostats=dict(sensor_zone=np.arange(Z, dtype=np.int32), target_zone=np.arange(Z, dtype=np.int32),
                                      heat_chan=np.full(Z, 3 * k + 2, np.int32), cool_chan=np.full(Z, -1, np.int32),
                                      heat_power=rng.uniform(200.0, 2000.0, Z), cool_power=np.zeros(Z), band=np.full(Z, 0.4)))
        om = oracle.OracleModel(m)

        def march(s, wk, za, zb, om=om):
            assert om.march(s, wk, za, zb)[0] == 0

        ref = st.copy()
        pr = m["zone_slot"]
        t, a, _ = loop_with_host_rule(march, m, ref, w[:, :, k, :], channel, {}, pr, local)
        probes.append(pr + slot0), ref_trace.append(t), ref_applied.append(a), ref_state.append(ref)
        fz.append((local["flows"], z0)), sz.append((local["thermostats"], z0))
        z0, slot0 = z0 + Z, slot0 + m["n_state"]

    def joined(groups, zone_keys):
        keys = groups[0][0].keys()
        return {key: np.concatenate([g[key] + (off if key in zone_keys else 0) for g, off in groups]) for key in keys}

    loads = dict(flows=joined(fz, ("zone",)), thermostats=joined(sz, ("sensor_zone", "target_zone")))
    probes, ref_trace, ref_applied = np.concatenate(probes), np.concatenate(ref_trace, axis=1), np.concatenate(ref_applied, axis=1)
    ref_state = np.concatenate(ref_state)
    assert (ref_applied > 0).any() and (ref_applied == 0).any()
    own = owned_slots(md)
    for opts in OPTIONS:
        got = state.copy()
        with HeatBatch(md, sites=site, **opts) as b:
            b.upload_state(got)
            trace, failed, applied, modes = b.march_series(w, n_sub, loads=loads, channel=channel, probes=probes)
            b.download_state(got)
        assert failed == -1
        assert_close(ref_trace, trace, "sites trace %s" % _id(opts))
        assert_close(ref_applied, applied, "sites applied %s" % _id(opts))
        assert_close(ref_state[own], got[own], "sites final state %s" % _id(opts))
