"""Series march on the GPU (include/heat_amd.h, heat_batch_march_series): n_steps caller timesteps in one call, the inputs
driven on the device from schedules, the probed slots recorded after every step.

The expected result is DEFINED by the loop `oracle_series` below: OracleModel.march (≙ ThermalModel::march,
src/model.rs:359-427) step by step, the inputs written into the state before each call exactly as
tests/test_energyplus_series.march_series writes them (validate_wall_heat_transfer.rs:675-705) and the probed slots read
after it. Trace and final state are compared with it at rtol = atol = 1e-9, the no-mass pass counts exactly; against the
per-call path of the library itself (heat_batch_march_ex with numpy writing the inputs) bit for bit."""
import os

import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, modeldict as mdl

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-9
INPUTS = (("solar_front", "solar_front_slot"), ("solar_back", "solar_back_slot"), ("ir_front", "ir_front_slot"),
          ("ir_back", "ir_back_slot"))


def owned_slots(md):
    return np.concatenate([mdl.node_slots(md), md["hs_front_slot"], md["hs_back_slot"], md["flow_front_slot"],
                           md["flow_back_slot"], md["zone_slot"]])


def assert_close(ref, got, what):
    ref, got = np.asarray(ref).ravel(), np.asarray(got).ravel()
    assert ref.shape == got.shape, what
    if not len(ref):
        return
    assert np.all(np.isfinite(got)), what
    err = np.abs(ref - got) / (ATOL + RTOL * np.abs(ref))
    print("%s: worst |diff| %.3e (%.3g of the tolerance)" % (what, np.abs(ref - got).max(), err.max()))
    assert err.max() <= 1.0, "%s: worst |diff| %.3e at %d (ref %.17g, got %.17g)" % (
        what, np.abs(ref - got).max(), int(err.argmax()), ref[err.argmax()], got[err.argmax()])


def write_inputs(md, state, k, channel, drives, own=None):
    """What the caller does before march call k: every driven slot = gain x channel value; the own-face term from the
    face temperature as it is now (validate_wall_heat_transfer.rs:689-699)."""
    for name, key in INPUTS:
        if drives.get(name) is None:
            continue
        chan, gain = drives[name]
        on = chan >= 0
        state[md[key][on]] = gain[on] * channel[k, chan[on]]
    if own is not None:
        first = md["first_node_slot"]
        last = first + np.diff(md["node_offset"]) - 1
        f, b = (own & 1) != 0, (own & 2) != 0
        state[md["ir_front_slot"][f]] += mdl.SIGMA * (state[first[f]] + 273.15) ** 4
        state[md["ir_back_slot"][b]] += mdl.SIGMA * (state[last[b]] + 273.15) ** 4


def term_row(terms, k):
    return None if terms is None else (terms if terms.ndim == 1 else terms[k])


def oracle_series(oracle, md, state, weather, channel, drives, probes, a0=None, b0=None, own=None, threads=1):
    """The definition of a series: returns (trace, no-mass passes); `state` is marched in place."""
    m = oracle.OracleModel(md)
    trace = np.zeros((len(weather), len(probes)))
    iters = 0
    for k in range(len(weather)):
        write_inputs(md, state, k, channel, drives, own)
        rc, it = m.march(state, weather[k], term_row(a0, k), term_row(b0, k), threads=threads)
        assert rc == 0
        iters += it
        trace[k] = state[probes]
    return trace, iters


def per_call_series(b, md, state, weather, channel, drives, probes, a0=None, b0=None):
    """The same loop through heat_batch_march_ex: the path a series replaces."""
    trace = np.zeros((len(weather), len(probes)))
    for k in range(len(weather)):
        write_inputs(md, state, k, channel, drives)
        b.march(state, weather[k], term_row(a0, k), term_row(b0, k), outputs=b.OUT_ALL)
        trace[k] = state[probes]
    return trace


def series_kwargs(channel, drives, probes, a0=None, b0=None, own=None, steps=slice(None)):
    kw = dict(channel=channel[steps], probes=probes, ir_own_face=own)
    for name, _ in INPUTS:
        if drives.get(name) is not None:
            kw[name] = drives[name]
    for name, t in (("zone_a0", a0), ("zone_b0", b0)):
        if t is not None:
            kw[name] = t if t.ndim == 1 else t[steps]
    return kw


def random_drives(md, rng, n_steps, undriven=0.25):
    """Eight channels — 0-3 solar-like (some values negative: the clamps of surface.rs:916-923 are exercised), 4-7
    long-wave-like — random gains, a quarter of the inputs not driven."""
    S = int(md["n_surfaces"])
    channel = np.concatenate([rng.uniform(-60.0, 600.0, (n_steps, 4)), rng.uniform(300.0, 450.0, (n_steps, 4))], axis=1)
    drives = {}
    for i, (name, _) in enumerate(INPUTS):
        chan = (rng.integers(0, 4, S) + (4 if i >= 2 else 0)).astype(np.int32)
        chan[rng.random(S) < undriven] = -1
        drives[name] = (chan, rng.uniform(0.5, 1.5, S))
    return channel, drives


def probes_of_every_kind(md, rng, n=60):
    S, Z = int(md["n_surfaces"]), int(md["n_zones"])
    s_ = rng.integers(0, S, n)
    nodes = md["first_node_slot"][s_] + rng.integers(0, 1 << 30, n) % np.diff(md["node_offset"])[s_]
    first = md["first_node_slot"][s_[:8]]
    last = first + np.diff(md["node_offset"])[s_[:8]] - 1
    return np.concatenate([nodes, first, last, md["hs_front_slot"][s_[:20]], md["hs_back_slot"][s_[20:40]],
                           md["flow_front_slot"][s_[40:]], md["flow_back_slot"][s_[:20]],
                           md["zone_slot"][rng.integers(0, Z, min(Z, 16))]]).astype(np.int64)


def zone_terms(md, rng, n_steps, form):
    """form 0: none; 1: one row for every step; 2: a row per step (model.rs:500-544: heaters, infiltration)."""
    Z = int(md["n_zones"])
    if form == 0:
        return None, None
    shape = (Z,) if form == 1 else (n_steps, Z)
    return rng.uniform(0.0, 400.0, shape), rng.uniform(0.0, 30.0, shape)


MODELS = {
    "ragged_mixed": lambda: mdl.ragged_mixed(700, Z=20, seed=5),
    "rooms_with_windows": lambda: mdl.rooms_with_windows(900, Z=60, seed=6),
    "glazing_cavity": lambda: mdl.glazing_cavity(300, Z=4, seed=7),
    "partitioned_buildings": lambda: mdl.partitioned_buildings(960, 12, seed=8),
    # beyond 8 192 surfaces the cluster-resident march starts at two sub-timesteps per call and runs before, not beside,
    # the streamed remainder (heat_amd.h, "Cluster-resident march")
    "partitioned_buildings_large": lambda: mdl.partitioned_buildings(9600, 10, seed=9),
    "rooms_with_windows_large": lambda: mdl.rooms_with_windows(9000, Z=500, seed=10),
}
OPTIONS = [dict(), dict(no_fusion=True), dict(force_general=True), dict(use_graph=True), dict(no_palette=True)]


def _id(o):
    return "-".join("%s=%s" % kv for kv in o.items()) or "planned"


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model", sorted(MODELS))
def test_series_matches_the_oracle_loop(oracle, model, opts):
    md, st = MODELS[model]()
    big = md["n_surfaces"] > 8192
    n_steps = 24
    for form, n_sub in enumerate((1, 2, 5)):
        rng = np.random.default_rng(100 * form + n_sub)
        channel, drives = random_drives(md, rng, n_steps)
        probes = probes_of_every_kind(md, rng)
        a0, b0 = zone_terms(md, rng, n_steps, form)
        w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
        ref = st.copy()
        ref_trace, iters = oracle_series(oracle, md, ref, w, channel, drives, probes, a0, b0, threads=16 if big else 1)
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(got)
            trace, failed = b.march_series(w, n_sub, **series_kwargs(channel, drives, probes, a0, b0))
            b.download_state(got)
            gpu_iters = b.nomass_iterations()
        assert failed == -1 and trace.shape == (n_steps, len(probes))
        assert_close(ref_trace, trace, "%s n_sub=%d trace" % (model, n_sub))
        own = owned_slots(md)
        assert_close(ref[own], got[own], "%s n_sub=%d final state" % (model, n_sub))
        if not big:  # (the threaded oracle counts no no-mass passes)
            assert gpu_iters == iters


@pytest.mark.parametrize("model", ["ragged_mixed", "rooms_with_windows"])
def test_own_face_term_matches_the_oracle_loop(oracle, model):
    """sigma (T + 273.15)^4 of the own face node at the start of the step, front and back, on some of the driven sides."""
    md, st = MODELS[model]()
    rng = np.random.default_rng(3)
    n_steps, n_sub = 24, 2
    channel, drives = random_drives(md, rng, n_steps)
    pick = rng.random(md["n_surfaces"])
    own = (np.where((drives["ir_front"][0] >= 0) & (pick < 0.6), 1, 0) |
           np.where((drives["ir_back"][0] >= 0) & (pick > 0.3), 2, 0)).astype(np.uint8)
    # channels 4-5: the net gain of the harness, for the sides whose own face term carries the level; 6-7: whole irradiances
    channel[:, 4:6] = rng.uniform(-40.0, 40.0, (n_steps, 2))
    for name, bit in (("ir_front", 1), ("ir_back", 2)):
        chan = drives[name][0]
        chan[chan >= 0] = np.where((own & bit) != 0, 4, 6)[chan >= 0] + chan[chan >= 0] % 2
    assert (own == 1).any() and (own == 2).any() and (own == 3).any() and (own == 0).any()
    probes = probes_of_every_kind(md, rng)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    ref = st.copy()
    ref_trace, _ = oracle_series(oracle, md, ref, w, channel, drives, probes, own=own)
    for opts in (dict(), dict(no_fusion=True), dict(force_general=True)):
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(got)
            trace, failed = b.march_series(w, n_sub, **series_kwargs(channel, drives, probes, own=own))
            b.download_state(got)
        assert failed == -1
        assert_close(ref_trace, trace, "%s own-face trace %s" % (model, _id(opts)))
        assert_close(ref[owned_slots(md)], got[owned_slots(md)], "%s own-face final state %s" % (model, _id(opts)))


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model", ["ragged_mixed", "rooms_with_windows", "partitioned_buildings_large"])
def test_series_equals_the_per_call_path_bit_for_bit(model, opts):
    """A series step runs the kernels of a heat_batch_march_ex call of n_sub on the same inputs: one multiplication per
    driven value, the same clamps and conversion, deterministic zone sums — not one bit may differ."""
    md, st = MODELS[model]()
    n_steps = 24
    own = owned_slots(md)
    for form, n_sub in enumerate((1, 2, 5)):
        rng = np.random.default_rng(7 + n_sub)
        channel, drives = random_drives(md, rng, n_steps)
        probes = probes_of_every_kind(md, rng)
        a0, b0 = zone_terms(md, rng, n_steps, form)
        w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
        ref = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(ref)
            ref_trace = per_call_series(b, md, ref, w, channel, drives, probes, a0, b0)
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(got)
            trace, failed = b.march_series(w, n_sub, **series_kwargs(channel, drives, probes, a0, b0))
            b.download_state(got)
        assert failed == -1
        assert np.array_equal(ref_trace, trace), "n_sub=%d: %d trace values differ, worst %.3e" % (
            n_sub, int((ref_trace != trace).sum()), np.abs(ref_trace - trace).max())
        assert np.array_equal(ref[own], got[own]), "n_sub=%d: %d state slots differ" % (n_sub, int((ref[own] != got[own]).sum()))


@pytest.mark.parametrize("opts", [dict(), dict(use_graph=True), dict(no_fusion=True)], ids=_id)
def test_series_cut_in_two_equals_the_series_in_one(opts):
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(11)
    n_steps, n_sub, cut = 24, 3, 7
    channel, drives = random_drives(md, rng, n_steps)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, n_steps, 2)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    one, two = st.copy(), st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(one)
        trace1, _ = b.march_series(w, n_sub, **series_kwargs(channel, drives, probes, a0, b0))
        b.download_state(one)
    with HeatBatch(md, **opts) as b:
        b.upload_state(two)
        ta, _ = b.march_series(w[:cut], n_sub, **series_kwargs(channel, drives, probes, a0, b0, steps=slice(0, cut)))
        tb, _ = b.march_series(w[cut:], n_sub, **series_kwargs(channel, drives, probes, a0, b0, steps=slice(cut, None)))
        b.download_state(two)
    assert np.array_equal(trace1, np.concatenate([ta, tb]))
    assert np.array_equal(one, two)


def test_series_between_plain_marches(oracle):
    """march -> series -> march on one batch: the series starts from the device's state, and the march after it does not
    take the caller's zone slots, which are older than the device's (heat_batch_upload_inputs)."""
    md, st = MODELS["ragged_mixed"]()
    rng = np.random.default_rng(13)
    n_steps, n_sub = 24, 2
    channel, drives = random_drives(md, rng, n_steps)
    probes = probes_of_every_kind(md, rng)
    w0 = mdl.weather_series(4, md["dt"])
    w = mdl.weather_series(n_steps * n_sub, md["dt"], t0=4 * md["dt"]).reshape(n_steps, n_sub, 3)
    w2 = mdl.weather_series(3, md["dt"], t0=(4 + n_steps * n_sub) * md["dt"])
    own = owned_slots(md)
    ref = st.copy()
    m = oracle.OracleModel(md)
    assert m.march(ref, w0)[0] == 0
    ref_trace, _ = oracle_series(oracle, md, ref, w, channel, drives, probes)
    ref_after_series = ref.copy()
    got = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(got)
        b.march(got, w0)
        trace, _ = b.march_series(w, n_sub, **series_kwargs(channel, drives, probes))
        assert_close(ref_trace, trace, "series after a march")
        # the caller's array still holds the state before the series; it writes its inputs (here: what the oracle's state
        # holds) and marches on
        irr = np.concatenate([md[key] for _, key in INPUTS])
        got[irr] = ref[irr]
        assert m.march(ref, w2)[0] == 0
        b.march(got, w2)
        assert_close(ref[own], got[own], "march after a series")
        after = st.copy()
        b.download_state(after)
        assert np.array_equal(after[own], got[own])
    assert not np.allclose(ref_after_series[md["zone_slot"]], st[md["zone_slot"]])


def test_series_of_weather_sites(oracle):
    """Four sites in one batch, each with its own weather and its own channels, against one oracle loop per site."""
    parts = [mdl.clustered_massive(240, Z=10, seed=31), mdl.rooms_with_windows(200, Z=10, seed=32),
             mdl.glazing_cavity(80, Z=2, seed=33), mdl.ragged_mixed(150, Z=6, seed=34)]
    K = len(parts)
    md, site = mdl.concat([m for m, _ in parts])
    state = np.concatenate([s for _, s in parts])
    n_steps, n_sub = 24, 3
    rng = np.random.default_rng(17)
    w = mdl.weather_sites(n_steps * n_sub, 45.0, K, seed=2).reshape(n_steps, n_sub, K, 3)
    channel = np.zeros((n_steps, 8 * K))
    drives = {name: (np.full(md["n_surfaces"], -1, np.int32), np.ones(md["n_surfaces"])) for name, _ in INPUTS}
    probes, ref_trace, ref_state, iters = [], [], [], 0
    s0 = slot0 = z0 = 0
    a0 = np.zeros((n_steps, md["n_zones"]))
    b0 = np.zeros((n_steps, md["n_zones"]))
    for k, (m, st) in enumerate(parts):
        ch, dr = random_drives(m, rng, n_steps)
        pr = probes_of_every_kind(m, rng, 40)
        ta, tb = zone_terms(m, rng, n_steps, 2)
        S = m["n_surfaces"]
        channel[:, 8 * k:8 * k + 8] = ch
        for name, _ in INPUTS:
            drives[name][0][s0:s0 + S] = np.where(dr[name][0] >= 0, dr[name][0] + 8 * k, -1)
            drives[name][1][s0:s0 + S] = dr[name][1]
        a0[:, z0:z0 + m["n_zones"]], b0[:, z0:z0 + m["n_zones"]] = ta, tb
        ref = st.copy()
        t, it = oracle_series(oracle, m, ref, w[:, :, k, :], ch, dr, pr, ta, tb)
        probes.append(pr + slot0)
        ref_trace.append(t)
        ref_state.append(ref)
        iters += it
        s0, slot0, z0 = s0 + S, slot0 + m["n_state"], z0 + m["n_zones"]
    assert np.array_equal(site, np.repeat(np.arange(K), [m["n_surfaces"] for m, _ in parts]))
    probes, ref_trace, ref_state = np.concatenate(probes), np.concatenate(ref_trace, axis=1), np.concatenate(ref_state)
    own = owned_slots(md)
    for opts in (dict(), dict(no_fusion=True), dict(use_graph=True), dict(fuse_always=True)):
        got = state.copy()
        with HeatBatch(md, sites=site, **opts) as b:
            b.upload_state(got)
            trace, failed = b.march_series(w, n_sub, **series_kwargs(channel, drives, probes, a0, b0))
            b.download_state(got)
            assert b.nomass_iterations() == iters
        assert failed == -1
        assert_close(ref_trace, trace, "sites trace %s" % _id(opts))
        assert_close(ref_state[own], got[own], "sites final state %s" % _id(opts))


ENERGYPLUS_CASES = ["massive_full", "massive_no_ir_no_solar", "massive_no_ir_yes_solar", "massive_yes_ir_no_solar",
                    "mixed_full", "mixed_no_ir_no_solar", "mixed_no_ir_yes_solar", "mixed_yes_ir_no_solar",
                    "nomass_full", "nomass_no_ir_no_solar", "nomass_no_ir_yes_solar", "nomass_yes_ir_no_solar",
                    "tilted", "horizontal"]


@pytest.mark.parametrize("case", ENERGYPLUS_CASES)
def test_energyplus_series_in_one_call(oracle, case):
    """The reference's validation harness (validate_wall_heat_transfer.rs:615-711), all 7 000 rows of a case as ONE series:
    solar as a channel, ir_gain / area / emissivity as the long-wave channel with the own-face bit where the harness adds
    sigma T^4 (emissivity > 1e-3), the zone as the probe. The harness records the zone BEFORE each march: row k of the
    trace is its value k + 1."""
    from test_energyplus_series import CASES, GEOMETRY, GOLD, march_series, single_zone_model
    layers, emis, sol = CASES[case]
    fx = dict(np.load(os.path.join(GOLD, "wall_%s.npz" % case)))
    n = len(fx["t_out"])
    md, st, d, n_sub = single_zone_model(oracle, layers, emis, sol, **GEOMETRY.get(case, {}))
    ref_state = st.copy()
    ref = march_series(oracle, md, ref_state, n_sub, fx, emis)
    w = np.repeat(np.stack([fx["t_out"], np.radians(fx["wind_dir_deg"]), fx["wind_speed"]], axis=1)[:, None, :], n_sub, axis=1)
    feedback = emis > 1e-3
    channel = np.stack([fx["solar"], fx["ir_gain"] / 60.0 / emis if feedback else np.zeros(n)], axis=1)
    kw = dict(channel=channel, solar_front=np.zeros(1, np.int32), probes=md["zone_slot"])
    if feedback:
        kw.update(ir_front=np.ones(1, np.int32), ir_own_face=np.ones(1, np.uint8))
    got_state = st.copy()
    got_state[md["zone_slot"][0]] = fx["zone_t"][0]
    with HeatBatch(md) as b:
        b.upload_state(got_state)
        trace, failed = b.march_series(w, n_sub, **kw)
        b.download_state(got_state)
    assert failed == -1 and trace.shape == (n, 1)
    found = np.concatenate([[fx["zone_t"][0]], trace[:-1, 0]])
    assert_close(ref, found, "%s zone temperature, %d steps" % (case, n))
    own = owned_slots(md)
    assert_close(ref_state[own], got_state[own], "%s final state" % case)


def test_numerical_failure_names_step_and_surface():
    """A NaN in a long-wave channel at step j, on sides that radiate: the yardstick is the per-call path on the same
    inputs — the series reports the step at which heat_batch_march_ex first returns a HEAT_N_* code, the same code and the
    same surface. Then the batch is healthy again."""
    md, st = mdl.clustered_massive(700, Z=28, dt=45.0, seed=3)
    S = md["n_surfaces"]
    bad = np.array([411, 97, 605])
    md["front_emissivity"] = md["front_emissivity"].copy()
    md["front_emissivity"][bad] = 0.9
    n_steps, n_sub, j = 9, 2, 5
    channel = np.full((n_steps, 2), 380.0)
    channel[j, 1] = np.nan
    chan = np.zeros(S, np.int32)
    chan[bad] = 1
    drives = dict(ir_front=(chan, np.ones(S)))
    probes = md["zone_slot"]
    w = mdl.weather_series(n_steps * n_sub, 45.0).reshape(n_steps, n_sub, 3)
    for opts in (dict(), dict(no_fusion=True), dict(force_general=True)):
        with HeatBatch(md, **opts) as b:      # the per-call path
            state = st.copy()
            b.upload_state(state)
            first, code = -1, 0
            for k in range(n_steps):
                write_inputs(md, state, k, channel, drives)
                try:
                    b.march(state, w[k], outputs=b.OUT_ALL)
                except HeatError as e:
                    first, code = k, e.code
                    break
            where = b.failed_surface()
        assert first == j and code > 0 and where[0] in bad and where[1] == code
        with HeatBatch(md, **opts) as b:
            b.upload_state(st.copy())
            with pytest.raises(HeatError) as e:
                b.march_series(w, n_sub, **series_kwargs(channel, drives, probes))
            assert e.value.code == code and e.value.failed_step == first
            assert b.failed_surface() == where
            assert "surface %d" % where[0] in str(e.value)
            # rows before the failing step are good; the batch marches a healthy series afterwards
            healthy = np.full((n_steps, 2), 380.0)
            b.upload_state(st.copy())
            trace, failed = b.march_series(w, n_sub, **series_kwargs(healthy, drives, probes))
            assert failed == -1 and np.all(np.isfinite(trace))
            again = st.copy()
            b.download_state(again)
        with HeatBatch(md, **opts) as b:      # ... the same bits as a batch that never failed
            b.upload_state(st.copy())
            fresh, _ = b.march_series(w, n_sub, **series_kwargs(healthy, drives, probes))
        assert np.array_equal(trace, fresh) and np.array_equal(e.value.trace[:j], fresh[:j])


def test_healthy_series_after_a_failure_matches_the_oracle(oracle):
    md, st = mdl.clustered_massive(300, Z=12, dt=45.0, seed=4)
    S = md["n_surfaces"]
    md["front_emissivity"] = np.full(S, 0.9)
    n_steps, n_sub = 6, 2
    rng = np.random.default_rng(5)
    channel, drives = random_drives(md, rng, n_steps)
    poisoned = channel.copy()
    poisoned[2, 4:] = np.nan
    probes = probes_of_every_kind(md, rng)
    w = mdl.weather_series(n_steps * n_sub, 45.0).reshape(n_steps, n_sub, 3)
    ref = st.copy()
    ref_trace, _ = oracle_series(oracle, md, ref, w, channel, drives, probes)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        with pytest.raises(HeatError) as e:
            b.march_series(w, n_sub, **series_kwargs(poisoned, drives, probes))
        assert e.value.code > 0 and e.value.failed_step == 2
        b.upload_state(st.copy())
        trace, failed = b.march_series(w, n_sub, **series_kwargs(channel, drives, probes))
        got = st.copy()
        b.download_state(got)
    assert failed == -1
    assert_close(ref_trace, trace, "healthy series after a failure")
    assert_close(ref[owned_slots(md)], got[owned_slots(md)], "its final state")


def test_the_empty_series(oracle):
    md, st = MODELS["ragged_mixed"]()
    rng = np.random.default_rng(19)
    channel, drives = random_drives(md, rng, 5)
    probes = probes_of_every_kind(md, rng)
    own = owned_slots(md)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        # n_steps = 0: nothing
        trace, failed = b.march_series(np.zeros((0, 3)), 2, probes=probes)
        assert trace.shape == (0, len(probes)) and failed == -1
        # n_sub = 0: nothing is marched, the inputs are set and the probes recorded (model.rs:369: the loop body never runs)
        trace, failed = b.march_series(None, 0, n_steps=5, **series_kwargs(channel, drives, probes))
        assert failed == -1 and np.array_equal(trace, np.tile(st[probes], (5, 1)))
        got = st.copy()
        b.download_state(got)
        assert np.array_equal(got, st)
        # ... and the inputs of the last step are on the device: a resident march now is the oracle's from them
        w = mdl.weather_series(3, md["dt"])
        ref = st.copy()
        write_inputs(md, ref, 4, channel, drives)
        assert oracle.OracleModel(md).march(ref, w)[0] == 0
        b.march_resident(w)
        b.synchronize()
        b.download_state(got)
        assert_close(ref[own], got[own], "march after a series of no sub-timestep")
    w = mdl.weather_series(8, md["dt"]).reshape(4, 2, 3)
    ref = st.copy()
    ref_trace, _ = oracle_series(oracle, md, ref, w, channel, {}, probes)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        # n_channels = 0: nothing driven; n_probes = 0: no trace
        trace, failed = b.march_series(w, 2, probes=probes)
        assert_close(ref_trace, trace, "series without channels")
        b.upload_state(st.copy())
        trace, failed = b.march_series(w, 2, solar_front=np.full(md["n_surfaces"], -1, np.int32))
        assert trace.shape == (4, 0) and failed == -1
        got = st.copy()
        b.download_state(got)
        assert_close(ref[own], got[own], "series without probes")


def test_sharded_batch_is_refused():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    from heat_amd import binding
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(np.zeros((2, 1, 3)), 1)
        assert e.value.code == -1 and "sharded" in str(e.value)
