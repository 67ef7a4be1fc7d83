"""Sky of a series on the GPU (include/heat_amd.h, heat_sky / heat_batch_march_series_sky): the incident solar and long-wave
irradiance of sky-facing sides formed on the device at every step, from one record per site and step and the surface's normal.

The rule is this library's own contract; its reference is heat_amd/sky.py (incident(): the rule in numpy, line for line).
Every reference loop here — the per-call path (test_series_gpu.per_call_series), the oracle loop (oracle_series), the CPU
definition of the ideal loads (ideal_loads_ref.cpu_series) — writes its inputs as gain x channel value: the sky enters them
as one extra channel column per sky-driven input, filled by sky.incident (`expanded`), so those loops run unchanged and write
exactly the rule's value into the slot (gain x v and v x gain are the same rounded product). That expansion — a column per
wall — is what the feature spares its callers.
Against the per-call path the series must be equal bit for bit; against the oracle at the project's rtol = atol = 1e-9."""
import ctypes as C

import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, binding, modeldict as mdl, sky
from ideal_loads_ref import accumulate, cpu_series
from test_ideal_loads_gpu import ACC, SAT, ideal_case
from test_series_gpu import (INPUTS, MODELS, RTOL, assert_close, oracle_series, owned_slots, per_call_series, probes_of_every_kind,
                             random_drives, series_kwargs, write_inputs, zone_terms, _id)
from test_series_report_gpu import assert_same, replay

pytestmark = pytest.mark.gpu

GAINED = ("solar_front", "ir_back")      # the inputs whose gain array the series carries; the other two are NULL


def random_normals(rng, S):
    """Random unit vectors, plus exactly vertical walls (z == 0), exactly upward roofs and exactly downward soffits."""
    v = rng.normal(size=(S, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    az = rng.uniform(0.0, 2 * np.pi, S)
    wall = np.arange(S) % 5 == 1
    v[wall] = np.stack([np.cos(az), np.sin(az), np.zeros(S)], axis=1)[wall]
    v[np.arange(S) % 11 == 3] = (0.0, 0.0, 1.0)
    v[np.arange(S) % 13 == 4] = (0.0, 0.0, -1.0)
    return v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()


def random_records(rng, n_steps, n_sites):
    """Suns all over the sphere (half of them below the horizon, many behind any given surface), nights without beam, a few
    negative diffuse values: with them the solar sum goes negative and the clamps of surface.rs:916-923 act."""
    sun = rng.normal(size=(n_steps, n_sites, 3))
    sun /= np.linalg.norm(sun, axis=2)[:, :, None]
    shape = (n_steps, n_sites)
    phase = np.add.outer(np.arange(n_steps), np.arange(n_sites))      # (by pattern, not by chance: short series have them all)
    sun[..., 2] = np.where(phase % 4 == 3, -np.abs(sun[..., 2]), sun[..., 2])
    beam = np.where(phase % 3 == 1, 0.0, rng.uniform(0.0, 900.0, shape))
    diffuse = np.where((phase % 6 == 1) | (phase % 6 == 2), rng.uniform(-400.0, -50.0, shape), rng.uniform(0.0, 300.0, shape))
    rec = np.concatenate([sun, np.stack([beam, diffuse, rng.uniform(0.0, 150.0, shape), rng.uniform(250.0, 420.0, shape),
                                         rng.uniform(330.0, 480.0, shape)], axis=2)], axis=2)
    assert (sun[..., 2] < 0).any() and (beam == 0).any() and (diffuse < 0).any()
    return rec


def sky_case(md, rng, n_steps, channel=None, drives=None, n_sites=1, site=None):
    """Channels and drives as random_drives makes them (or the given ones), then random mode bits per surface: an input the
    sky drives loses its channel. Returns (channel, drives of the call — gains on GAINED only —, drives of the reference —
    the same with ones for the NULL gains —, sky arguments)."""
    S = int(md["n_surfaces"])
    if channel is None:
        channel, drives = random_drives(md, rng, n_steps)
    mode = rng.integers(0, 16, S).astype(np.uint8)
    mode[rng.random(S) < 0.25] = 0
    drives = {name: (chan.copy(), gain) for name, (chan, gain) in drives.items()}
    # (the first ten surfaces by pattern, so that the smallest model has every combination of a side's two fields: both from
    # the sky; one from the sky beside a channel; one from the sky beside nothing — front sides, then back sides)
    for side, (solar, ir) in enumerate(((0, 2), (1, 3))):
        for j, (m_s, m_i, other) in enumerate(((1, 1, -1), (1, 0, 4), (1, 0, -1), (0, 1, 0), (0, 1, -1))):
            q = 5 * side + j
            mode[q] = (mode[q] & ~np.uint8(1 << solar | 1 << ir)) | (m_s << solar) | (m_i << ir)
            drives[INPUTS[ir if m_s else solar][0]][0][q] = other
    call, ref = {}, {}
    for bit, (name, _) in enumerate(INPUTS):
        chan, gain = drives[name]
        chan = np.where((mode >> bit & 1) != 0, -1, chan).astype(np.int32)
        call[name] = (chan, gain if name in GAINED else None)
        ref[name] = (chan, gain if name in GAINED else np.ones(S))
    args = dict(record=random_records(rng, n_steps, n_sites), mode=mode, normals=random_normals(rng, S))
    # every combination of the two fields of a side occurs: both from the sky, one from the sky beside a channel, beside nothing
    for solar, ir in ((0, 2), (1, 3)):
        s_on, i_on = (mode >> solar & 1) != 0, (mode >> ir & 1) != 0
        assert (s_on & i_on).any() and (s_on & ~i_on & (call[INPUTS[ir][0]][0] >= 0)).any() and (s_on & ~i_on & (call[INPUTS[ir][0]][0] < 0)).any()
        assert (i_on & ~s_on & (call[INPUTS[solar][0]][0] >= 0)).any() and (i_on & ~s_on & (call[INPUTS[solar][0]][0] < 0)).any()
    return channel, call, ref, args


def expanded(md, channel, ref_drives, args, site=None):
    """The sky as channels, for the reference loops: one column per sky-driven input, filled by sky.incident."""
    S = int(md["n_surfaces"])
    site = np.zeros(S, np.int64) if site is None else np.asarray(site, dtype=np.int64)
    rec, mode, normals = args["record"], args["mode"], args["normals"]
    cols, base, out, lowest = [channel], channel.shape[1], {}, np.inf
    for bit, (name, _) in enumerate(INPUTS):
        chan, gain = ref_drives[name]
        on = np.flatnonzero(mode >> bit & 1)
        v = sky.incident(rec[:, site[on], :], tuple(n[on] for n in normals), name)            # [n_steps, len(on)]
        chan = chan.copy()
        chan[on] = base + np.arange(len(on))
        base += len(on)
        cols.append(v)
        out[name] = (chan, gain)
        if name == "solar_front" and v.size:
            lowest = min(lowest, (v * gain[on]).min())
    assert lowest < 0, "no negative front solar value: the clamp is not exercised"
    return np.concatenate(cols, axis=1), out


def call_kwargs(channel, call, probes, a0=None, b0=None, steps=slice(None), args=None):
    kw = series_kwargs(channel, call, probes, a0, b0, steps=steps)
    if args is not None:
        kw["sky"] = dict(args, record=args["record"][steps])
    return kw


# ---- 1. bit for bit against the per-call path ----
SKY_MODELS = {"ragged_mixed": MODELS["ragged_mixed"], "rooms_with_windows": MODELS["rooms_with_windows"],
              "partitioned_buildings_large": MODELS["partitioned_buildings_large"]}
OPTIONS = [dict(), dict(no_fusion=True), dict(use_graph=True), dict(force_general=True), dict(no_palette=True)]


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model", sorted(SKY_MODELS))
def test_sky_series_equals_the_per_call_path_bit_for_bit(model, opts):
    """A side with only one field sky-driven keeps the other field's uploaded value: the per-call loop, which writes only
    the driven slots into a state whose other slots stay as uploaded, shows it by construction."""
    md, st = SKY_MODELS[model]()
    n_steps = 12
    own = owned_slots(md)
    for form, n_sub in enumerate((1, 2, 5)):
        rng = np.random.default_rng(70 + n_sub)
        channel, call, ref_drives, args = sky_case(md, rng, n_steps)
        probes = probes_of_every_kind(md, rng)
        a0, b0 = zone_terms(md, rng, n_steps, form)
        w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
        ref_channel, ref_drives = expanded(md, channel, ref_drives, args)
        ref = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(ref)
            ref_trace = per_call_series(b, md, ref, w, ref_channel, ref_drives, probes, a0, b0)
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(got)
            trace, failed = b.march_series(w, n_sub, **call_kwargs(channel, call, probes, a0, b0, args=args))
            b.download_state(got)
        assert failed == -1
        assert np.array_equal(ref_trace, trace), "n_sub=%d: %d trace values differ, worst %.3e" % (
            n_sub, int((ref_trace != trace).sum()), np.abs(ref_trace - trace).max())
        assert np.array_equal(ref[own], got[own]), "n_sub=%d: %d state slots differ" % (n_sub, int((ref[own] != got[own]).sum()))


# ---- 2. against the oracle loop, with sites ----
def test_sky_series_of_weather_sites_matches_the_oracle_loop(oracle):
    """The four-part model of test_series_gpu.test_series_of_weather_sites, each site with its own weather, channels and sky
    records, against one oracle loop per site: a wrong site index or record stride shows here."""
    parts = [mdl.clustered_massive(240, Z=10, seed=31), mdl.rooms_with_windows(200, Z=10, seed=32),
             mdl.glazing_cavity(80, Z=2, seed=33), mdl.ragged_mixed(150, Z=6, seed=34)]
    K = len(parts)
    md, site = mdl.concat([m for m, _ in parts])
    state = np.concatenate([s for _, s in parts])
    n_steps, n_sub = 24, 3
    rng = np.random.default_rng(18)
    w = mdl.weather_sites(n_steps * n_sub, 45.0, K, seed=2).reshape(n_steps, n_sub, K, 3)
    S_all = md["n_surfaces"]
    channel = np.zeros((n_steps, 8 * K))
    call = {name: (np.full(S_all, -1, np.int32), np.ones(S_all) if name in GAINED else None) for name, _ in INPUTS}
    record = np.zeros((n_steps, K, 8))
    mode = np.zeros(S_all, np.uint8)
    normals = tuple(np.zeros(S_all) for _ in range(3))
    probes, ref_trace, ref_state, iters = [], [], [], 0
    s0 = slot0 = z0 = 0
    a0 = np.zeros((n_steps, md["n_zones"]))
    b0 = np.zeros((n_steps, md["n_zones"]))
    for k, (m, st) in enumerate(parts):
        ch, cl, rf, args = sky_case(m, rng, n_steps)
        pr = probes_of_every_kind(m, rng, 40)
        ta, tb = zone_terms(m, rng, n_steps, 2)
        S = m["n_surfaces"]
        channel[:, 8 * k:8 * k + 8] = ch
        for name, _ in INPUTS:
            call[name][0][s0:s0 + S] = np.where(cl[name][0] >= 0, cl[name][0] + 8 * k, -1)
            if name in GAINED:
                call[name][1][s0:s0 + S] = cl[name][1]
        record[:, k] = args["record"][:, 0]
        mode[s0:s0 + S] = args["mode"]
        for a in range(3):
            normals[a][s0:s0 + S] = args["normals"][a]
        a0[:, z0:z0 + m["n_zones"]], b0[:, z0:z0 + m["n_zones"]] = ta, tb
        ref = st.copy()
        ref_channel, ref_drives = expanded(m, ch, rf, args)
        t, it = oracle_series(oracle, m, ref, w[:, :, k, :], ref_channel, ref_drives, pr, ta, tb)
        probes.append(pr + slot0)
        ref_trace.append(t)
        ref_state.append(ref)
        iters += it
        s0, slot0, z0 = s0 + S, slot0 + m["n_state"], z0 + m["n_zones"]
    assert np.array_equal(site, np.repeat(np.arange(K), [m["n_surfaces"] for m, _ in parts]))
    probes, ref_trace, ref_state = np.concatenate(probes), np.concatenate(ref_trace, axis=1), np.concatenate(ref_state)
    own = owned_slots(md)
    args = dict(record=record, mode=mode, normals=normals)
    for opts in (dict(), dict(no_fusion=True), dict(use_graph=True), dict(fuse_always=True)):
        got = state.copy()
        with HeatBatch(md, sites=site, **opts) as b:
            b.upload_state(got)
            trace, failed = b.march_series(w, n_sub, **call_kwargs(channel, call, probes, a0, b0, args=args))
            b.download_state(got)
            assert b.nomass_iterations() == iters
        assert failed == -1
        assert_close(ref_trace, trace, "sky sites trace %s" % _id(opts))
        assert_close(ref_state[own], got[own], "sky sites final state %s" % _id(opts))


# ---- 3. the sky has no memory ----
@pytest.mark.parametrize("opts", [dict(), dict(use_graph=True), dict(no_fusion=True)], ids=_id)
def test_sky_series_cut_in_two_equals_the_series_in_one(opts):
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(12)
    n_steps, n_sub, cut = 24, 3, 7
    channel, call, _, args = sky_case(md, rng, n_steps)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, n_steps, 2)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    one, two = st.copy(), st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(one)
        trace1, _ = b.march_series(w, n_sub, **call_kwargs(channel, call, probes, a0, b0, args=args))
        b.download_state(one)
    with HeatBatch(md, **opts) as b:
        b.upload_state(two)
        ta, _ = b.march_series(w[:cut], n_sub, **call_kwargs(channel, call, probes, a0, b0, slice(0, cut), args))
        tb, _ = b.march_series(w[cut:], n_sub, **call_kwargs(channel, call, probes, a0, b0, slice(cut, None), args))
        b.download_state(two)
    assert np.array_equal(trace1, np.concatenate([ta, tb]))
    assert np.array_equal(one, two)


def test_no_sub_timestep_still_sets_the_inputs_of_every_step(oracle):
    md, st = MODELS["ragged_mixed"]()
    rng = np.random.default_rng(20)
    n_steps = 5
    channel, call, ref_drives, args = sky_case(md, rng, n_steps)
    probes = probes_of_every_kind(md, rng)
    ref_channel, ref_drives = expanded(md, channel, ref_drives, args)
    own = owned_slots(md)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed = b.march_series(None, 0, n_steps=n_steps, **call_kwargs(channel, call, probes, args=args))
        assert failed == -1 and np.array_equal(trace, np.tile(st[probes], (n_steps, 1)))
        # the inputs of the last step are on the device: a resident march now is the oracle's from them
        w = mdl.weather_series(3, md["dt"])
        ref = st.copy()
        write_inputs(md, ref, n_steps - 1, ref_channel, ref_drives)
        assert oracle.OracleModel(md).march(ref, w)[0] == 0
        b.march_resident(w)
        b.synchronize()
        got = st.copy()
        b.download_state(got)
    assert_close(ref[own], got[own], "march after a sky series of no sub-timestep")


# ---- 4. with loads, a report and ideal loads in the same call ----
def test_sky_with_loads_a_report_and_ideal_loads(oracle):
    model, n_steps, n_sub = "ragged_mixed", 16, 2
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case(model, n_steps, n_sub, 300 + n_sub)
    rng = np.random.default_rng(41)
    channel, call, ref_drives, args = sky_case(md, rng, n_steps, channel, drives)
    P = len(probes)
    groups = [(probes[rng.integers(0, P, n)], rng.uniform(-2.0, 3.0, n)) for n in (5, 0, 40)]
    report = dict(stats=("min", "step_min", "max", "step_max", "sum"), group_trace=True, groups=groups)
    ref_channel, ref_drives = expanded(md, channel, ref_drives, args)
    ref_state = st.copy()
    ref = cpu_series(oracle, md, ref_state, w, n_sub, ref_channel, ref_drives, probes, loads, ideal, a0, b0)
    print("reference sub-timesteps heating %d, cooling %d, floating %d; saturated %d + %d; smallest |need - cap| / S = %.3g" % (
        ref["n_heat"], ref["n_cool"], ref["n_free"], ref["n_sat_heating"].sum(), ref["n_sat_cooling"].sum(), ref["margin"]))
    assert ref["n_heat"] > 0 and ref["n_cool"] > 0 and ref["n_free"] > 0 and (ref["applied"] != 0).any()
    assert ref["margin"] > 1e-7                           # (test_ideal_loads_gpu: the counts cannot depend on rounding)
    got = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(got)
        out = b.march_series(w, n_sub, loads=loads, ideal=ideal, report=report, **call_kwargs(channel, call, probes, a0, b0, args=args))
        b.download_state(got)
    assert out["failed_step"] == -1
    # at test_ideal_loads_gpu's tolerances
    assert_close(ref["trace"], out["trace"], "sky + ideal trace")
    own = owned_slots(md)
    assert_close(ref_state[own], got[own], "sky + ideal final state")
    assert_close(ref["applied"], out["applied"], "sky + ideal applied")
    assert np.array_equal(ref["modes"], out["modes"])
    dq = np.abs(out["ideal_q"] - ref["ideal_q"]) / ref["scale"]
    print("ideal_q: worst |dq| / S = %.3e (bound %.1e)" % (dq.max(), 1e-9 * n_sub))
    assert np.all(np.isfinite(out["ideal_q"])) and dq.max() <= 1e-9 * n_sub
    for k in SAT:
        assert np.array_equal(ref[k], out["ideal"][k]), k
    # the report against the reference's trace: every probed value is within tol = 1e-9 (1 + |ref|) of the reference, so a
    # group within sum |w| tol, a minimum or maximum within the largest tol of its column, a sum within the sum of them
    where = {int(s): i for i, s in enumerate(probes)}
    tol = RTOL * (1.0 + np.abs(ref["trace"]))
    gcols = [np.array([where[int(s)] for s in slots], dtype=np.int64) for slots, _ in groups]
    ref_groups = np.stack([(wt * ref["trace"][:, c]).sum(axis=1) for c, (_, wt) in zip(gcols, groups)], axis=1)
    gtol = np.stack([(np.abs(wt) * tol[:, c]).sum(axis=1) + 1e-12 for c, (_, wt) in zip(gcols, groups)], axis=1)
    rep = out["report"]
    assert np.all(np.abs(rep["group_trace"] - ref_groups) <= gtol)
    values, vtol = np.concatenate([ref["trace"], ref_groups], axis=1), np.concatenate([tol, gtol], axis=1)
    want = replay(values)
    assert np.all(np.abs(rep["q_min"] - want["q_min"]) <= vtol.max(axis=0))
    assert np.all(np.abs(rep["q_max"] - want["q_max"]) <= vtol.max(axis=0))
    assert np.all(np.abs(rep["q_sum"] - want["q_sum"]) <= vtol.sum(axis=0))
    # ... and exactly the rules over this call's own rows
    mine = replay(np.concatenate([out["trace"], rep["group_trace"]], axis=1))
    assert_same(mine, rep, ("q_min", "q_step_min", "q_max", "q_step_max", "q_sum"), "sky + ideal report")
    assert_same(accumulate(out["ideal_q"]), out["ideal"], ACC, "sky + ideal accumulators")
    # one call and two: the same bits
    cut = 6
    two = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(two)
        first = b.march_series(w[:cut], n_sub, loads=loads, ideal=ideal, report=report,
                               **call_kwargs(channel, call, probes, a0, b0, slice(0, cut), args))
        loads2 = dict(loads, thermostats=dict(loads["thermostats"], mode=first["modes"]))
        second = b.march_series(w[cut:], n_sub, loads=loads2, ideal=dict(ideal, resume=first["ideal"], step_base=cut),
                                report=dict(report, resume=first["report"], step_base=cut),
                                **call_kwargs(channel, call, probes, a0, b0, slice(cut, None), args))
        b.download_state(two)
    for k in ("trace", "ideal_q", "applied"):
        assert np.array_equal(out[k], np.concatenate([first[k], second[k]])), k
    assert np.array_equal(out["report"]["group_trace"], np.concatenate([first["report"]["group_trace"], second["report"]["group_trace"]]))
    assert np.array_equal(out["modes"], second["modes"])
    assert_same(out["ideal"], second["ideal"], ACC + SAT, "cut at %d" % cut)
    assert_same(out["report"], second["report"], ("q_min", "q_step_min", "q_max", "q_step_max", "q_sum"), "cut at %d" % cut)
    assert np.array_equal(got, two)


# ---- 5. no sky is the call without sky ----
def test_no_sky_and_an_all_zero_mode_are_the_call_without_sky():
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(23)
    n_steps, n_sub = 10, 2
    S = int(md["n_surfaces"])
    channel, drives = random_drives(md, rng, n_steps)
    probes = probes_of_every_kind(md, rng)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    kw = series_kwargs(channel, drives, probes)
    plain = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(plain)
        trace, failed = b.march_series(w, n_sub, **kw)
        b.download_state(plain)
    assert failed == -1
    # an all-zero mode (records and normals are not looked at), through the new entry point
    zero = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(zero)
        t0, _ = b.march_series(w, n_sub, sky=dict(record=random_records(rng, n_steps, 1), mode=np.zeros(S, np.uint8)), **kw)
        b.download_state(zero)
    assert np.array_equal(trace, t0) and np.array_equal(plain, zero)
    # sky == NULL
    null = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(null)
        s, keep = binding.make_series(w, n_sub, **kw)
        t1, f1 = np.zeros_like(trace), C.c_int32(5)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert b._L.heat_batch_march_series_sky(b._h, C.byref(s), None, None, None, None, dp(t1), None, None, C.byref(f1)) == 0
        b.download_state(null)
    assert f1.value == -1 and np.array_equal(trace, t1) and np.array_equal(plain, null)
    # a plain series after a sky series: the bits of a fresh batch
    channel2, call, _, args = sky_case(md, rng, n_steps, channel, drives)
    after = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        t_sky, _ = b.march_series(w, n_sub, **call_kwargs(channel2, call, probes, args=args))
        assert not np.array_equal(t_sky, trace)
        b.upload_state(after)
        t2, _ = b.march_series(w, n_sub, **kw)
        b.download_state(after)
    assert np.array_equal(trace, t2) and np.array_equal(plain, after)


# ---- 6. refusals through the batch ----
def test_bad_skies_and_sharded_batches_are_refused_by_the_march():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    S = int(md["n_surfaces"])
    rng = np.random.default_rng(29)
    n_steps, n_sub = 3, 1
    w = np.zeros((n_steps, n_sub, 3))
    mode = np.full(S, 5, np.uint8)
    args = dict(record=random_records(rng, n_steps, 1), mode=mode, normals=random_normals(rng, S))
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        chan = np.full(S, -1, np.int32)
        chan[131] = 0
        with pytest.raises(HeatError) as e:                                  # a mode bit plus a channel
            b.march_series(w, n_sub, channel=np.zeros((n_steps, 1)), ir_front=chan, sky=args)
        assert e.value.code == -4 and "surface 131:" in str(e.value)
        normals = [a.copy() for a in args["normals"]]
        normals[2][66] = np.nan
        with pytest.raises(HeatError) as e:                                  # a normal that is not finite
            b.march_series(w, n_sub, sky=dict(args, normals=normals))
        assert e.value.code == -1 and "surface 66:" in str(e.value)
        # ... and the batch marches a good sky afterwards
        trace, failed = b.march_series(w, n_sub, probes=md["zone_slot"], sky=args)
        assert failed == -1 and np.all(np.isfinite(trace))
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, n_sub, sky=args)
        assert e.value.code == -1 and "sharded" in str(e.value)
