"""Solar gains of a series on the GPU (include/heat_amd.h, heat_solar_gains / heat_batch_march_series_gains): the solar
radiation the windows transmit, formed on the device at every step from the sky's records, and what the room's faces receive
of it through the caller's entry list.

The rule is this library's own contract; its reference is heat_amd/solar_gains.py (transmitted() and received(): the rule in
numpy, line for line). Every reference loop here — the per-call path (test_series_gpu.per_call_series), the oracle loop
(oracle_series), the CPU definition of the ideal loads (ideal_loads_ref.cpu_series) — writes its inputs as gain x channel
value: the gains enter them as one extra channel column per receiver, filled by solar_gains.received (`with_gains`), beside
the columns test_sky_gpu.expanded makes for the sky-driven inputs, so those loops run unchanged. That expansion — a column per
inside face — is what the feature spares its callers.
Against the per-call path the series must be equal bit for bit; against the oracle at the project's rtol = atol = 1e-9."""
import ctypes as C

import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, binding, modeldict as mdl, solar_gains
from ideal_loads_ref import accumulate, cpu_series
from test_ideal_loads_gpu import ACC, SAT, ideal_case
from test_series_gpu import (MODELS, RTOL, assert_close, oracle_series, owned_slots, per_call_series, probes_of_every_kind, random_drives,
                             series_kwargs, write_inputs, zone_terms, _id)
from test_series_report_gpu import assert_same, replay
from test_sky_gpu import OPTIONS, SKY_MODELS, call_kwargs, expanded, random_normals, sky_case

pytestmark = pytest.mark.gpu

EN = ("en_surface", "en_side", "en_aperture", "en_beam", "en_diffuse")
SOLAR = ("solar_front", "solar_back")


def longest_gap(has):
    """The longest run of sides without entries between two sides that have them."""
    at = np.flatnonzero(has)
    return int(np.diff(at).max()) - 1 if len(at) > 1 else 0


def gains_case(md, rng, n_steps, channel=None, drives=None):
    """A sky case (test_sky_gpu.sky_case: channels, sky-driven inputs, gains on solar_front and ir_back only) plus solar
    gains: apertures in two zones of three shared out by distribute_by_area with shares of their own, then — by pattern, not
    by chance, and asserted — the cases the tables and the kernel can get wrong. Receivers lose their solar channel and their
    solar sky bit: an input has one source. Returns (channel, drives of the call, drives of the reference, sky arguments,
    gains arguments)."""
    S, Z = int(md["n_surfaces"]), int(md["n_zones"])
    channel, call, ref, args = sky_case(md, rng, n_steps, channel, drives)
    args["record"][..., 0] = -np.abs(args["record"][..., 0])              # the sun stays in the west: sun_x <= 0 at every step
    back_space = md["back_kind"] == mdl.SPACE
    dark = (md["back_zone"] % 3 == 2) if Z >= 3 else (md["back_zone"] == Z - 1)       # zones without a window
    lo, gap = S // 3, min(130, S // 3)                                     # the backs of surfaces [lo, lo + gap) receive nothing
    outside = (np.arange(S) < lo) | (np.arange(S) >= lo + gap)
    windows = np.flatnonzero(back_space & ~dark & outside)[::5]
    free = np.flatnonzero(back_space & dark & outside)                     # their backs receive only what is forced below
    NA = len(windows)
    assert NA >= 3 and len(free) >= 4
    en = solar_gains.distribute_by_area(md, windows)
    keep = (en["en_side"] == 0) | outside[en["en_surface"]]
    en = {k: v[keep] for k, v in en.items()}
    n0 = len(en["en_surface"])
    en["en_beam"] = en["en_beam"] * rng.uniform(0.5, 1.5, n0)
    en["en_diffuse"] = en["en_diffuse"] * rng.uniform(0.5, 1.5, n0)
    lists = {k: [en[k]] for k in EN}

    def add(surface, side, aperture):
        aperture = np.atleast_1d(aperture)
        n = len(aperture)
        for k, v in zip(EN, (np.full(n, surface), np.full(n, side), aperture, rng.uniform(1e-3, 2e-2, n), rng.uniform(1e-3, 2e-2, n))):
            lists[k].append(v)

    one, many = int(free[0]), int(free[1])
    add(one, 1, 1)                                                         # a receiver with exactly one entry
    add(many, 1, np.arange(70) % NA)                                       # one with more than 64, reading windows of other zones
    part = np.flatnonzero(back_space & (md["front_kind"] == mdl.SPACE) & outside)
    both = int(part[0]) if len(part) else int(free[2])
    add(both, 0, 0)                                                        # both sides of one partition
    add(both, 1, 2)
    add(int(en["en_surface"][0]), int(en["en_side"][0]), NA - 1)           # far from the first entry of its receiver: the list's ends
    gains = {k: np.concatenate(lists[k]).astype(en[k].dtype) for k in EN}
    key = gains["en_side"].astype(np.int64) * S + gains["en_surface"]
    if len(np.unique(key)) % 64 == 0:                                      # the last slice is not a full one
        add(int(free[3]), 1, 0)
        gains = {k: np.concatenate(lists[k]).astype(en[k].dtype) for k in EN}
        key = gains["en_side"].astype(np.int64) * S + gains["en_surface"]
    count = np.bincount(key, minlength=2 * S)
    nx, ny, nz = random_normals(rng, NA)
    nx[0], ny[0], nz[0] = 1.0, 0.0, 0.0                                    # a window that faces east: the sun is always behind it
    gains.update(ap_surface=windows, ap_normal=(nx, ny, nz), ap_tau_diffuse=rng.uniform(0.2, 0.8, NA),
                 ap_tau_coef=np.concatenate([rng.uniform(0.3, 0.9, (NA, 1)), rng.uniform(-0.2, 0.2, (NA, 5))], axis=1),
                 ap_scale=md["area"][windows] * rng.uniform(0.5, 1.0, NA))
    # a receiver beside a sky-driven and one beside a channel-driven long-wave field on the same side
    backs = np.unique(gains["en_surface"][gains["en_side"] == 1])
    q_sky, q_chan = int(backs[0]), int(backs[1])
    mode = args["mode"]
    mode[q_sky] |= 8
    mode[q_chan] &= ~np.uint8(8)
    ir_back = call["ir_back"][0].copy()
    ir_back[q_sky], ir_back[q_chan] = -1, 5
    call["ir_back"], ref["ir_back"] = (ir_back, call["ir_back"][1]), (ir_back, ref["ir_back"][1])
    # an input has one source
    for side, name in enumerate(SOLAR):
        on = np.flatnonzero(count[side * S:(side + 1) * S])
        mode[on] &= ~np.uint8(1 << side)
        chan = call[name][0].copy()
        chan[on] = -1
        call[name], ref[name] = (chan, call[name][1]), (chan, ref[name][1])
    # ---- the cases, asserted ----
    assert count[S + one] == 1
    assert count[S + many] > 64 and np.all(md["back_zone"][windows[gains["en_aperture"][key == S + many]]] != md["back_zone"][many])
    assert count[both] > 0 and count[S + both] > 0
    assert np.all(count[S + windows] > 0)                                  # an aperture is itself a receiver
    first = np.flatnonzero(key == key[0])
    assert first[0] == 0 and first[-1] >= len(key) - 2                     # entries of one receiver at both ends of the list
    # (in the caller's order of the sides; the models used with the per-call path have S >= 700: two slices' worth)
    assert longest_gap(count > 0) >= gap and not count[S + lo:S + lo + gap].any() and count[S + lo + gap:].any() and count[S:S + lo].any()
    assert int((count > 0).sum()) % 64 != 0
    assert mode[q_sky] & 8 and count[S + q_sky] > 0 and call["ir_back"][0][q_chan] >= 0 and count[S + q_chan] > 0
    assert (args["record"][..., 4] < 0).any()                              # negative diffuse values: with_gains asserts the clamp acts
    return channel, call, ref, args, gains


def with_gains(md, ref_channel, ref_drives, args, gains, site=None):
    """The gains as channels, for the reference loops: one column per receiver, filled by solar_gains.received. Returns the
    widened table and drives, transmitted [n_steps, n_apertures] and ap_sum [n_apertures] as the rule gives them."""
    S = int(md["n_surfaces"])
    site = np.zeros(S, np.int64) if site is None else np.asarray(site, dtype=np.int64)
    pb, pd = solar_gains.transmitted(args["record"][:, site[gains["ap_surface"]], :], gains["ap_normal"], gains["ap_tau_coef"],
                                     gains["ap_tau_diffuse"], gains["ap_scale"])
    assert np.all(pb[:, 0] == 0.0) and np.any(pd[:, 0] != 0.0) and (pb[:, 1:] > 0).any()      # the sun is always behind aperture 0
    v, has = solar_gains.received(pb, pd, n_surfaces=S, **{k: gains[k] for k in EN})
    cols, base, out, lowest = [ref_channel], ref_channel.shape[1], dict(ref_drives), np.inf
    for side, name in enumerate(SOLAR):
        chan, gain = ref_drives[name]
        on = np.flatnonzero(has[side])
        assert np.all(chan[on] < 0) and not (args["mode"][on] >> side & 1).any()
        chan = chan.copy()
        chan[on] = base + np.arange(len(on))
        base += len(on)
        cols.append(v[:, side, on])
        out[name] = (chan, gain)
        lowest = min(lowest, (v[:, side, on] * gain[on]).min())
    assert lowest < 0, "no negative received value: the clamp is not exercised"
    p = pb + pd
    ap_sum = np.zeros(p.shape[1])
    for k in range(len(p)):
        ap_sum = ap_sum + p[k]
    return np.concatenate(cols, axis=1), out, p, ap_sum


def gains_kwargs(channel, call, probes, a0, b0, args, gains, steps=slice(None), ap_sum=None):
    return dict(call_kwargs(channel, call, probes, a0, b0, steps, args), gains=dict(gains, ap_sum=ap_sum))


# ---- 1. bit for bit against the per-call path ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model", sorted(SKY_MODELS))
def test_gains_series_equals_the_per_call_path_bit_for_bit(model, opts):
    md, st = SKY_MODELS[model]()
    n_steps = 12
    own = owned_slots(md)
    for form, n_sub in enumerate((1, 2, 5)):
        rng = np.random.default_rng(170 + n_sub)
        channel, call, ref_drives, args, gains = gains_case(md, rng, n_steps)
        probes = probes_of_every_kind(md, rng)
        a0, b0 = zone_terms(md, rng, n_steps, form)
        w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
        ref_channel, ref_drives = expanded(md, channel, ref_drives, args)
        ref_channel, ref_drives, ref_p, ref_sum = with_gains(md, ref_channel, ref_drives, args, gains)
        ref = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(ref)
            ref_trace = per_call_series(b, md, ref, w, ref_channel, ref_drives, probes, a0, b0)
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(got)
            trace, failed, transmitted, ap_sum = b.march_series(w, n_sub, **gains_kwargs(channel, call, probes, a0, b0, args, gains))
            b.download_state(got)
        assert failed == -1
        assert np.array_equal(ref_p, transmitted), "n_sub=%d: %d transmitted powers differ" % (n_sub, int((ref_p != transmitted).sum()))
        assert np.array_equal(ref_sum, ap_sum), "n_sub=%d: %d aperture sums differ" % (n_sub, int((ref_sum != ap_sum).sum()))
        assert np.array_equal(ref_trace, trace), "n_sub=%d: %d trace values differ, worst %.3e" % (
            n_sub, int((ref_trace != trace).sum()), np.abs(ref_trace - trace).max())
        assert np.array_equal(ref[own], got[own]), "n_sub=%d: %d state slots differ" % (n_sub, int((ref[own] != got[own]).sum()))


# ---- 2. against the oracle loop, with sites ----
def test_gains_series_of_weather_sites_matches_the_oracle_loop(oracle):
    """The four-part model of test_sky_gpu, each site with its own weather, channels, sky records and windows, against one
    oracle loop per site: an aperture that reads another site's record shows here."""
    parts = [mdl.clustered_massive(240, Z=10, seed=31), mdl.rooms_with_windows(200, Z=10, seed=32),
             mdl.glazing_cavity(80, Z=2, seed=33), mdl.ragged_mixed(150, Z=6, seed=34)]
    K = len(parts)
    md, site = mdl.concat([m for m, _ in parts])
    state = np.concatenate([s for _, s in parts])
    n_steps, n_sub = 24, 3
    rng = np.random.default_rng(118)
    w = mdl.weather_sites(n_steps * n_sub, 45.0, K, seed=2).reshape(n_steps, n_sub, K, 3)
    S_all = md["n_surfaces"]
    channel = np.zeros((n_steps, 8 * K))
    call = {name: (np.full(S_all, -1, np.int32), np.ones(S_all) if name in ("solar_front", "ir_back") else None)
            for name in ("solar_front", "solar_back", "ir_front", "ir_back")}
    record = np.zeros((n_steps, K, 8))
    mode = np.zeros(S_all, np.uint8)
    normals = tuple(np.zeros(S_all) for _ in range(3))
    probes, ref_trace, ref_state, ref_p, ref_sum, all_gains, iters = [], [], [], [], [], [], 0
    s0 = slot0 = z0 = ap0 = 0
    a0 = np.zeros((n_steps, md["n_zones"]))
    b0 = np.zeros((n_steps, md["n_zones"]))
    for k, (m, st) in enumerate(parts):
        ch, cl, rf, args, gains = gains_case(m, rng, n_steps)
        pr = probes_of_every_kind(m, rng, 40)
        ta, tb = zone_terms(m, rng, n_steps, 2)
        S = m["n_surfaces"]
        channel[:, 8 * k:8 * k + 8] = ch
        for name in call:
            call[name][0][s0:s0 + S] = np.where(cl[name][0] >= 0, cl[name][0] + 8 * k, -1)
            if call[name][1] is not None:
                call[name][1][s0:s0 + S] = cl[name][1]
        record[:, k] = args["record"][:, 0]
        mode[s0:s0 + S] = args["mode"]
        for a in range(3):
            normals[a][s0:s0 + S] = args["normals"][a]
        a0[:, z0:z0 + m["n_zones"]], b0[:, z0:z0 + m["n_zones"]] = ta, tb
        ref = st.copy()
        ref_channel, ref_drives = expanded(m, ch, rf, args)
        ref_channel, ref_drives, p, total = with_gains(m, ref_channel, ref_drives, args, gains)
        t, it = oracle_series(oracle, m, ref, w[:, :, k, :], ref_channel, ref_drives, pr, ta, tb)
        all_gains.append(dict(gains, ap_surface=gains["ap_surface"] + s0, en_surface=gains["en_surface"] + s0,
                              en_aperture=gains["en_aperture"] + ap0))
        probes.append(pr + slot0)
        ref_trace.append(t)
        ref_state.append(ref)
        ref_p.append(p)
        ref_sum.append(total)
        iters += it
        s0, slot0, z0, ap0 = s0 + S, slot0 + m["n_state"], z0 + m["n_zones"], ap0 + len(gains["ap_surface"])
    probes, ref_trace, ref_state = np.concatenate(probes), np.concatenate(ref_trace, axis=1), np.concatenate(ref_state)
    gains = {k: np.concatenate([g[k] for g in all_gains]) for k in all_gains[0] if k != "ap_normal"}
    gains["ap_normal"] = tuple(np.concatenate([g["ap_normal"][a] for g in all_gains]) for a in range(3))
    own = owned_slots(md)
    args = dict(record=record, mode=mode, normals=normals)
    for opts in (dict(), dict(no_fusion=True), dict(use_graph=True), dict(fuse_always=True)):
        got = state.copy()
        with HeatBatch(md, sites=site, **opts) as b:
            b.upload_state(got)
            trace, failed, transmitted, ap_sum = b.march_series(w, n_sub, **gains_kwargs(channel, call, probes, a0, b0, args, gains))
            b.download_state(got)
            assert b.nomass_iterations() == iters
        assert failed == -1
        assert np.array_equal(np.concatenate(ref_p, axis=1), transmitted) and np.array_equal(np.concatenate(ref_sum), ap_sum)
        assert_close(ref_trace, trace, "gains sites trace %s" % _id(opts))
        assert_close(ref_state[own], got[own], "gains sites final state %s" % _id(opts))


# ---- 3. no memory beyond ap_sum ----
@pytest.mark.parametrize("opts", [dict(), dict(use_graph=True), dict(no_fusion=True)], ids=_id)
def test_gains_series_cut_in_two_equals_the_series_in_one(opts):
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(112)
    n_steps, n_sub, cut = 24, 3, 7
    channel, call, _, args, gains = gains_case(md, rng, n_steps)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, n_steps, 2)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    one, two = st.copy(), st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(one)
        trace1, _, p1, sum1 = b.march_series(w, n_sub, **gains_kwargs(channel, call, probes, a0, b0, args, gains))
        b.download_state(one)
    with HeatBatch(md, **opts) as b:
        b.upload_state(two)
        ta, _, pa, sum_a = b.march_series(w[:cut], n_sub, **gains_kwargs(channel, call, probes, a0, b0, args, gains, slice(0, cut)))
        tb, _, pb, sum_b = b.march_series(w[cut:], n_sub, **gains_kwargs(channel, call, probes, a0, b0, args, gains, slice(cut, None), sum_a))
        b.download_state(two)
    assert np.array_equal(trace1, np.concatenate([ta, tb])) and np.array_equal(p1, np.concatenate([pa, pb]))
    assert np.array_equal(sum1, sum_b) and not np.array_equal(sum1, sum_a) and np.all(sum_a != 0)
    assert np.array_equal(one, two)


def test_no_sub_timestep_still_sets_the_inputs_of_every_step(oracle):
    md, st = MODELS["ragged_mixed"]()
    rng = np.random.default_rng(120)
    n_steps = 5
    channel, call, ref_drives, args, gains = gains_case(md, rng, n_steps)
    probes = probes_of_every_kind(md, rng)
    ref_channel, ref_drives = expanded(md, channel, ref_drives, args)
    ref_channel, ref_drives, ref_p, ref_sum = with_gains(md, ref_channel, ref_drives, args, gains)
    own = owned_slots(md)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, transmitted, ap_sum = b.march_series(None, 0, n_steps=n_steps, **gains_kwargs(channel, call, probes, None, None, args, gains))
        assert failed == -1 and np.array_equal(trace, np.tile(st[probes], (n_steps, 1)))
        assert np.array_equal(ref_p, transmitted) and np.array_equal(ref_sum, ap_sum)
        # the inputs of the last step are on the device: a resident march now is the oracle's from them
        w = mdl.weather_series(3, md["dt"])
        ref = st.copy()
        write_inputs(md, ref, n_steps - 1, ref_channel, ref_drives)
        assert oracle.OracleModel(md).march(ref, w)[0] == 0
        b.march_resident(w)
        b.synchronize()
        got = st.copy()
        b.download_state(got)
    assert_close(ref[own], got[own], "march after a gains series of no sub-timestep")


# ---- 4. with loads, a report and ideal loads in the same call ----
def test_gains_with_loads_a_report_and_ideal_loads(oracle):
    model, n_steps, n_sub = "ragged_mixed", 16, 2
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = ideal_case(model, n_steps, n_sub, 300 + n_sub)
    rng = np.random.default_rng(141)
    channel, call, ref_drives, args, gains = gains_case(md, rng, n_steps, channel, drives)
    P = len(probes)
    groups = [(probes[rng.integers(0, P, n)], rng.uniform(-2.0, 3.0, n)) for n in (5, 0, 40)]
    report = dict(stats=("min", "step_min", "max", "step_max", "sum"), group_trace=True, groups=groups)
    ref_channel, ref_drives = expanded(md, channel, ref_drives, args)
    ref_channel, ref_drives, ref_p, ref_sum = with_gains(md, ref_channel, ref_drives, args, gains)
    ref_state = st.copy()
    ref = cpu_series(oracle, md, ref_state, w, n_sub, ref_channel, ref_drives, probes, loads, ideal, a0, b0)
    print("reference sub-timesteps heating %d, cooling %d, floating %d; saturated %d + %d; smallest |need - cap| / S = %.3g" % (
        ref["n_heat"], ref["n_cool"], ref["n_free"], ref["n_sat_heating"].sum(), ref["n_sat_cooling"].sum(), ref["margin"]))
    assert ref["n_heat"] > 0 and ref["n_cool"] > 0 and ref["n_free"] > 0 and (ref["applied"] != 0).any()
    assert ref["margin"] > 1e-7                           # (test_ideal_loads_gpu: the counts cannot depend on rounding)
    got = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(got)
        out = b.march_series(w, n_sub, loads=loads, ideal=ideal, report=report, **gains_kwargs(channel, call, probes, a0, b0, args, gains))
        b.download_state(got)
    assert out["failed_step"] == -1
    assert np.array_equal(ref_p, out["transmitted"]) and np.array_equal(ref_sum, out["ap_sum"])
    # at test_ideal_loads_gpu's tolerances
    assert_close(ref["trace"], out["trace"], "gains + ideal trace")
    own = owned_slots(md)
    assert_close(ref_state[own], got[own], "gains + ideal final state")
    assert_close(ref["applied"], out["applied"], "gains + ideal applied")
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
    assert_same(mine, rep, ("q_min", "q_step_min", "q_max", "q_step_max", "q_sum"), "gains + ideal report")
    assert_same(accumulate(out["ideal_q"]), out["ideal"], ACC, "gains + ideal accumulators")
    # one call and two: the same bits
    cut = 6
    two = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(two)
        first = b.march_series(w[:cut], n_sub, loads=loads, ideal=ideal, report=report,
                               **gains_kwargs(channel, call, probes, a0, b0, args, gains, slice(0, cut)))
        loads2 = dict(loads, thermostats=dict(loads["thermostats"], mode=first["modes"]))
        second = b.march_series(w[cut:], n_sub, loads=loads2, ideal=dict(ideal, resume=first["ideal"], step_base=cut),
                                report=dict(report, resume=first["report"], step_base=cut),
                                **gains_kwargs(channel, call, probes, a0, b0, args, gains, slice(cut, None), first["ap_sum"]))
        b.download_state(two)
    for k in ("trace", "ideal_q", "applied", "transmitted"):
        assert np.array_equal(out[k], np.concatenate([first[k], second[k]])), k
    assert np.array_equal(out["report"]["group_trace"], np.concatenate([first["report"]["group_trace"], second["report"]["group_trace"]]))
    assert np.array_equal(out["modes"], second["modes"]) and np.array_equal(out["ap_sum"], second["ap_sum"])
    assert_same(out["ideal"], second["ideal"], ACC + SAT, "cut at %d" % cut)
    assert_same(out["report"], second["report"], ("q_min", "q_step_min", "q_max", "q_step_max", "q_sum"), "cut at %d" % cut)
    assert np.array_equal(got, two)


# ---- 5. no gains is the call without gains ----
def test_no_gains_and_empty_gains_are_the_call_without_gains():
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(123)
    n_steps, n_sub = 10, 2
    channel, call, _, args, gains = gains_case(md, rng, n_steps)
    probes = probes_of_every_kind(md, rng)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    kw = call_kwargs(channel, call, probes, args=args)                      # the sky of the case, and no gains
    plain = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(plain)
        trace, failed = b.march_series(w, n_sub, **kw)
        b.download_state(plain)
    assert failed == -1
    for empty in (None, {}):                                                # gains=None; neither an aperture nor an entry
        same = st.copy()
        with HeatBatch(md) as b:
            b.upload_state(same)
            out = b.march_series(w, n_sub, gains=empty, **kw)
            b.download_state(same)
        assert np.array_equal(trace, out[0]) and out[1] == -1 and np.array_equal(plain, same)
        if empty is not None:
            assert out[2].shape == (n_steps, 0) and out[3].shape == (0,)
    # gains == NULL and sky == NULL through the new entry point: the series without either
    skyless = series_kwargs(channel, call, probes)
    ref = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(ref)
        t_ref, _ = b.march_series(w, n_sub, **skyless)
        b.download_state(ref)
    null = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(null)
        s, keep = binding.make_series(w, n_sub, **skyless)
        t1, p1, f1 = np.zeros_like(trace), np.full((n_steps, 3), 7.0), C.c_int32(5)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert b._L.heat_batch_march_series_gains(b._h, C.byref(s), None, None, None, None, None, dp(t1), None, None, dp(p1), C.byref(f1)) == 0
        b.download_state(null)
    assert f1.value == -1 and np.array_equal(t_ref, t1) and np.array_equal(ref, null) and np.all(p1 == 7.0)
    # a plain series after a gains series: the bits of a fresh batch
    after = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        t_gains = b.march_series(w, n_sub, **gains_kwargs(channel, call, probes, None, None, args, gains))[0]
        assert not np.array_equal(t_gains, trace)
        b.upload_state(after)
        t2, _ = b.march_series(w, n_sub, **kw)
        b.download_state(after)
    assert np.array_equal(trace, t2) and np.array_equal(plain, after)


def test_apertures_nobody_receives_from_are_transmitted_and_nothing_else():
    """Apertures without any entry: k_series_apertures runs alone (no receiver tables, no k_series_solar_gains), transmitted
    and ap_sum are the rule's, and the march is the march without gains to the bit."""
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(124)
    n_steps, n_sub = 10, 2
    channel, call, _, args, gains = gains_case(md, rng, n_steps)
    probes = probes_of_every_kind(md, rng)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    kw = call_kwargs(channel, call, probes, args=args)
    alone = {k: v for k, v in gains.items() if k not in EN}
    pb, pd = solar_gains.transmitted(args["record"][:, np.zeros(len(alone["ap_surface"]), np.int64), :], alone["ap_normal"],
                                     alone["ap_tau_coef"], alone["ap_tau_diffuse"], alone["ap_scale"])
    start = rng.uniform(0.0, 1e3, pb.shape[1])
    ref_sum = start.copy()
    for k in range(n_steps):
        ref_sum = ref_sum + (pb[k] + pd[k])
    plain, got = st.copy(), st.copy()
    with HeatBatch(md) as b:
        b.upload_state(plain)
        trace, failed = b.march_series(w, n_sub, **kw)
        b.download_state(plain)
    with HeatBatch(md) as b:
        b.upload_state(got)
        t, f, transmitted, ap_sum = b.march_series(w, n_sub, gains=dict(alone, ap_sum=start), **kw)
        b.download_state(got)
    assert failed == -1 and f == -1 and (pb + pd != 0).any()
    assert np.array_equal(transmitted, pb + pd) and np.array_equal(ap_sum, ref_sum)
    assert np.array_equal(trace, t) and np.array_equal(plain, got)


# ---- 6. refusals through the batch ----
def test_bad_gains_and_sharded_batches_are_refused_by_the_march():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    S = int(md["n_surfaces"])
    rng = np.random.default_rng(129)
    n_steps, n_sub = 3, 1
    w = np.zeros((n_steps, n_sub, 3))
    windows = np.arange(10) * 17
    gains = dict(solar_gains.distribute_by_area(md, windows), ap_surface=windows, ap_normal=random_normals(rng, 10),
                 ap_tau_coef=rng.uniform(0, 0.2, (10, 6)), ap_tau_diffuse=rng.uniform(0.2, 0.8, 10), ap_scale=md["area"][windows])
    sky = dict(record=np.abs(rng.normal(size=(n_steps, 1, 8))))
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        q, side = int(gains["en_surface"][0]), int(gains["en_side"][0])
        chan = np.full(S, -1, np.int32)
        chan[q] = 0
        with pytest.raises(HeatError) as e:                                  # a receiver with a channel
            b.march_series(w, n_sub, channel=np.zeros((n_steps, 1)), sky=sky, gains=gains, **{SOLAR[side]: chan})
        assert e.value.code == -4 and "entry 0:" in str(e.value)
        scale = gains["ap_scale"].copy()
        scale[6] = np.nan
        with pytest.raises(HeatError) as e:                                  # a scale that is not finite
            b.march_series(w, n_sub, sky=sky, gains=dict(gains, ap_scale=scale))
        assert e.value.code == -1 and "aperture 6:" in str(e.value)
        with pytest.raises(HeatError) as e:                                  # apertures without records
            b.march_series(w, n_sub, gains=gains)
        assert e.value.code == -1 and "aperture 0" in str(e.value)
        # refused before any device work: every slot the batch owns is what was uploaded, to the bit (had a step of one of the
        # three series run, the nodes and the zones would have moved)
        own = owned_slots(md)
        behind = st.copy()
        behind[own] = np.nan
        b.download_state(behind)
        assert np.array_equal(behind[own], st[own])
        # ... and the batch marches good gains afterwards
        trace, failed, transmitted, ap_sum = b.march_series(w, n_sub, probes=md["zone_slot"], sky=sky, gains=gains)
        assert failed == -1 and np.all(np.isfinite(trace)) and np.all(np.isfinite(transmitted)) and (transmitted != 0).any()
        b.download_state(behind)
        assert not np.array_equal(behind[own], st[own])                      # (a series that runs does move them)
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, n_sub, sky=sky, gains=gains)
        assert e.value.code == -1 and "sharded" in str(e.value)
