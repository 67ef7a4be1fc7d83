"""Ambient-side temperatures after creation, on the GPU (include/heat_amd.h: heat_batch_set_ambient, heat_ambient_drive /
heat_batch_march_series_ambient).

The setter is held to the oracle: before each march call new temperatures go to the batch through set_ambient and to the
oracle by writing its front_ambient / back_ambient arrays in place; states are compared with the suite's assert_state_close
(1e-9), no-mass pass counts exactly. Each case first shows on the oracle alone that it discriminates
(ambient_cases.discrimination: every driven side, every both-sides-Ambient wall with a driven front; the same is asserted on
the CPU by tests/test_ambient_series_host.py).
The series is held bit for bit to the per-call loop of the library itself — heat_amd/ambient.py's apply() on the zone
temperatures the state holds, set_ambient, one heat_batch_march_ex — and at 1e-9 to the oracle loop with the same rule
between the oracle's marches."""
import ctypes as C

import numpy as np
import pytest

import ambient_cases as ac
from heat_amd import HeatBatch, HeatError, ambient as amb, binding, modeldict as mdl, room_radiation as rrm
from test_parity_gpu import assert_state_close
from test_series_gpu import assert_close, owned_slots
from test_zone_loads_gpu import random_loads

pytestmark = pytest.mark.gpu

ALL = sorted(ac.FAMILIES)


def per_call_loop(b, c, state, drive, steps=None):
    """The path a driven series replaces: per step the rule on the host from the zone temperatures the state holds (what
    the previous call's download left there), the setter, one march call. Returns (trace, ambient_t, sums)."""
    md = c.md
    steps = range(c.n_steps) if steps is None else steps
    trace, ambient_t = np.zeros((len(steps), len(c.probes))), np.zeros((len(steps), len(drive["surface"])))
    total = np.zeros(len(drive["surface"]))
    for i, k in enumerate(steps):
        ac.write_inputs(c, state, k)
        v = amb.apply(drive, c.channel[k], state[md["zone_slot"]])
        b.set_ambient(drive["surface"], drive["side"], v)
        b.march(state, c.weather[k], c.a0, c.b0, outputs=b.OUT_ALL)
        trace[i], ambient_t[i] = state[c.probes], v
        total = total + v
    return trace, ambient_t, total


def reference_loop(c, drive=None):
    want = c.state.copy()
    with HeatBatch(c.md, **c.opts) as b:
        b.upload_state(want)
        out = per_call_loop(b, c, want, c.drive if drive is None else drive)
    return (want,) + out


# ---- 1. the setter against the oracle ----
@pytest.mark.parametrize("name", ALL)
def test_setter_matches_the_oracle(oracle, name):
    c = ac.case(name)
    md = c.md
    assert (c.both & (c.side == 0)).sum() > 10 and (c.both & (c.side == 1)).sum() > 10       # walls Ambient on both sides, driven either way
    ref, iters, sides, walls = ac.discrimination(oracle, c)
    assert sides.all(), "%d of %d driven sides do not tell a driven run from the descriptor's constants" % ((~sides).sum(), len(sides))
    assert len(walls) and walls.all(), "%d of %d walls do not tell a driven front from a driven back alone" % ((~walls).sum(), len(walls))
    got = c.state.copy()
    with HeatBatch(md, **c.opts) as b:
        if c.opts.get("fuse_always"):
            assert b.n_fused_surfaces > 0, b.class_counts()
        b.upload_state(got)
        for k in range(c.n_steps):
            b.set_ambient(c.surface, c.side, c.set_values[k])
            b.march(got, c.weather[k], c.a0, c.b0)
        gpu_iters = b.nomass_iterations()
    assert gpu_iters == iters, "no-mass loop took a different number of passes (%d vs %d)" % (iters, gpu_iters)
    assert_state_close(md, ref, got)


# ---- 2. the series against the per-call loop, bit for bit ----
@pytest.mark.parametrize("name", ALL)
def test_series_equals_the_per_call_loop_bit_for_bit(name):
    c = ac.case(name)
    md = c.md
    mz = c.drive["mix_zone"]
    assert ((mz >= 0) & (mz == c.own_zone)).any() and ((mz >= 0) & (mz == c.far) & (c.far != c.home)).any() and (mz < 0).any()
    if c.cluster:
        assert ((mz >= 0) & (mz // c.cluster != c.home // c.cluster)).any()               # a zone of another cluster
    want, ref_trace, ref_t, ref_sum = reference_loop(c)
    got = c.state.copy()
    with HeatBatch(md, **c.opts) as b:
        b.upload_state(got)
        trace, failed, ambient_t, total = b.march_series(c.weather, c.n_sub, ambient=c.drive, **ac.series_kwargs(c))
        b.download_state(got)
    own = owned_slots(md)
    assert failed == -1 and np.all(np.isfinite(trace))
    assert np.array_equal(ref_t, ambient_t), "%d ambient temperatures differ, worst %.3e" % (
        int((ref_t != ambient_t).sum()), np.abs(ref_t - ambient_t).max())
    assert np.array_equal(ref_sum, total)
    assert np.array_equal(ref_trace, trace), "%d trace values differ, worst %.3e" % (
        int((ref_trace != trace).sum()), np.abs(ref_trace - trace).max())
    assert np.array_equal(want[own], got[own]), "%d state slots differ" % int((want[own] != got[own]).sum())
    mixed = mz >= 0
    assert not np.array_equal(ambient_t[1][mixed], ambient_t[-1][mixed])                  # (the zones move: the rule follows them)


# ---- 3. the series against the oracle loop ----
@pytest.mark.parametrize("name", ac.ORACLE_FAMILIES)
def test_series_matches_the_oracle_loop(oracle, name):
    c = ac.case(name)
    md = c.md
    ref, ref_trace, ref_t, iters = ac.oracle_drive_series(oracle, c)
    got = c.state.copy()
    with HeatBatch(md, **c.opts) as b:
        if c.opts.get("fuse_always"):
            assert b.n_fused_surfaces > 0, b.class_counts()
        b.upload_state(got)
        trace, failed, ambient_t, total = b.march_series(c.weather, c.n_sub, ambient=c.drive, **ac.series_kwargs(c))
        b.download_state(got)
        assert b.nomass_iterations() == iters
    assert failed == -1
    own = owned_slots(md)
    assert_close(ref_trace, trace, "%s trace" % name)
    assert_close(ref[own], got[own], "%s final state" % name)
    assert_close(ref_t, ambient_t, "%s ambient temperatures" % name)
    assert np.array_equal(ref_t[0], ambient_t[0])                                         # (step 0 is formed from the uploaded zones)


# ---- 4. cut, NULL forms, outputs, n_sub == 0 ----
@pytest.mark.parametrize("name", ["ragged_mixed-use_graph", "clustered_massive-fuse_always"])
def test_series_cut_in_two_and_arrays_not_asked_for(name):
    c = ac.case(name)
    md, cut = c.md, 2
    kw = lambda steps=slice(None): ac.series_kwargs(c, steps)
    one, two, none = c.state.copy(), c.state.copy(), c.state.copy()
    with HeatBatch(md, **c.opts) as b:
        b.upload_state(one)
        trace1, _, t1, sum1 = b.march_series(c.weather, c.n_sub, ambient=c.drive, **kw())
        b.download_state(one)
    with HeatBatch(md, **c.opts) as b:
        b.upload_state(two)
        ta, _, t_a, sum_a = b.march_series(c.weather[:cut], c.n_sub, ambient=c.drive, **kw(slice(0, cut)))
        tb, _, t_b, sum_b = b.march_series(c.weather[cut:], c.n_sub, ambient=dict(c.drive, sum_temperature=sum_a), **kw(slice(cut, None)))
        b.download_state(two)
    assert np.array_equal(trace1, np.concatenate([ta, tb])) and np.array_equal(t1, np.concatenate([t_a, t_b]))
    assert np.array_equal(sum1, sum_b) and not np.array_equal(sum_a, sum_b) and np.array_equal(one, two)
    # neither array asked for: no other bit changes
    with HeatBatch(md, **c.opts) as b:
        b.upload_state(none)
        t0, f0, a0, s0 = b.march_series(c.weather, c.n_sub, ambient=dict(c.drive, sum_temperature=False), ambient_t=False, **kw())
        b.download_state(none)
    assert f0 == -1 and a0.shape == (0, len(c.surface)) and s0.shape == (0,)
    assert np.array_equal(t0, trace1) and np.array_equal(none, one)


def test_null_gain_offset_and_mix_equal_the_per_call_loop():
    """The NULL forms: no gain, no offset, no mix_zone (mix NULL too) — and mix_zone given but -1 everywhere with mix NULL."""
    c = ac.case("uniform_massive-n13-npl4")
    md = c.md
    bare = dict(surface=c.surface, side=c.side, chan=c.drive["chan"])
    own = owned_slots(md)
    want, ref_trace, ref_t, ref_sum = reference_loop(c, bare)
    for drive in (bare, dict(bare, mix_zone=np.full(len(c.surface), -1, np.int32))):
        got = c.state.copy()
        with HeatBatch(md, **c.opts) as b:
            b.upload_state(got)
            trace, failed, ambient_t, total = b.march_series(c.weather, c.n_sub, ambient=drive, **ac.series_kwargs(c))
            b.download_state(got)
        assert failed == -1 and np.array_equal(ref_t, ambient_t) and np.array_equal(ref_sum, total)
        assert np.array_equal(ref_trace, trace) and np.array_equal(want[own], got[own])
        assert np.array_equal(ambient_t, c.channel[:, c.drive["chan"]])


def test_absent_and_empty_drive_are_the_call_without_a_drive():
    c = ac.case("ragged_mixed-planned")
    md = c.md
    kw = ac.series_kwargs(c)
    plain = c.state.copy()
    with HeatBatch(md) as b:
        b.upload_state(plain)
        trace, failed = b.march_series(c.weather, c.n_sub, **kw)
        b.download_state(plain)
    assert failed == -1
    same = c.state.copy()
    with HeatBatch(md) as b:
        b.upload_state(same)
        out = b.march_series(c.weather, c.n_sub, ambient={}, **kw)
        b.download_state(same)
    assert np.array_equal(trace, out[0]) and out[1] == -1 and np.array_equal(plain, same)
    assert out[2].shape == (c.n_steps, 0) and out[3].shape == (0,)
    # ambient == NULL through the new entry point: heat_batch_march_series_radiation
    null = c.state.copy()
    with HeatBatch(md) as b:
        b.upload_state(null)
        s, keep = binding.make_series(c.weather, c.n_sub, **kw)
        t1, f1, t_amb = np.zeros_like(trace), C.c_int32(5), np.full((c.n_steps, 3), 7.0)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert b._L.heat_batch_march_series_ambient(b._h, C.byref(s), *(None,) * 7, dp(t1), *(None,) * 7, None, dp(t_amb), C.byref(f1)) == 0
        b.download_state(null)
    assert f1.value == -1 and np.array_equal(trace, t1) and np.array_equal(plain, null) and np.all(t_amb == 7.0)
    # a driven series differs, and leaves its last step's temperatures behind: a plain series after it is NOT the fresh one
    with HeatBatch(md) as b:
        b.upload_state(c.state.copy())
        driven = b.march_series(c.weather, c.n_sub, ambient=c.drive, **kw)
        assert driven[1] == -1 and not np.array_equal(driven[0], trace)
        b.upload_state(c.state.copy())
        after, _ = b.march_series(c.weather, c.n_sub, **kw)
    assert not np.array_equal(after, trace)


def test_no_sub_timestep_still_sets_every_steps_values():
    c = ac.case("glazing_cavity")
    md = c.md
    kw = dict(ac.series_kwargs(c), zone_a0=None, zone_b0=None)
    # the per-call loop with calls of no sub-timestep: the values of the last step stay, then one real call
    want = c.state.copy()
    with HeatBatch(md) as b:
        b.upload_state(want)
        zones = want[md["zone_slot"]].copy()
        for k in range(c.n_steps):
            v = amb.apply(c.drive, c.channel[k], zones)
            b.set_ambient(c.surface, c.side, v)
        b.march(want, c.weather[0], c.a0, c.b0, outputs=b.OUT_ALL)
    got = c.state.copy()
    with HeatBatch(md) as b:
        b.upload_state(got)
        trace, failed, ambient_t, total = b.march_series(None, 0, n_steps=c.n_steps, ambient=c.drive, **kw)
        b.march(got, c.weather[0], c.a0, c.b0, outputs=b.OUT_ALL)
    rows = np.stack([amb.apply(c.drive, c.channel[k], zones) for k in range(c.n_steps)])
    assert failed == -1 and np.array_equal(ambient_t, rows) and not np.array_equal(rows[0], rows[-1])
    assert np.array_equal(trace, np.tile(c.state[c.probes], (c.n_steps, 1)))
    assert np.array_equal(want, got)
    untouched = c.state.copy()
    with HeatBatch(md) as b:                                   # (and the values matter: the descriptor's give another state)
        b.upload_state(untouched)
        b.march(untouched, c.weather[0], c.a0, c.b0, outputs=b.OUT_ALL)
    assert not np.array_equal(untouched, got)


# ---- 5. one combined call ----
def test_drive_with_loads_a_thermostat_an_ideal_load_and_room_radiation():
    """Zone loads with thermostats, ideal loads (they make the series march streamed), room radiation and an ambient drive in
    one call, against the per-call loop: one series of ONE step per call — the same loads, ideal loads and radiation, their
    memories carried (thermostat modes, accumulators, sums), no drive — with the rule on the host and set_ambient before it."""
    c = ac.case("ragged_mixed-planned")
    md, n_steps, n_sub = c.md, c.n_steps, c.n_sub
    S, Z = int(md["n_surfaces"]), int(md["n_zones"])
    rng = np.random.default_rng(77)
    channel, loads = random_loads(md, c.state, rng, n_steps, c.channel)
    t_mid = float(np.median(c.state[md["zone_slot"]]))
    channel = np.concatenate([channel, np.full((n_steps, 1), t_mid + 0.7), np.full((n_steps, 1), t_mid + 1.9)], axis=1)
    nc = channel.shape[1]
    zone = np.arange(0, Z, 2, dtype=np.int32)
    ideal = dict(zone=zone, heat_chan=np.full(len(zone), nc - 2, np.int32), cool_chan=np.full(len(zone), nc - 1, np.int32),
                 heat_cap=np.where(np.arange(len(zone)) % 2 == 0, 2000.0, np.inf), cool_cap=np.full(len(zone), np.inf))
    rad = rrm.exchange_by_area(md)
    inputs = dict(c.inputs)
    for s, key, kind in ((0, "ir_front", "front_kind"), (1, "ir_back", "back_kind")):      # an input has one source
        chan = inputs[key][0].copy()
        chan[md[kind] == mdl.SPACE] = -1
        inputs[key] = (chan, inputs[key][1])
    assert (c.drive["mix_zone"][:, None] == zone[None, :]).any()                        # a side mixes with a zone that is held
    kw = lambda steps: dict(channel=channel[steps], probes=c.probes, zone_a0=c.a0, zone_b0=c.b0, **inputs)
    got = c.state.copy()
    with HeatBatch(md) as b:
        b.upload_state(got)
        out = b.march_series(c.weather, n_sub, loads=loads, ideal=ideal, radiation=rad, ambient=c.drive, **kw(slice(None)))
        b.download_state(got)
    assert out["failed_step"] == -1 and (out["ideal_q"] != 0).any() and (out["applied"] != 0).any() and (out["irradiance"] > 0).all()
    want = c.state.copy()
    rows = {k: [] for k in ("trace", "ideal_q", "applied", "irradiance", "ambient_t")}
    total = np.zeros(len(c.surface))
    with HeatBatch(md) as b:
        b.upload_state(want)
        modes, resume, rsum = None, None, None
        for k in range(n_steps):
            v = amb.apply(c.drive, channel[k], want[md["zone_slot"]])
            b.set_ambient(c.surface, c.side, v)
            step = b.march_series(c.weather[k:k + 1], n_sub,
                                  loads=loads if modes is None else dict(loads, thermostats=dict(loads["thermostats"], mode=modes)),
                                  ideal=ideal if resume is None else dict(ideal, resume=resume, step_base=k),
                                  radiation=rad if rsum is None else dict(rad, sum_irradiance=rsum), **kw(slice(k, k + 1)))
            assert step["failed_step"] == -1
            modes, resume, rsum = step["modes"], step["ideal"], step["sum_irradiance"]
            b.download_state(want)
            for key in ("trace", "ideal_q", "applied", "irradiance"):
                rows[key].append(step[key])
            rows["ambient_t"].append(v[None, :])
            total = total + v
    for key in rows:
        assert np.array_equal(np.concatenate(rows[key]), out[key]), key
    assert np.array_equal(total, out["sum_temperature"]) and np.array_equal(rsum, out["sum_irradiance"])
    assert np.array_equal(modes, out["modes"]) and np.array_equal(want, got)


# ---- 6. durability ----
@pytest.mark.parametrize("name", ["uniform_massive-n32-npl0", "partitioned_buildings-8"])
def test_values_of_the_last_step_survive_an_upload(name):
    c = ac.case(name)
    md = c.md
    # the per-call loop, then: upload, inputs, fusion switched, and one more call without setting anything
    want = c.state.copy()
    with HeatBatch(md, **c.opts) as b:
        b.upload_state(want)
        per_call_loop(b, c, want, c.drive)
        want = c.state.copy()
        b.upload_state(want)
        b.march(want, c.weather[0], c.a0, c.b0, outputs=b.OUT_ALL)
    got = c.state.copy()
    with HeatBatch(md, **c.opts) as b:
        b.upload_state(got)
        _, failed, ambient_t, _ = b.march_series(c.weather, c.n_sub, ambient=c.drive, **ac.series_kwargs(c))
        assert failed == -1
        got = c.state.copy()
        b.upload_state(got)
        b.upload_inputs(got)
        b.set_fusion(False)
        b.set_fusion(True)
        b.march(got, c.weather[0], c.a0, c.b0, outputs=b.OUT_ALL)
    assert np.array_equal(want, got)
    fresh = c.state.copy()
    with HeatBatch(md, **c.opts) as b:
        b.upload_state(fresh)
        b.march(fresh, c.weather[0], c.a0, c.b0, outputs=b.OUT_ALL)
    assert not np.array_equal(fresh, got)                      # (the descriptor's temperatures give another state)


# ---- 7. refusals and failures ----
def test_refusals_on_a_live_batch_leave_the_state_untouched():
    c = ac.case("clustered_massive-fuse_always")
    md = c.md
    S = int(md["n_surfaces"])
    N = len(c.surface)
    i = np.arange(N)
    not_ambient = int(np.flatnonzero(md["back_kind"] != mdl.AMBIENT)[0])
    kw = ac.series_kwargs(c)
    own = owned_slots(md)
    with HeatBatch(md, **c.opts) as b:
        b.upload_state(c.state.copy())
        for bad, code, names in ((dict(surface=np.where(i == 3, not_ambient, c.surface), side=np.where(i == 3, 1, c.side)), -4, "ambient side 3:"),
                                 (dict(surface=np.where(i == 9, c.surface[2], c.surface), side=np.where(i == 9, c.side[2], c.side)), -4, "ambient side 9:"),
                                 (dict(chan=np.where(i == 5, c.channel.shape[1], c.drive["chan"])), -4, "ambient side 5:"),
                                 (dict(surface=np.where(i == 7, S, c.surface)), -4, "ambient side 7:"),
                                 (dict(side=np.where(i == 4, 2, c.side)), -1, "ambient side 4:"),
                                 (dict(gain=np.where(i == 6, np.inf, 1.0)), -1, "ambient side 6:"),
                                 (dict(mix_zone=np.where(i == 8, int(md["n_zones"]), c.drive["mix_zone"]), mix=np.ones(N)), -4, "ambient side 8:")):
            with pytest.raises(HeatError) as e:
                b.march_series(c.weather, c.n_sub, ambient=dict(c.drive, **bad), **kw)
            assert e.value.code == code and names in str(e.value), str(e.value)
        for args, code, names in (((np.array([not_ambient]), np.array([1]), np.array([5.0])), -4, "entry 0"),
                                  ((c.surface[[0, 1, 0]], c.side[[0, 1, 0]], np.zeros(3)), -4, "entry 2"),
                                  ((c.surface[:2], np.array([c.side[0], 3]), np.zeros(2)), -1, "entry 1"),
                                  ((np.array([0, S]) + 0 * c.surface[:2], c.side[:2], np.zeros(2)), -4, "entry")):
            with pytest.raises(HeatError) as e:
                b.set_ambient(*args)
            assert e.value.code == code and names in str(e.value), str(e.value)
        b.set_ambient([], [], [])                              # n == 0 does nothing
        # refused before any device work: every slot the batch owns is what was uploaded, to the bit — and so are the
        # temperatures: a march gives what a fresh batch gives
        behind = c.state.copy()
        behind[own] = np.nan
        b.download_state(behind)
        assert np.array_equal(behind[own], c.state[own])
        b.march(behind, c.weather[0], c.a0, c.b0, outputs=b.OUT_ALL)
    fresh = c.state.copy()
    with HeatBatch(md, **c.opts) as b:
        b.upload_state(fresh)
        b.march(fresh, c.weather[0], c.a0, c.b0, outputs=b.OUT_ALL)
    assert np.array_equal(fresh, behind)
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:                    # (the zones are probed: a shard holds only some of the surfaces)
            b.march_series(c.weather, c.n_sub, ambient=c.drive, **dict(kw, probes=md["zone_slot"]))
        assert e.value.code == -1 and "sharded" in str(e.value)
        with pytest.raises(HeatError) as e:
            b.set_ambient(c.surface[:1], c.side[:1], [1.0])
        assert e.value.code == -1 and "sharded" in str(e.value)


def test_a_nan_channel_fails_like_the_per_call_loop():
    c = ac.case("uniform_massive-n13-npl0")
    md, at = c.md, 3
    channel = c.channel.copy()
    channel[at, 8:] = np.nan
    d = ac.Case()
    d.__dict__.update(c.__dict__)
    d.channel = channel
    want, seen = c.state.copy(), None
    with HeatBatch(md, **c.opts) as b:
        b.upload_state(want)
        for k in range(c.n_steps):
            try:
                per_call_loop(b, d, want, c.drive, [k])
            except HeatError as e:
                seen = (e.code, k)
                break
    print("the per-call loop with a NaN channel at step %d: (code, step) = %s" % (at, seen))
    got = None
    with HeatBatch(md, **c.opts) as b:
        b.upload_state(c.state.copy())
        try:
            b.march_series(c.weather, c.n_sub, ambient=c.drive, **ac.series_kwargs(d))
        except HeatError as e:
            got = (e.code, e.failed_step)
    assert got == seen
