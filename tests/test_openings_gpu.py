"""Openings of a series on the GPU (include/heat_amd.h, heat_batch_march_series_openings): volume flows through windows, doorways
and vents formed at the head of every step from the zone temperatures the device holds, written into derived channels of the
device's copy of the channel table and read from there by the air paths, the zone loads' flows and the species.

The first test holds the one new rounded operation, sqrt, to numpy.sqrt bit for bit on an adversarial set. The expected result of
the others is DEFINED by openings_cases.loop_with_rules — heat_amd.openings.apply (the header's contract in numpy, one rounded
operation per line) and then the existing terms' rules on the row with its derived columns, applied between per-step march calls
to the zone temperatures the call before returned: through heat_batch_march_ex the series must agree bit for bit, through
OracleModel.march (≙ ThermalModel::march, src/model.rs:359-427) at rtol = atol = 1e-9, the project's parity bound, with the
discrete outputs equal. tests/test_openings_host.py runs the same cases through the oracle alone and asserts that the flows
respond, that controlled paths open and close and that no controller decision comes within 1e-6 K of its threshold. The rule is
this project's own: the reference has no counterpart (model.rs:546,592-593).

20 zones are 30 openings, less than a wavefront; 500 zones 750: two full workgroups of 256 and a ragged third (750 = 11 * 64 +
46); the sqrt test runs 700 (two full workgroups and a tail of 188 = 2 * 64 + 60)."""
import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, air_species as asp, binding, modeldict as mdl, openings as opn
import air_species_cases as asc
import openings_cases as oc
from air_handlers_cases import handlers_with
from test_series_gpu import assert_close, owned_slots, series_kwargs, _id

pytestmark = pytest.mark.gpu

OPTIONS = [dict(), dict(use_graph=True), dict(no_fusion=True)]
LARGE = "rooms_with_windows_large"
N_STEPS = oc.N_STEPS
NAMES = ("trace", "failed_step", "applied", "modes", "air", "handlers", "species", "openings")


def kwargs(c, steps=slice(None)):
    return series_kwargs(c["channel"], c["drives"], c["probes"], c["a0"], c["b0"], steps=steps)


def series(c, opts, openings="case", steps=slice(None), state=None, carry=None, step_base=0, **more):
    """One series with the case's loads, air paths, handlers, species and `openings` on a fresh batch, resumed from `carry` (a
    loop's, or carried() of a series). Returns (the named result, the final state)."""
    got = c["st"].copy() if state is None else state.copy()
    openings = c["openings"] if isinstance(openings, str) else openings
    loads, air, handlers, species = c["loads"], c["air"], c["handlers"], c["species"]
    if carry:
        loads = dict(loads, thermostats=dict(loads["thermostats"], mode=carry["modes"]))
        air = dict(air, **{k: carry["air"][k] for k in asc.AIR_ACC})
        handlers = handlers_with(handlers, carry["handlers"])
        species = asc.species_with(species, carry["species"], step_base)
        if openings is not None:
            openings = oc.openings_with(openings, carry["openings"], step_base)
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(got)
        out = b.march_series(c["w"][steps], c["n_sub"], loads=loads, air=air, handlers=handlers, species=species, openings=openings,
                             **dict(kwargs(c, steps), **more))
        b.download_state(got)
    names = NAMES if openings is not None else NAMES[:-1]
    assert len(out) == len(names)
    out = dict(zip(names, out))
    assert out["failed_step"] == -1
    return out, got


def carried(got):
    return dict(modes=got["modes"], air={k: got["air"][k] for k in asc.AIR_ACC}, handlers={k: v for k, v in got["handlers"].items() if v.ndim == 1},
                species={k: got["species"][k] for k in ("conc",) + asp.ACC}, openings={k: got["openings"][k] for k in opn.ACC})


def same(ref, got, what, close=None):
    """A loop's result against a series': the discrete outputs exactly; the rows and sums bit for bit, or through close."""
    def value(r, g, name):
        if close is None:
            assert np.array_equal(r, g, equal_nan=True), "%s %s: %d differ, worst %.3e" % (what, name, int((r != g).sum()), np.nanmax(np.abs(r - g)))
        else:
            close(r, g, "%s %s" % (what, name))

    acc = ref["carry"]
    assert np.array_equal(acc["openings"]["step_max"], got["openings"]["step_max"]), "%s step_max" % what
    for key in asc.DISCRETE:
        assert np.array_equal(acc["species"][key], got["species"][key]), "%s %s" % (what, key)
    assert np.array_equal(acc["modes"], got["modes"]), "%s modes" % what
    for key in ("state", "steps_open", "switches"):
        assert np.array_equal(acc["air"][key], got["air"][key]), "%s air %s: %d differ" % (what, key, int((acc["air"][key] != got["air"][key]).sum()))
    value(ref["opening_v"], got["openings"]["opening_v"], "opening_v")
    value(acc["openings"]["sum_v"], got["openings"]["sum_v"], "sum_v")
    value(acc["openings"]["max_v"], got["openings"]["max_v"], "max_v")
    value(ref["path_q"], got["air"]["path_q"], "path_q")
    value(ref["applied"], got["applied"], "applied")
    value(ref["branch_q"], got["handlers"]["branch_q"], "branch_q")
    for key in asp.ROWS:
        value(ref[key], got["species"][key], key)
    for key in asc.REAL:
        value(acc["species"][key], got["species"][key], key)
    value(ref["trace"], got["trace"], "trace")


# ---- 1. sqrt on the device ----
def adversarial_radicands(n=700):
    """Where a sqrt that is not correctly rounded goes wrong first: perfect squares and their two neighbours (the root of the
    lower neighbour must round down to just below an integer), 4^n and 2 4^n — the two ends of the mantissa's range, where the
    seed's relative error and the result's ulp change — one ulp either side across the exponent range, the smallest normal and
    subnormals (the scaled path), the top of the range (no overflow inside), 0.0, and seeded random mantissas at random
    exponents. All finite and >= 0: each is a valid c0."""
    rng = np.random.default_rng(2026)
    k = np.concatenate([np.arange(1.0, 21.0), rng.integers(21, 2 ** 26, 40).astype(np.float64)])
    sq = k * k
    assert (sq < 2.0 ** 53).all()                                            # exact squares
    tiny, big = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    e = np.arange(-510, 511, 34, dtype=np.float64)
    p4, p24 = 4.0 ** e, 2.0 * 4.0 ** e
    sub = np.array([5e-324, 1e-323, 1.5e-323, 4.9e-322, 1e-310, 2.2250738585072009e-308, tiny / 4.0, tiny / 2.0 ** 30, tiny / 2.0 ** 51])
    edge = np.array([0.0, tiny, np.nextafter(tiny, 1.0), np.nextafter(tiny, 0.0), big, np.nextafter(big, 0.0), big / 2.0, big / 4.0, np.nextafter(big / 4.0, 0.0),
                     1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 2.0, np.nextafter(2.0, 1.0), np.nextafter(2.0, 3.0), 0.01])
    fixed = np.concatenate([sq, np.nextafter(sq, 0.0), np.nextafter(sq, np.inf), p4, np.nextafter(p4, 0.0), np.nextafter(p4, np.inf),
                            p24, np.nextafter(p24, 0.0), np.nextafter(p24, np.inf), sub, edge])
    m = n - len(fixed)
    assert m >= 200
    rand = np.ldexp(rng.uniform(1.0, 2.0, m), rng.integers(-1022, 1023, m))
    x = np.concatenate([fixed, rand])
    assert len(x) == n and np.isfinite(x).all() and (x >= 0.0).all()
    return rng.permutation(x)


def test_sqrt_on_the_device_equals_numpy_sqrt_bit_for_bit():
    """700 openings between the two zones of a small model with cw = cs = ca = 0 and area = 1: y == c0[i] exactly and
    V == sqrt(c0[i]). numpy.sqrt is the correctly rounded root (IEEE 754 requires it of the hardware instruction numpy uses)."""
    md, st = mdl.clustered_massive(64, Z=2, seed=3)
    n = 700
    c0 = adversarial_radicands(n)
    op = dict(zone_a=np.zeros(n, np.int32), zone_b=np.ones(n, np.int32), out_chan=np.arange(n), area=np.ones(n), cw=np.zeros(n), cs=np.zeros(n),
              ca=np.zeros(n), c0=c0)
    want = np.sqrt(c0)
    assert np.array_equal(opn.apply(st[md["zone_slot"]], np.zeros(n), op)[1], want)          # the rule on the host: y == c0
    w = mdl.weather_series(2, md["dt"]).reshape(2, 1, 3)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, got = b.march_series(w, 1, channel=np.full((2, n), np.nan), probes=md["zone_slot"], openings=op)
    assert failed == -1
    v = got["opening_v"]
    wrong = np.flatnonzero(v[0].view(np.uint64) != want.view(np.uint64))
    print("sqrt: %d radicands, %d differ from numpy.sqrt%s" % (n, len(wrong), "".join(
        "\n  sqrt(%r) = %r, numpy %r" % (float(c0[i]), float(v[0, i]), float(want[i])) for i in wrong[:10])))
    assert len(wrong) == 0
    assert np.array_equal(v[1].view(np.uint64), want.view(np.uint64))
    assert np.array_equal(got["max_v"], want) and np.array_equal(got["sum_v"], (0.0 + want) + want) and (got["step_max"] == 0).all()


# ---- 2. bit for bit against the per-call loop ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", [("ragged_mixed", 2), ("ragged_mixed", 5), (LARGE, 2), (LARGE, 5)])
def test_series_with_openings_equals_the_per_call_path_bit_for_bit(model, n_sub, opts):
    c = oc.case(model, N_STEPS, n_sub, 2, oc.SEED, floor=False)
    n = opn.n_openings(c["openings"])
    assert (n == 30 and model == "ragged_mixed") or (n == 750 and model == LARGE)
    assert (np.asarray(c["openings"]["c0"]) == 0.0).sum() >= n // 3
    own = owned_slots(c["md"])
    ref_state = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(ref_state)
        ref = oc.loop_with_rules(lambda s, wk, za, zb: b.march(s, wk, za, zb, outputs=b.OUT_ALL), c, ref_state)
    oc.assert_coverage(oc.coverage(c, ref), "%s n_sub=%d (per-call path)" % (model, n_sub))
    got, state = series(c, opts)
    same(ref, got, model)
    assert np.array_equal(ref_state[own], state[own]), "%d state slots differ" % int((ref_state[own] != state[own]).sum())


# ---- 3. the oracle loop ----
_ORACLE_LOOPS = {}


def oracle_loop(oracle, model, n_sub):
    c = oc.case(model, N_STEPS, n_sub, 2, oc.SEED)
    if (model, n_sub) not in _ORACLE_LOOPS:  # (the same for every option set; left unchanged)
        m = oracle.OracleModel(c["md"])

        def march(s, wk, za, zb):
            assert m.march(s, wk, za, zb, threads=1)[0] == 0

        state = c["st"].copy()
        _ORACLE_LOOPS[(model, n_sub)] = (oc.loop_with_rules(march, c, state), state)
    return (c,) + _ORACLE_LOOPS[(model, n_sub)]


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", oc.ORACLE_CASES)
def test_series_with_openings_matches_the_oracle_loop(oracle, model, n_sub, opts):
    """rtol = atol = 1e-9 on the cases whose controller decisions keep 1e-6 K from their thresholds in the oracle loop
    (tests/test_openings_host.py asserts it; the assertion is repeated here on the loop this test compares against). Every
    opening has c0 >= 0.01: with c0 = 0 the flow is proportional to sqrt|dT|, which is not Lipschitz at dT = 0 — a 1e-9 K
    difference in temperatures becomes 3e-5 in V — so no bound on the temperatures bounds V there; with c0 >= 0.01 dV / dT is
    at most area * (cs / Tm + ca) / (2 * 0.1), about 0.05 m3/s per K for the cases' doorways."""
    c, ref, ref_state = oracle_loop(oracle, model, n_sub)
    assert (np.asarray(c["openings"]["c0"]) >= 0.01).all() and oc.margin(c, ref) >= oc.MARGIN
    oc.assert_coverage(oc.coverage(c, ref), "%s n_sub=%d (oracle loop)" % (model, n_sub))
    got, state = series(c, opts)
    same(ref, got, model, close=assert_close)
    own = owned_slots(c["md"])
    assert_close(ref_state[own], state[own], "%s final state" % model)


# ---- 4. cut ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("cut", [7, 16])
def test_series_with_openings_cut_in_two_equals_the_series_in_one(cut, opts):
    c = oc.case("rooms_with_windows", N_STEPS, 2, 2, oc.SEED, floor=False)
    one, state1 = series(c, opts)
    first, mid = series(c, opts, steps=slice(0, cut))
    second, state2 = series(c, opts, steps=slice(cut, None), state=mid, carry=carried(first), step_base=cut)
    assert (one["openings"]["step_max"] >= cut).any() and (one["openings"]["step_max"] < cut).any() and first["air"]["state"].any()
    assert np.array_equal(one["trace"], np.concatenate([first["trace"], second["trace"]]))
    assert np.array_equal(one["openings"]["opening_v"], np.concatenate([first["openings"]["opening_v"], second["openings"]["opening_v"]]))
    assert np.array_equal(one["air"]["path_q"], np.concatenate([first["air"]["path_q"], second["air"]["path_q"]]))
    for key in opn.ACC:
        assert np.array_equal(one["openings"][key], second["openings"][key]), key
    for key in ("conc",) + asp.ACC:
        assert np.array_equal(one["species"][key], second["species"][key]), key
    assert np.array_equal(one["modes"], second["modes"]) and np.array_equal(one["air"]["state"], second["air"]["state"])
    assert np.array_equal(state1, state2)


# ---- 5. no openings ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_no_openings_is_the_series_with_species_bit_for_bit(opts):
    c = asc.case("rooms_with_windows", 12, 3, 2, 5)
    C, dp = binding.C, binding._dp
    results = []
    for how in ("plain", "empty", "null"):
        state = c["st"].copy()
        with HeatBatch(c["md"], **opts) as b:
            b.upload_state(state)
            terms = dict(loads=c["loads"], air=c["air"], handlers=c["handlers"], species=c["species"])
            if how == "plain":
                trace, failed, applied, modes, air, hd, sp = b.march_series(c["w"], 3, **terms, **kwargs(c))
            elif how == "empty":
                trace, failed, applied, modes, air, hd, sp, op = b.march_series(c["w"], 3, openings={}, **terms, **kwargs(c))
                assert op["opening_v"].shape == (12, 0) and op["sum_v"].size == 0
            else:  # op == NULL through the C ABI
                s, keep = binding.make_series(c["w"], 3, **kwargs(c))
                l, lkeep = binding.make_zone_loads(**c["loads"])
                a, akeep = binding.make_air_paths(**c["air"])
                h, hkeep = binding.make_air_handlers(**c["handlers"])
                spc, spkeep = binding.make_air_species(**c["species"])
                Z = int(c["md"]["n_zones"])
                trace, applied, f = np.zeros((12, len(c["probes"]))), np.zeros((12, l.n_thermostats)), C.c_int32(7)
                path_q, branch_q, conc_rows = np.zeros((12, a.n_paths)), np.zeros((12, h.n_branches)), np.zeros((12, spc.n_species, Z))
                call = binding.SeriesCall(size=C.sizeof(binding.SeriesCall), s=C.pointer(s), l=C.pointer(l), air=C.pointer(a), failed_step=C.pointer(f),
                                          trace=trace.ctypes.data_as(dp), applied=applied.ctypes.data_as(dp), path_q=path_q.ctypes.data_as(dp))
                assert b._L.heat_batch_march_series_openings(b._h, C.byref(call), None, None, None, C.byref(h), None, None, None,
                                                             branch_q.ctypes.data_as(dp), C.byref(spc), conc_rows.ctypes.data_as(dp), None, None,
                                                             None, None) == 0
                failed, modes = f.value, lkeep["th_mode"]
                air = dict(path_q=path_q, **{k: akeep[k] for k in asc.AIR_ACC})
                hd = dict(branch_q=branch_q, bypass=hkeep["bypass"])
                sp = dict(conc_rows=conc_rows, **{k: spkeep[k] for k in ("conc",) + asp.ACC})
            b.download_state(state)
        assert failed == -1
        results.append((trace, applied, modes, state, hd["branch_q"], hd["bypass"], sp["conc_rows"]) + tuple(sp[k] for k in ("conc",) + asp.ACC) +
                       tuple(air[k] for k in ("path_q",) + asc.AIR_ACC))
    for other in results[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(results[0], other))


# ---- 6. nullable outputs ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_an_array_that_is_not_asked_for_changes_no_bit_of_the_others(opts):
    c = oc.case("ragged_mixed", N_STEPS, 2, 2, oc.SEED, floor=False)
    full, state = series(c, opts)
    n = opn.n_openings(c["openings"])
    # (step_max follows max_v: it is kept where max_v is)
    for stats, rows in ((("sum_v",), False), (("max_v",), False), (("max_v", "step_max"), False), ((), True), ((), False), (binding.OPENING_STATS, False)):
        got, st = series(c, opts, openings=dict(c["openings"], stats=stats), opening_v=rows)
        assert set(got["openings"]) == {"opening_v"} | set(stats)
        assert got["openings"]["opening_v"].shape == ((N_STEPS if rows else 0), n)
        for key, v in got["openings"].items():
            if v.size:
                assert np.array_equal(v, full["openings"][key]), (stats, rows, key)
        assert np.array_equal(got["trace"], full["trace"]) and np.array_equal(got["applied"], full["applied"]) and np.array_equal(st, state)
        assert np.array_equal(got["air"]["path_q"], full["air"]["path_q"]) and np.array_equal(got["species"]["conc_rows"], full["species"]["conc_rows"])


# ---- 7. refusals ----
def test_bad_openings_and_sharded_batches_are_refused_and_leave_the_device_untouched():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    w, channel = np.zeros((2, 1, 3)), np.zeros((2, 6))
    ok = dict(zone_a=[1, 2], zone_b=[-1, 3], temp_chan=[0, -1], wind_chan=[1, -1], frac_chan=[2, -1], out_chan=[4, 5], area=[0.5, 0.5], cs=[9.0, 9.0],
              c0=[0.01, 0.01])
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        for bad, code, needle in ((dict(ok, zone_a=[8, 2]), -4, "opening 0:"),
                                  (dict(ok, zone_b=[-1, 2]), -1, "opening 1:"),
                                  (dict(ok, out_chan=[4, 6]), -4, "opening 1:"),
                                  (dict(ok, out_chan=[4, 4]), -4, "opening 1:"),
                                  (dict(ok, temp_chan=[-1, -1]), -4, "opening 0:"),
                                  (dict(ok, temp_chan=[0, 0]), -4, "opening 1:"),
                                  (dict(ok, wind_chan=[5, -1]), -4, "opening 0:"),
                                  (dict(ok, area=[0.5, -0.5]), -1, "opening 1:"),
                                  (dict(ok, c0=[np.nan, 0.01]), -1, "opening 0:"),
                                  (dict(ok, cs=[9.0, np.inf]), -1, "opening 1:")):
            with pytest.raises(HeatError) as e:
                b.march_series(w, 1, channel=channel, openings=bad)
            assert e.value.code == code and needle in str(e.value), str(e.value)
        got = st.copy()
        own = owned_slots(md)
        got[own] = np.nan                                             # (a download writes the slots the device owns, and only those)
        b.download_state(got)
        assert np.array_equal(got, st)
        # the batch marches on: a good term afterwards
        trace, failed, op = b.march_series(w, 1, channel=channel, openings=ok, probes=md["zone_slot"])
        assert failed == -1 and np.isfinite(op["opening_v"]).all()
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, 1, channel=channel, openings=ok)
        assert e.value.code == -1 and "sharded" in str(e.value)


# ---- 8. a derived channel nothing reads ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_a_derived_channel_read_by_nothing_changes_no_bit_of_the_march(opts):
    c = asc.case("rooms_with_windows", N_STEPS, 2, 2, asc.SEED)
    Z, nc = int(c["md"]["n_zones"]), c["channel"].shape[1]
    terms = dict(loads=c["loads"], air=c["air"], handlers=c["handlers"], species=c["species"])
    plain = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(plain)
        want = b.march_series(c["w"], 2, **terms, **kwargs(c))
        b.download_state(plain)
    # one opening per zone to its neighbour, each writing a column of its own that no consumer names
    wide = dict(c, channel=np.concatenate([c["channel"], np.full((N_STEPS, Z), np.nan)], axis=1))
    op = dict(zone_a=np.arange(Z), zone_b=(np.arange(Z) + 1) % Z, out_chan=nc + np.arange(Z), **opn.doorway(np.full(Z, 0.9), 2.0, 0.6))
    state = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(state)
        got = b.march_series(c["w"], 2, openings=op, **terms, **kwargs(wide))
        b.download_state(state)
    assert len(got) == len(want) + 1 and np.array_equal(plain, state)
    for x, y in zip(want, got):
        for u, v in (zip(x.values(), y.values()) if isinstance(x, dict) else [(x, y)]):
            assert np.array_equal(u, v, equal_nan=True)
    # ... while the openings did respond to the march: V follows the zone temperatures of every step
    v = got[-1]["opening_v"]
    T = np.concatenate([c["st"][c["md"]["zone_slot"]][None, :], got[0][:-1, -Z:]])      # (the cases' last probes are the zones)
    want_v = np.array([opn.apply(T[k], wide["channel"][k], op)[1] for k in range(N_STEPS)])
    assert np.array_equal(v, want_v) and (v.max(axis=0) > v.min(axis=0)).all()


# ---- 9. no sub-timestep; NaN ----
def test_a_series_of_no_sub_timestep_still_evaluates_the_openings():
    c = oc.case("ragged_mixed", 6, 0, 2, 21, floor=False)
    ref = oc.loop_with_rules(lambda s, wk, za, zb: None, c, c["st"].copy())          # nothing marches: every step sees the start
    state = c["st"].copy()
    with HeatBatch(c["md"]) as b:
        b.upload_state(state)
        got = dict(zip(NAMES, b.march_series(None, 0, n_steps=6, loads=c["loads"], air=c["air"], handlers=c["handlers"], species=c["species"],
                                             openings=c["openings"], **kwargs(c))))
        b.download_state(state)
    assert got["failed_step"] == -1 and np.array_equal(state, c["st"]) and (ref["opening_v"] != 0).any()
    assert np.array_equal(ref["opening_v"], got["openings"]["opening_v"]) and np.array_equal(ref["path_q"], got["air"]["path_q"])
    for key in opn.ACC:
        assert np.array_equal(ref["carry"]["openings"][key], got["openings"][key]), key


def test_a_nan_flow_is_data_until_a_consumer_adds_it_to_a_zone():
    """A NaN open fraction makes V NaN. Read by nothing it stays in its rows and fails nothing; read by an air path it makes the
    target's a0 / b0 NaN, which the path reports as HEAT_N_NAN_ZONE at that step, as it does for a NaN in an ordinary channel."""
    md, st = mdl.clustered_massive(700, Z=28, dt=45.0, seed=3)
    n_steps, j = 9, 5
    channel = np.tile([5.0, 1.0, np.nan], (n_steps, 1))                  # the outside temperature, the open fraction, the derived channel
    channel[j, 1] = np.nan
    op = dict(zone_a=[13], zone_b=[-1], temp_chan=[0], frac_chan=[1], out_chan=[2], area=[0.02], cs=[9.0], c0=[0.01])
    w = mdl.weather_series(n_steps * 2, 45.0).reshape(n_steps, 2, 3)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, got = b.march_series(w, 2, openings=op, channel=channel, probes=md["zone_slot"])
        assert failed == -1 and np.isfinite(trace).all()
        v = got["opening_v"][:, 0]
        assert np.isnan(v[j]) and np.isfinite(np.delete(v, j)).all() and np.isnan(got["sum_v"][0]) and np.isfinite(got["max_v"][0])
        b.upload_state(st.copy())
        with pytest.raises(HeatError) as e:
            b.march_series(w, 2, openings=op, air=dict(target=[13], source=[-1], temp_chan=[0], volume_chan=[2]), channel=channel, probes=md["zone_slot"])
        assert e.value.failed_step == j and e.value.code == 3, str(e.value)   # HEAT_N_NAN_ZONE
        assert b.failed_surface() == (13, 3) and np.all(np.isfinite(e.value.trace[:j]))
