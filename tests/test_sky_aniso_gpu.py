"""Anisotropic sky of a series on the GPU (include/heat_amd.h, heat_sky_aniso / heat_batch_march_series_call): every sky-driven
solar side, every aperture and every blind takes the diffuse radiation by one coefficient pair per site and step and one band per
consumer, formed on the device beside the 64-byte record.

The rule is this library's own contract; its reference is the rule in numpy (heat_amd/sky.py incident(), solar_gains.py
transmitted(), blinds.py incident_on(), each with aniso=) inside the LOOP WITH FEEDBACK of the blind tests
(sky_aniso_cases.loop). Against that loop through the library's own per-call path the series must be equal bit for bit; against
the same loop through the oracle at the project's rtol = atol = 1e-9. Without an anisotropic sky the struct entry point must be
heat_batch_march_series_blinds exactly. tests/test_sky_aniso_host.py asserts the rule's hand-worked values on the CPU."""
import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, binding, blinds as bl, modeldict as mdl
import blinds_cases as bc
import shades_cases as sc
import sky_aniso_cases as ac
import ambient_cases
from test_blinds_gpu import MARGIN, SMALL, sites_case, weather_of
from test_series_all_terms_gpu import everything, named, same
from test_series_gpu import MODELS, assert_close, owned_slots, probes_of_every_kind, zone_terms, _id
from test_sky_gpu import OPTIONS, SKY_MODELS

pytestmark = pytest.mark.gpu

N_STEPS = ac.N_STEPS


def kwargs(c, probes, a0=None, b0=None, steps=slice(None), ap_sum=None, carry=None, **more):
    return bc.blinded_kwargs(c, probes, a0, b0, steps, ap_sum, carry=carry, aniso=ac.aniso_kwargs(c, steps), **more)


def same_series(ref, want_state, c, out, got_state, own, what):
    """A loop's result against (trace, failed, transmitted, ap_sum, sunlit, blinds) of a series, bit for bit."""
    trace, failed, transmitted, ap_sum, sunlit, blinds = out
    assert failed == -1
    bc.same_blinds(ref, blinds, what + ": ")
    assert np.array_equal(c.f, sunlit), "%s: sunlit keeps the geometric fraction" % what
    assert np.array_equal(ref["transmitted"], transmitted), "%s: %d transmitted powers differ" % (what, int((ref["transmitted"] != transmitted).sum()))
    assert np.array_equal(ref["ap_sum"], ap_sum), "%s: aperture sums differ" % what
    assert np.array_equal(ref["trace"], trace), "%s: %d trace values differ, worst %.3e" % (
        what, int((ref["trace"] != trace).sum()), np.abs(ref["trace"] - trace).max())
    assert np.array_equal(want_state[own], got_state[own]), "%s: %d state slots differ" % (what, int((want_state[own] != got_state[own]).sum()))


# ---- 1. bit for bit against the per-call loop with feedback ----
@pytest.mark.parametrize("opts", OPTIONS + [dict(fuse_always=True)], ids=_id)
@pytest.mark.parametrize("model", SMALL)
def test_anisotropic_series_equals_the_per_call_loop_bit_for_bit(model, opts):
    md, st = SKY_MODELS[model]()
    own = owned_slots(md)
    for form, n_sub in enumerate((1, 2, 5)):
        rng = np.random.default_rng(570 + n_sub)
        c = ac.aniso_case(md, st, rng)
        probes = probes_of_every_kind(md, rng)
        a0, b0 = zone_terms(md, rng, N_STEPS, form)
        w = weather_of(md, n_sub)
        want = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(want)
            ref = ac.loop(c, want, bc.marcher(b, c, w, a0, b0), probes)
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(got)
            out = b.march_series(w, n_sub, **kwargs(c, probes, a0, b0))
            b.download_state(got)
        same_series(ref, want, c, out, got, own, "n_sub=%d" % n_sub)
        cov = ac.coverage(c, ref)
        print("n_sub=%d: %s" % (n_sub, cov))
        assert ac.covered(cov), cov
        bcov = bc.coverage(c, ref)
        assert bcov["closed"] > 0 and bcov["reopened"] > 0, bcov


# ---- 2. without an anisotropic sky the struct entry point is heat_batch_march_series_blinds ----
def blinds_on(kw):
    """Controlled blinds on every third shade of a call's shades, their thresholds the median and the lower quartile of the
    isotropic irradiance on the shade's plane over the call's steps."""
    shades, rec = kw["shades"], kw["sky"]["record"]
    I = bl.incident_on(shades, rec, sc.sunlit_of(shades, rec))
    shade = np.arange(0, sc.N_SHADES, 3, dtype=np.int32)
    n = len(shade)
    return dict(shade=shade, beam_closed=np.full(n, 0.1), diffuse_closed=np.full(n, 0.4), ground_closed=np.full(n, 0.5),
                irr_close=np.nanquantile(I[:, shade], 0.5, axis=0), irr_open=np.nanquantile(I[:, shade], 0.25, axis=0))


@pytest.mark.parametrize("name,with_ideal", [("clustered_massive-fuse_always", False), ("ragged_mixed-planned", True)], ids=["fused", "streamed-ideal"])
def test_the_struct_entry_point_without_aniso_is_the_widest_positional_one(name, with_ideal):
    c = ambient_cases.case(name)
    md = c.md
    own = owned_slots(md)
    kw = everything(name, with_ideal)()
    kw["blinds"] = blinds_on(kw)
    S, NA = int(md["n_surfaces"]), len(kw["gains"]["ap_surface"])
    rng = np.random.default_rng(581)
    zeros = dict(coef=np.zeros((c.n_steps, 1, 2)), front_band=rng.random(S), back_band=rng.random(S), aperture_band=rng.random(NA),
                 shade_band=rng.random(sc.N_SHADES))
    moved = dict(zeros, coef=np.full((c.n_steps, 1, 2), 0.3))
    runs = {}
    for key, aniso in (("positional", None), ("struct", {}), ("zeros", zeros), ("moved", moved)):
        state = c.state.copy()
        with HeatBatch(md, **c.opts) as b:
            b.upload_state(state)
            out = b.march_series(c.weather, c.n_sub, aniso=aniso, **kw)
            b.download_state(state)
        out = out if isinstance(out, dict) else named(out[:13]) | dict(blinds=out[13])
        assert out["failed_step"] == -1, key
        runs[key] = (out, state)

    def flat(out):
        for k, v in sorted(out.items()):
            if isinstance(v, dict):
                for k2, v2 in sorted(v.items()):
                    yield k + "." + k2, np.asarray(v2)
            else:
                yield k, np.asarray(v)

    want, want_state = runs["positional"]
    assert want["blinds"]["position"].any() and not want["blinds"]["position"].all() and want["transmitted"].any()
    got, got_state = runs["struct"]
    for (k, a), (k2, b2) in zip(flat(want), flat(got)):
        assert k == k2 and same(a, b2), "aniso == NULL: %s differs" % k
    assert same(want_state, got_state)
    # all-zero coefficients and random bands: the isotropic values (the sign of a zero aside)
    got, got_state = runs["zeros"]
    for (k, a), (k2, b2) in zip(flat(want), flat(got)):
        assert k == k2 and a.shape == b2.shape and np.array_equal(a, b2, equal_nan=a.dtype.kind == "f"), "zero coefficients: %s differs" % k
    assert np.array_equal(want_state[own], got_state[own])
    # ... and the case discriminates: coefficients that are not zero move what the windows transmit and what the blinds see
    got, _ = runs["moved"]
    assert not np.array_equal(want["transmitted"], got["transmitted"]) and not np.array_equal(want["blinds"]["incident"], got["blinds"]["incident"])
    assert not np.array_equal(want["trace"], got["trace"])


# ---- 3. weather sites against the oracle loop ----
def test_anisotropic_series_of_weather_sites_matches_the_oracle_loop(oracle):
    md, site, state, cases, kw = sites_case(seed=518)
    K, n_sub = len(cases), 3
    rng = np.random.default_rng(519)
    for c, _, _ in cases:
        ac.widen(c, rng)
    kw = dict(kw, aniso=dict(coef=np.concatenate([c.coef for c, _, _ in cases], axis=1),
                             **{k: np.concatenate([c.bands[k] for c, _, _ in cases]) for k in ac.BANDS}))
    assert len(set(tuple(kw["aniso"]["coef"][:, k, 0]) for k in range(K))) == K                 # every site has coefficients of its own
    w = mdl.weather_sites(N_STEPS * n_sub, 45.0, K, seed=2).reshape(N_STEPS, n_sub, K, 3)
    refs, states, iters = [], [], []
    for k, (c, pr, (ta, tb)) in enumerate(cases):
        s = c.state.copy()
        refs.append(ac.loop(c, s, bc.oracle_marcher(oracle.OracleModel(c.md), w[:, :, k, :], ta, tb, iters), pr))
        states.append(s)
        assert ac.covered(ac.coverage(c, refs[-1]))
    ref = {key: np.concatenate([r[key] for r in refs], axis=-1) for key in ("trace", "position", "incident", "transmitted", "ap_sum")}
    ref_state = np.concatenate(states)
    # a site whose every comparison is further than MARGIN from a tie: its decisions cannot differ between device and oracle
    sure = np.concatenate([np.full(bc.N_BLINDS, r["margin"]["I"] > MARGIN and r["margin"]["T"] > MARGIN) for r in refs])
    print("margins of the oracle loops: %s; positions compared exactly at %d of %d sites" % (
        [r["margin"] for r in refs], int(sure.sum()) // bc.N_BLINDS, K))
    assert sure.any()
    own = owned_slots(md)
    for opts in (dict(), dict(use_graph=True), dict(fuse_always=True)):
        got = state.copy()
        with HeatBatch(md, sites=site, **opts) as b:
            b.upload_state(got)
            trace, failed, transmitted, ap_sum, sunlit, blinds = b.march_series(w, n_sub, **kw)
            b.download_state(got)
            assert b.nomass_iterations() == sum(iters)
        assert failed == -1
        # exactly: the irradiance on the shades' planes (it depends on no zone) and the positions of the sure sites
        assert np.array_equal(ref["incident"], blinds["incident"]), "sites %s: %d irradiances differ" % (
            _id(opts), int((ref["incident"] != blinds["incident"]).sum()))
        assert np.array_equal(ref["position"][:, sure], blinds["position"][:, sure], equal_nan=True)
        assert_close(ref["transmitted"], transmitted, "anisotropic sites transmitted %s" % _id(opts))
        assert_close(ref["ap_sum"], ap_sum, "anisotropic sites ap_sum %s" % _id(opts))
        assert_close(ref["trace"], trace, "anisotropic sites trace %s" % _id(opts))
        assert_close(ref_state[own], got[own], "anisotropic sites final state %s" % _id(opts))


# ---- 4. the rule has no memory ----
@pytest.mark.parametrize("opts", [dict(), dict(use_graph=True)], ids=_id)
def test_anisotropic_series_cut_in_two_equals_the_series_in_one(opts):
    md, st = MODELS["rooms_with_windows"]()
    rng = np.random.default_rng(512)
    n_sub, cut = 3, 7
    c = ac.aniso_case(md, st, rng)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, N_STEPS, 2)
    w = weather_of(md, n_sub)
    one, two = st.copy(), st.copy()
    with HeatBatch(md, **opts) as b:
        b.upload_state(one)
        t1, _, p1, sum1, f1, bl1 = b.march_series(w, n_sub, **kwargs(c, probes, a0, b0))
        b.download_state(one)
    with HeatBatch(md, **opts) as b:
        b.upload_state(two)
        ta, _, pa, sum_a, fa, bla = b.march_series(w[:cut], n_sub, **kwargs(c, probes, a0, b0, slice(0, cut)))
        tb, _, pb, sum_b, fb, blb = b.march_series(w[cut:], n_sub, **kwargs(c, probes, a0, b0, slice(cut, None), sum_a, carry=bla))
        b.download_state(two)
    assert np.array_equal(t1, np.concatenate([ta, tb])) and np.array_equal(p1, np.concatenate([pa, pb])) and np.array_equal(f1, np.concatenate([fa, fb]))
    for key in ("position", "incident"):
        assert np.array_equal(bl1[key], np.concatenate([bla[key], blb[key]]), equal_nan=True), key
    for key in ("state",) + bc.ACC:
        assert np.array_equal(bl1[key], blb[key]), key
    assert np.array_equal(sum1, sum_b) and np.array_equal(one, two)
    assert np.array_equal(bl1["incident"], c.I[:, c.blinds["shade"]]) and not np.array_equal(bl1["incident"], c.I_iso[:, c.blinds["shade"]])


# ---- 5. refusals through the batch ----
def test_bad_anisotropic_skies_and_sharded_batches_are_refused_by_the_march():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    S = int(md["n_surfaces"])
    rng = np.random.default_rng(529)
    n_steps, n_sub = 3, 1
    w = np.zeros((n_steps, n_sub, 3))
    mode = np.zeros(S, np.uint8)
    mode[::2] = 1                                                            # the fronts of the even surfaces are sky-driven
    sky = dict(record=np.abs(rng.normal(size=(n_steps, 1, 8))), mode=mode)
    normal = (np.zeros(10), -np.ones(10), np.zeros(10))
    right, up = sc.shading.frame_of(normal)
    front = np.full(S, -1, np.int32)
    front[::2] = np.arange(0, S, 2) % 10
    shades = dict(surface=np.arange(10) * 17, normal=normal, right=right, up=up, width=np.full(10, 1.2), height=np.full(10, 1.5),
                  overhang_depth=np.full(10, 0.6), overhang_gap=np.full(10, 0.2), front_shade=front)
    gains = dict(ap_surface=np.array([4, 40]), ap_normal=(np.zeros(2), -np.ones(2), np.zeros(2)), ap_tau_coef=np.full((2, 6), 0.1),
                 ap_tau_diffuse=np.full(2, 0.5), ap_scale=np.ones(2))
    aniso = dict(coef=rng.uniform(0.1, 0.5, (n_steps, 1, 2)), front_band=rng.random(S), back_band=rng.random(S), aperture_band=rng.random(2),
                 shade_band=rng.random(10))

    def damaged(key, at, v):
        a = aniso[key].copy()
        a[at] = v
        return dict(aniso, **{key: a})

    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        common = dict(sky=sky, shades=shades, gains=gains)
        for kw, who in ((dict(common, aniso=damaged("front_band", 6, np.nan)), "surface 6:"),
                        (dict(common, aniso=damaged("front_band", 198, -0.5)), "surface 198:"),
                        (dict(common, aniso=damaged("aperture_band", 1, np.inf)), "aperture 1:"),
                        (dict(common, aniso=damaged("shade_band", 9, -1e-9)), "shade 9:"),
                        (dict(common, aniso=dict(aniso, coef=None)), "coef is NULL"),
                        (dict(sky=sky, shades=shades, aniso=aniso), "aperture_band"),
                        (dict(sky=sky, aniso={k: v for k, v in aniso.items() if k != "aperture_band"}), "shade_band"),
                        (dict(aniso={k: aniso[k] for k in ("coef", "front_band")}), "sky is NULL"),
                        (dict(sky=dict(record=None, mode=np.zeros(S, np.uint8)), aniso={k: aniso[k] for k in ("coef", "front_band")}), "sky->record is NULL")):
            with pytest.raises(HeatError) as e:
                b.march_series(w, n_sub, **kw)
            assert e.value.code == -1 and who in str(e.value), (who, str(e.value))
        s, _ = binding.make_series(w, n_sub)
        call = binding.SeriesCall(size=8, s=binding.C.pointer(s))
        assert b._L.heat_batch_march_series_call(b._h, binding.C.byref(call)) == -1 and "size 8" in b._L.heat_last_error().decode()
        # refused before any device work: every slot the batch owns is what was uploaded, to the bit
        own = owned_slots(md)
        behind = st.copy()
        behind[own] = np.nan
        b.download_state(behind)
        assert np.array_equal(behind[own], st[own])
        # ... and the batch marches a good anisotropic sky afterwards
        # (no back is sky-driven, no front of an odd surface: their bands are not read)
        good = dict(damaged("back_band", 6, np.nan), front_band=damaged("front_band", 7, -1.0)["front_band"])
        trace, failed, transmitted, ap_sum, sunlit = b.march_series(w, n_sub, probes=md["zone_slot"], sky=sky, shades=shades, gains=gains, aniso=good)
        assert failed == -1 and np.all(np.isfinite(trace)) and np.all(np.isfinite(transmitted)) and transmitted.shape == (n_steps, 2)
        b.download_state(behind)
        assert not np.array_equal(behind[own], st[own])                      # (a series that runs does move them)
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, n_sub, sky=sky, shades=shades, aniso={k: v for k, v in aniso.items() if k != "aperture_band"})
        assert e.value.code == -1 and "sharded" in str(e.value)


# ---- 6. n_sub == 0 ----
def test_no_sub_timestep_still_sets_the_anisotropic_inputs():
    md, st = MODELS["ragged_mixed"]()
    rng = np.random.default_rng(520)
    c = ac.aniso_case(md, st, rng)
    probes = probes_of_every_kind(md, rng)
    ref = ac.loop(c, st.copy(), lambda state, k: None, probes)               # (nothing marches: the zones stay)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, transmitted, ap_sum, sunlit, blinds = b.march_series(None, 0, n_steps=N_STEPS, **kwargs(c, probes))
    assert failed == -1 and np.array_equal(trace, np.tile(st[probes], (N_STEPS, 1)))
    bc.same_blinds(ref, blinds)
    assert np.array_equal(ref["transmitted"], transmitted) and np.array_equal(ref["ap_sum"], ap_sum) and np.array_equal(c.f, sunlit)
    assert np.array_equal(blinds["incident"], c.I[:, c.blinds["shade"]]) and not np.array_equal(blinds["incident"], c.I_iso[:, c.blinds["shade"]])
