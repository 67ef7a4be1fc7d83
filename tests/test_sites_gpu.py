"""Weather sites on the GPU (include/heat_amd.h, heat_batch_create_sites): a batch of K sites is K reference models marched
in lockstep, each with its own weather (src/model.rs:359-427; the weather reaches the Outdoor sides only: t_out,
model.rs:79-96; wind speed, convection.rs:157-167; wind direction, surface.rs:37-46). Every site's slots are compared with
the oracle's march of that site's own model and weather at rtol = atol = 1e-9."""
import ctypes as C

import numpy as np
import pytest

from heat_amd import HeatBatch, binding, modeldict as mdl

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-9


def assert_state_close(md, ref, got):
    for name, idx in (("nodes", mdl.node_slots(md)), ("hs_front", md["hs_front_slot"]), ("hs_back", md["hs_back_slot"]),
                      ("flow_front", md["flow_front_slot"]), ("flow_back", md["flow_back_slot"]),
                      ("zones", md["zone_slot"])):
        r, g = ref[idx], got[idx]
        err = np.abs(r - g) / (ATOL + RTOL * np.abs(r))
        assert np.all(np.isfinite(g)), name
        assert err.max() <= 1.0 if len(err) else True, "%s: worst |diff| %.3e at %d (ref %.17g, got %.17g)" % (
            name, np.abs(r - g).max(), int(err.argmax()), r[err.argmax()], g[err.argmax()])
    owned = np.zeros(len(ref), dtype=bool)
    for idx in (mdl.node_slots(md), md["hs_front_slot"], md["hs_back_slot"], md["flow_front_slot"],
                md["flow_back_slot"], md["zone_slot"]):
        owned[idx] = True
    assert np.array_equal(ref[~owned], got[~owned], equal_nan=True)


def five_sites(interleave=False):
    parts = [mdl.clustered_massive(240, Z=10, seed=31), mdl.rooms_with_windows(200, Z=10, seed=32),
             mdl.glazing_cavity(80, Z=2, seed=33), mdl.ragged_mixed(150, Z=6, seed=34),
             mdl.partitioned_buildings(192, 10, seed=35)]
    md, site = mdl.concat([m for m, _ in parts], interleave=interleave)
    return parts, md, site, np.concatenate([s for _, s in parts])


def oracle_per_site(oracle, parts, w, threads=1):
    """Each site's own model through the oracle with that site's weather; the states joined as concat joins them."""
    out, iters = [], 0
    for k, (m, st) in enumerate(parts):
        ref = st.copy()
        rc, it = oracle.OracleModel(m).march(ref, w[:, k, :], threads=threads)
        assert rc == 0
        out.append(ref)
        iters += it
    return np.concatenate(out), iters


def run_sites(md, site, state, w, path="march", **kw):
    got = state.copy()
    with HeatBatch(md, sites=site, **kw) as b:
        assert b.n_sites == w.shape[1]
        b.upload_state(got)
        if path == "march":
            b.march(got, w)
        elif path == "resident":
            b.march_resident(w)
            b.synchronize()
            b.download_state(got)
        else:  # split phase: set_weather -> step_surfaces -> step_zones, per sub-timestep
            b.set_weather(w)
            for i in range(w.shape[0]):
                b.step_surfaces(i)
                b.step_zones(None, 1)
            b.synchronize()
            b.download_state(got)
        return got, b.nomass_iterations(), b.n_fused_surfaces, b.n_fused_launches


OPTIONS = [dict(), dict(no_fusion=True), dict(fuse_always=True), dict(force_general=True), dict(nodes_per_lane=4),
           dict(nodes_per_lane=8), dict(nodes_per_lane=16), dict(no_palette=True), dict(use_graph=True)]


@pytest.mark.parametrize("opts", OPTIONS, ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()) or "default")
@pytest.mark.parametrize("n_sub", [1, 2, 7, 20])
def test_independent_sites_match_each_sites_oracle(oracle, opts, n_sub):
    parts, md, site, state = five_sites()
    w = mdl.weather_sites(n_sub, 45.0, 5, seed=n_sub)
    ref, iters = oracle_per_site(oracle, parts, w)
    for path in ("march", "resident", "split"):
        got, gpu_iters, n_fused, _ = run_sites(md, site, state, w, path, **opts)
        assert_state_close(md, ref, got)
        assert gpu_iters == iters, path
        if opts.get("fuse_always") and path != "split":
            assert n_fused > 0


@pytest.mark.parametrize("n_sub", [2, 20])
def test_default_plan_fuses_sites_of_buildings(oracle, n_sub):
    """Buildings only (no glazing): the default plan marches every cluster resident, each workgroup on its own site."""
    parts = [mdl.clustered_massive(300, Z=12, seed=s) for s in range(3)] + [mdl.partitioned_buildings(192, 10, seed=5)]
    md, site = mdl.concat([m for m, _ in parts])
    state = np.concatenate([s for _, s in parts])
    w = mdl.weather_sites(n_sub, 45.0, len(parts), seed=11)
    ref, _ = oracle_per_site(oracle, parts, w)
    for path in ("march", "resident"):
        got, _, n_fused, n_launches = run_sites(md, site, state, w, path)
        assert n_fused > 0 and n_launches > 0
        assert_state_close(md, ref, got)


@pytest.mark.parametrize("opts", [dict(), dict(no_fusion=True), dict(fuse_always=True), dict(use_graph=True)],
                         ids=["default", "no_fusion", "fuse_always", "graph"])
def test_interleaved_sites(oracle, opts):
    parts, md, site, _ = five_sites(interleave=True)
    assert site[:5].tolist() == [0, 1, 2, 3, 4]
    state = np.empty(md["n_state"])  # (the slots are the models' back to back whatever the surface order)
    state[:] = np.concatenate([s for _, s in parts])
    w = mdl.weather_sites(7, 45.0, 5, seed=3)
    ref, iters = oracle_per_site(oracle, parts, w)
    for path in ("march", "resident"):
        got, gpu_iters, _, _ = run_sites(md, site, state, w, path, **opts)
        assert_state_close(md, ref, got)
        assert gpu_iters == iters


def test_zone_faced_from_two_sites(oracle):
    """A wall of site 1 faces a zone of site 0: the cluster holds two sites' Outdoor sides — legal, and streamed."""
    a, sa = mdl.clustered_massive(120, Z=4, seed=41)
    b, sb = mdl.clustered_massive(120, Z=4, seed=42)
    md, site = mdl.concat([a, b])
    s_bridge = int(np.flatnonzero((site == 1) & (md["back_kind"] == mdl.SPACE) & (md["front_kind"] == mdl.OUTDOOR))[0])
    md["back_zone"] = md["back_zone"].copy()
    md["back_zone"][s_bridge] = 0  # a zone of site 0
    state = np.concatenate([sa, sb])
    n_sub = 6
    w = mdl.weather_sites(n_sub, 45.0, 2, seed=5)
    # the oracle march put together: each site's surfaces with its own weather, then the zones (model.rs:369-424)
    ref = state.copy()
    om = oracle.OracleModel(md)
    bounds = [(0, 120), (120, 240)]
    zs = md["zone_slot"]
    for k in range(n_sub):
        t_cur = ref[zs].copy()
        for s_, (s0, s1) in enumerate(bounds):
            rc, _ = om.iterate_surfaces(ref, w[k, s_, 1], w[k, s_, 2], w[k, s_, 0], s0, s1)
            assert rc == 0
        A, B, Cc = om.zones_abc(ref)
        big = np.abs(B) > 1e-9
        ref[zs] = np.where(big, A / np.where(big, B, 1.0) + (t_cur - A / np.where(big, B, 1.0)) *
                           np.exp(-B * md["dt"] / Cc), t_cur)
    # the cluster of zone 0 — zone 0, the zones its walls join it to, the bridging wall — is the one that holds two sites
    mixed = cluster_surfaces(md, 0)
    assert s_bridge in mixed and len(set(site[mixed].tolist())) == 2
    for opts in (dict(), dict(fuse_always=True)):
        got = state.copy()
        with HeatBatch(md, sites=site, **opts) as bt:
            bt.upload_state(got)
            bt.march(got, w)
            n_fused = bt.n_fused_surfaces
        assert_state_close(md, ref, got)
        if opts:
            # every cluster fuses without sites; with them exactly the mixed one streams
            one = binding.plan_check(md, fuse_always=True)
            two = binding.plan_check_sites(md, 2, site, fuse_always=True)
            assert one[5] == md["n_surfaces"]
            assert two[5] == n_fused == md["n_surfaces"] - len(mixed)


def cluster_surfaces(md, zone):
    """The surfaces of the zone-connected cluster of `zone` (model.rs:556-590: surfaces meet only through zones)."""
    fk, bk, fz, bz = md["front_kind"], md["back_kind"], md["front_zone"], md["back_zone"]
    zones, changed = {zone}, True
    while changed:
        changed = False
        for s_ in range(md["n_surfaces"]):
            zs = {int(z) for z, k in ((fz[s_], fk[s_]), (bz[s_], bk[s_])) if k == mdl.SPACE}
            if zs & zones and not zs <= zones:
                zones |= zs
                changed = True
    return np.array([s_ for s_ in range(md["n_surfaces"]) if any(
        k == mdl.SPACE and int(z) in zones for z, k in ((fz[s_], fk[s_]), (bz[s_], bk[s_])))], dtype=np.int64)


def test_weather_beyond_the_record_limit_is_refused():
    """n_sub * n_sites records per call are capped (2^24, 512 MB pinned): refused before anything is read or allocated."""
    parts = [mdl.clustered_massive(60, Z=2, seed=s)[0] for s in (1, 2)]
    md, site = mdl.concat(parts)
    with HeatBatch(md, sites=site) as b:
        w, _ = binding.as_weather(np.zeros((1, 2, 3)), 2)
        rc = b._L.heat_batch_set_weather(b._h, w, (1 << 23) + 1, None, None)
        assert rc == -1 and b"weather records" in b._L.heat_last_error()
        with pytest.raises(ValueError):
            b.march_resident(np.zeros((4, 3)))  # single-site weather for a batch of two sites
        b.march_resident(mdl.weather_sites(3, 45.0, 2))  # (still usable)
        b.synchronize()


def test_one_site_is_bit_identical_to_a_batch_without_sites():
    md, st = mdl.clustered_massive(600, Z=24, seed=7)
    w1 = mdl.weather_series(9, 45.0)
    for opts in (dict(), dict(fuse_always=True), dict(no_fusion=True, use_graph=True)):
        plain, sited = st.copy(), st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(plain)
            b.march(plain, w1)
        with HeatBatch(md, sites=np.zeros(md["n_surfaces"], np.int32), **opts) as b:
            assert b.n_sites == 1
            b.upload_state(sited)
            b.march(sited, w1[:, None, :])
        assert np.array_equal(plain, sited)


def test_identical_weather_at_every_site_matches_the_joined_model():
    parts, md, site, state = five_sites()
    w1 = mdl.weather_series(7, 45.0)
    plain = state.copy()
    with HeatBatch(md) as b:
        b.upload_state(plain)
        b.march(plain, w1)
    got, _, _, _ = run_sites(md, site, state, np.repeat(w1[:, None, :], 5, axis=1))
    assert_state_close(md, plain, got)


def test_sites_at_size(oracle):
    """About 200 000 surfaces over 64 sites, against each site's oracle march (threaded, as test_config5 does)."""
    parts = []
    for k in range(64):
        if k % 4 == 3:
            parts.append(mdl.rooms_with_windows(3000, Z=150, seed=100 + k))
        else:
            parts.append(mdl.clustered_massive(3200, Z=128, seed=100 + k))
    md, site = mdl.concat([m for m, _ in parts])
    state = np.concatenate([s for _, s in parts])
    assert md["n_surfaces"] > 190_000
    w = mdl.weather_sites(10, 45.0, 64, seed=9)
    ref, _ = oracle_per_site(oracle, parts, w, threads=16)  # (the threaded oracle counts no no-mass passes)
    for opts in (dict(), dict(use_graph=True, no_fusion=True)):
        got, _, _, _ = run_sites(md, site, state, w, "resident", **opts)
        assert_state_close(md, ref, got)
