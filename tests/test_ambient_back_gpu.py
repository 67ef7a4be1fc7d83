"""Back sides that face an ambient temperature (Boundary::AmbientTemperature on the back), on the GPU.

The reference gives such a side a rule of its own (surface.rs:672-686, oracle/heat_oracle.c calc_border_conditions): its
radiant temperature is t_front — the FRONT side's air: the front zone, the front ambient temperature or the outdoor air —
and the surface temperature its convection coefficient is evaluated on is the FRONT node's. The device code carries that
rule in every kernel family (the front side's source packed into the back record by the planner; the front node shuffled
from the surface's first lane; the front zone read from LDS in the cluster-resident march; the small and the general
kernel), and no generator of heat_amd/modeldict.py makes such a side: tests/helpers.ambient_backs converts a share of a
generated model's surfaces, across all three kinds of front side.

Every case first shows, on the oracle's result, that it discriminates: for nine in ten converted surfaces hs_back is more
than 1e-3 (relative) away from the TARP coefficient of the back_ambient against the LAST node — what a kernel without the
rule would write. Then the march is held to the oracle with the suite's run_both / assert_state_close (1e-9; run_both
also holds the streamed kernels to the oracle whenever the plan fuses), no-mass pass counts equal.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import ambient_backs
from heat_amd import HeatBatch
from heat_amd import modeldict as mdl
from test_parity_gpu import assert_state_close, run_both

pytestmark = pytest.mark.gpu


def convert(md, st, seed, fraction=0.4):
    """Converts `fraction` of the surfaces; returns them, with zone terms that make the zones move."""
    rng = np.random.default_rng(seed)
    conv = ambient_backs(md, st, rng, fraction)
    fk = md["front_kind"][conv]
    assert {int(k) for k in fk} == {mdl.SPACE, mdl.AMBIENT, mdl.OUTDOOR}, "all three kinds of front side"
    Z = int(md["n_zones"])
    return conv, rng.uniform(0., 60., Z), rng.uniform(0.1, 2., Z)


def assert_discriminates(oracle, md, ref, conv):
    """hs_back of the oracle against the reading a kernel without the rule would produce."""
    lib = oracle.lib()
    err = C.c_int(0)
    n = np.diff(md["node_offset"])[conv]
    last = md["first_node_slot"][conv] + n - 1
    off = 0
    for s, ls, nn in zip(conv, last, n):
        wrong = lib.or_tarp_natural(float(md["back_ambient"][s]), float(ref[ls]), float(md["cos_tilt"][s]), C.byref(err))
        hs = ref[md["hs_back_slot"][s]]
        off += abs(hs - wrong) > 1e-3 * abs(wrong)
    assert off >= 0.9 * len(conv), "only %d of %d converted surfaces tell the rule from its absence" % (off, len(conv))


def parity(oracle, md, st, w, a0, b0, conv, **opts):
    ref, got, iters, gpu_iters, counts = run_both(oracle, md, st, w, a0, b0, **opts)
    assert_discriminates(oracle, md, ref, conv)
    assert iters == gpu_iters, "no-mass loop took a different number of passes (%d vs %d)" % (iters, gpu_iters)
    assert_state_close(md, ref, got)
    return counts


@pytest.mark.parametrize("npl", [0, 4, 8, 16])
@pytest.mark.parametrize("n", [2, 7, 13, 32, 50, 64])
def test_uniform_massive_walls(oracle, n, npl):
    """Single-lane walls (the other side's kind read from bits 4-5 of the record) and walls over several lanes (the
    front node in another lane than the back side: T[0] shuffled from the surface's first lane)."""
    md, st = mdl.uniform_massive(420, n, Z=6, dt=45.0, seed=3 * n + npl)
    conv, a0, b0 = convert(md, st, 100 + n + npl)
    w = mdl.weather_series(7, 45.0, wind_speed=4.5, wind_deg=200.0)
    counts = parity(oracle, md, st, w, a0, b0, conv, nodes_per_lane=npl)
    assert counts[3] == 0


@pytest.mark.parametrize("opts", [dict(), dict(force_general=True), dict(no_palette=True), dict(no_fusion=True),
                                  dict(use_graph=True)], ids=lambda o: "-".join(o) or "planned")
def test_ragged_mixed_walls(oracle, opts):
    """Chunk-loop walls, the small kernel (two no-mass nodes) and no-mass facings; pass counts equal."""
    md, st = mdl.ragged_mixed(1500, Z=15, dt=45.0, seed=20260402)
    conv, a0, b0 = convert(md, st, 7)
    n = np.diff(md["node_offset"])[conv]
    assert (n == 2).any() and (n > 32).any()
    w = mdl.weather_series(5, 45.0)
    counts = parity(oracle, md, st, w, a0, b0, conv, **opts)
    if not opts:
        assert counts[3] > 0 and sum(counts[:3]) > 0
    if "force_general" in opts:
        assert counts[4] == md["n_surfaces"]


@pytest.mark.parametrize("opts", [dict(), dict(fuse_always=True), dict(no_palette=True)], ids=lambda o: "-".join(o) or "planned")
def test_glazing_and_cavity_walls(oracle, opts):
    md, st = mdl.glazing_cavity(400, Z=8, dt=45.0, seed=9)
    conv, a0, b0 = convert(md, st, 11)
    w = mdl.weather_series(5, 45.0)
    parity(oracle, md, st, w, a0, b0, conv, **opts)


@pytest.mark.parametrize("opts", [dict(), dict(fuse_always=True), dict(no_fusion=True), dict(use_graph=True),
                                  dict(fuse_always=True, nodes_per_lane=4), dict(fuse_always=True, nodes_per_lane=16)],
                         ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()) or "planned")
def test_clustered_walls_in_the_resident_march(oracle, opts):
    """Small clusters: the cluster-resident march reads the front side's zone of a Space / Ambient wall from LDS."""
    md, st = mdl.clustered_massive(900, Z=36, dt=45.0, seed=13)
    conv, a0, b0 = convert(md, st, 17)
    assert ((md["front_kind"][conv] == mdl.SPACE)).sum() > 20
    w = mdl.weather_series(6, 45.0, wind_speed=2.0, wind_deg=300.0)
    parity(oracle, md, st, w, a0, b0, conv, **opts)
    if opts.get("fuse_always"):
        with HeatBatch(md, **opts) as b:
            print("clustered %s: %d of %d surfaces cluster-resident" % (opts, b.n_fused_surfaces, md["n_surfaces"]))
            assert b.n_fused_surfaces > 0, (b.n_fused_surfaces, b.class_counts())


@pytest.mark.parametrize("rooms,n,opts", [(8, 20, {}), (8, 9, dict(fuse_always=True, nodes_per_lane=4)), (40, 20, {}),
                                          (40, 7, dict(fuse_always=True))])
def test_buildings_of_rooms(oracle, rooms, n, opts):
    """One cluster per building: a workgroup (8 rooms) or a team of workgroups (40 rooms)."""
    per = rooms * 12
    md, st = mdl.partitioned_buildings(max(3 * per, 480), n, rooms=rooms, dt=45.0, seed=rooms + n)
    conv, a0, b0 = convert(md, st, rooms)
    w = mdl.weather_series(5, 45.0, wind_speed=3.5, wind_deg=120.0)
    parity(oracle, md, st, w, a0, b0, conv, **opts)
    with HeatBatch(md, **opts) as b:
        print("rooms %d %s: %d of %d surfaces cluster-resident" % (rooms, opts, b.n_fused_surfaces, md["n_surfaces"]))
        assert b.n_fused_surfaces > 0, b.class_counts()


@pytest.mark.parametrize("opts", [dict(), dict(fuse_always=True), dict(force_general=True)], ids=lambda o: "-".join(o) or "planned")
def test_rooms_with_windows(oracle, opts):
    md, st = mdl.rooms_with_windows(800, Z=40, dt=45.0, seed=29)
    conv, a0, b0 = convert(md, st, 31)
    n = np.diff(md["node_offset"])[conv]
    assert (n == 4).any() and (n == 2).any()          # windows and thin partitions among the converted
    w = mdl.weather_series(5, 45.0)
    parity(oracle, md, st, w, a0, b0, conv, **opts)


def test_two_shards_on_one_device(oracle):
    """As test_shards_of_the_cluster_partition_march_without_any_exchange: every rank's batch from the whole descriptor."""
    from heat_amd import binding
    md, st = mdl.clustered_massive(1200, Z=48, dt=45.0, seed=21)
    conv, a0, b0 = convert(md, st, 23)
    w = mdl.weather_series(6, 45.0, wind_speed=2.5, wind_deg=310.0)
    ref = st.copy()
    rc, iters = oracle.OracleModel(md).march(ref, w, a0, b0)
    assert rc == 0
    assert_discriminates(oracle, md, ref, conv)
    ranks, n_shared = binding.partition(md, 2)
    assert n_shared == 0 and ranks.max() == 1
    got = st.copy()
    total = 0
    for r in range(2):
        assert (ranks[conv] == r).any()
        with HeatBatch(md, n_ranks=2, rank=r, rank_of_surface=ranks, use_graph=True) as b:
            b.upload_state(st)
            b.march(got, w[:2], a0, b0)
            b.march_resident(w[2:], a0, b0)
            b.synchronize()
            b.download_state(got)
            total += b.nomass_iterations()
    assert total == iters
    assert_state_close(md, ref, got)


def test_series_with_a_driven_long_wave_input_on_a_converted_back(oracle):
    """march_series against the per-call loop (bit for bit) and the oracle loop. The long-wave irradiance of a back side
    that faces an ambient temperature is driven — and, by the rule, not read: its radiant temperature is t_front."""
    import test_series_gpu as ts
    md, st = mdl.rooms_with_windows(700, Z=35, dt=45.0, seed=37)
    conv, a0, b0 = convert(md, st, 41)
    rng = np.random.default_rng(43)
    n_steps, n_sub = 8, 3
    channel, drives = ts.random_drives(md, rng, n_steps)
    assert (drives["ir_back"][0][conv] >= 0).any()
    probes = np.concatenate([ts.probes_of_every_kind(md, rng), md["hs_back_slot"][conv[:30]],
                             md["flow_back_slot"][conv[:30]]]).astype(np.int64)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    ref = st.copy()
    ref_trace, iters = ts.oracle_series(oracle, md, ref, w, channel, drives, probes, a0, b0)
    assert_discriminates(oracle, md, ref, conv)
    own = ts.owned_slots(md)
    for opts in (dict(), dict(no_fusion=True)):
        per = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(per)
            per_trace = ts.per_call_series(b, md, per, w, channel, drives, probes, a0, b0)
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            b.upload_state(got)
            trace, failed = b.march_series(w, n_sub, **ts.series_kwargs(channel, drives, probes, a0, b0))
            b.download_state(got)
            gpu_iters = b.nomass_iterations()
        assert failed == -1 and gpu_iters == iters
        assert np.array_equal(per_trace, trace) and np.array_equal(per[own], got[own])
        ts.assert_close(ref_trace, trace, "trace %s" % opts)
        ts.assert_close(ref[own], got[own], "final state %s" % opts)


def test_drop_in_march_with_an_output_mask(oracle):
    """heat_batch_march_ex on a caller-owned state: the first call asks for the zones only, the second for everything."""
    md, st = mdl.ragged_mixed(600, Z=6, dt=45.0, seed=47)
    conv, a0, b0 = convert(md, st, 53)
    w = mdl.weather_series(6, 45.0)
    ref = st.copy()
    rc, iters = oracle.OracleModel(md).march(ref, w, a0, b0)
    assert rc == 0
    assert_discriminates(oracle, md, ref, conv)
    got = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(got)
        b.march(got, w[:3], a0, b0, outputs=HeatBatch.OUT_ZONES)
        assert np.array_equal(got[mdl.node_slots(md)], st[mdl.node_slots(md)])       # not asked for: not written
        b.march(got, w[3:], a0, b0, outputs=HeatBatch.OUT_ALL)
        assert b.nomass_iterations() == iters
    assert_state_close(md, ref, got)
