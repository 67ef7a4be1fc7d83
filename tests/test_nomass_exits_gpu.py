"""Every copy of the no-mass loop in kernels.hip (small_step, the one-node facing solve of fast_tile_march, its chunk
loop, k_surfaces_general — streamed and inside the cluster-resident march) through every exit of march_nomass
(surface.rs:790-898; tests/nomass_ref.py names them A to E), against the CPU oracle at the project's 1e-9 with equal pass
counts. The cases are those of tests/nomass_exit_cases.py; tests/test_nomass_exits_host.py holds them, on the host, to the
conditions under which a result here says something: the oracle within 1e-11 K of the loop in longdouble, every exit
reached in every family, no decision within 1e-6 of its threshold, a pass more or less moving a node by 1e-6 K at least.

Every family is marched in two orders — interleaved, every tile of 64 lanes mixing all exits, and grouped, one batch per
exit, so that equal totals of passes are equal counts per exit — in calls of one and of three sub-timesteps (three in one
call are what the resident march needs), under every option that applies to it."""
import functools

import numpy as np
import pytest

import nomass_exit_cases as nec
from heat_amd import HeatBatch, HeatError
from heat_amd import modeldict as mdl
from test_parity_gpu import assert_state_close

pytestmark = pytest.mark.gpu

HEAT_N_NAN_NOMASS = OR_ERR_NAN_NOMASS = 2

OPTIONS = {"planned": {}, "npl4": dict(nodes_per_lane=4), "npl8": dict(nodes_per_lane=8), "npl16": dict(nodes_per_lane=16),
           "no_palette": dict(no_palette=True), "general": dict(force_general=True), "streamed": dict(no_fusion=True),
           "resident": dict(fuse_always=True)}


def kind_of(family):
    return nec.FAMILIES[family.split(":")[-1]][1]


def options_of(family):
    if kind_of(family) != "fast":          # (the blocking factor and the palette are the register kernel's)
        return ["planned", "general", "streamed", "resident"]
    # per-node constants know the inline facing solve only: without the palette a two-node chunk is the catch-all's
    return [o for o in OPTIONS if o != "no_palette" or family.startswith("facing")]


RUNS = [(f, o) for f in nec.CASES for o in options_of(f)]


@functools.lru_cache(maxsize=None)
def reference(oracle, family, batch, n_sub):
    c = nec.case(family)
    md = mdl.subset(c.md, dict(nec.batches(c))[batch])
    ref = c.st.copy()
    rc, iters = oracle.OracleModel(md).march(ref, nec.WEATHER[:n_sub])
    assert rc == 0 and iters > 0
    ref.setflags(write=False)
    return md, ref, iters


def check_classes(family, option, md, n_own, counts, n_fused):
    S = int(md["n_surfaces"])
    kind = kind_of(family)
    if option == "general":
        assert counts[4] == S, counts
    elif kind == "small":
        assert counts[3] == n_own and counts[4] == 0, counts
    elif kind == "general":
        assert counts[4] == n_own and counts[3] == 0, counts
    else:
        assert counts[3] == 0, counts
        if family.startswith("chunk2") and option in ("npl4", "npl8", "npl16"):
            assert counts[4] < S, counts           # (a forced blocking factor may cut a two-node chunk in two)
        else:
            assert counts[4] == 0, counts
    if option == "resident" and kind != "general":
        assert n_fused == S, (n_fused, counts)     # small surfaces in the mixed workgroups of their walls' clusters
    if option in ("streamed", "general"):
        assert n_fused == 0


@pytest.mark.parametrize("family,option", RUNS)
def test_every_exit_in_every_copy_of_the_loop(oracle, family, option):
    c = nec.case(family)
    worst = 0.0
    for batch, idx in nec.batches(c):
        n_own = int((idx < c.n_own).sum())
        for n_sub in nec.N_SUB:
            md, ref, iters = reference(oracle, family, batch, n_sub)
            got = c.st.copy()
            with HeatBatch(md, **OPTIONS[option]) as b:
                check_classes(family, option, md, n_own, b.class_counts(), b.n_fused_surfaces)
                b.upload_state(got)
                b.march(got, nec.WEATHER[:n_sub])
                gpu_iters = b.nomass_iterations()
                assert (b.n_fused_launches > 0) == (b.n_fused_surfaces > 0)
            nodes = mdl.node_slots(md)
            worst = max(worst, float(np.abs(got[nodes] - ref[nodes]).max()))
            assert gpu_iters == iters, "%s, %d sub-timesteps: %d passes, the oracle %d" % (batch, n_sub, gpu_iters, iters)
            assert_state_close(md, ref, got)
    print("%s %s: worst |dT| against the oracle %.3e K" % (family, option, worst))


@pytest.mark.parametrize("fusion", ["planned", "streamed"])
@pytest.mark.parametrize("model", ["glazing_cavity", "rooms_with_windows"])
def test_generators_of_the_suite_without_wind(oracle, model, fusion):
    """modeldict.glazing_cavity leaves exit C once the wind drops (47 B and 7 D exits, a surface at 621 passes in one
    sub-timestep: tests/test_nomass_exits_host.py); rooms_with_windows stays in it, with more passes."""
    md, st = mdl.glazing_cavity(400, Z=8, dt=45.0) if model == "glazing_cavity" else mdl.rooms_with_windows(600, Z=12, dt=45.0)
    w = mdl.weather_series(25, 45.0, wind_speed=0.0)
    ref = st.copy()
    rc, iters = oracle.OracleModel(md).march(ref, w)
    assert rc == 0
    got = st.copy()
    with HeatBatch(md, **OPTIONS[fusion]) as b:
        b.upload_state(got)
        b.march(got, w)
        assert b.nomass_iterations() == iters
    assert_state_close(md, ref, got)


# ---------------------------------------------------------------------------------------------------------------------
# Exit E
E_MODES = ["planned", "streamed", "general", "resident"]
# (a wall of the catch-all kernel keeps its cluster out of the resident march: long_run has no resident run)
E_RUNS = [(f, m) for f in nec.E_FAMILIES for m in E_MODES if not (m == "resident" and nec.FAMILIES[f][1] == "general")]


@pytest.mark.parametrize("family,mode", E_RUNS)
def test_nan_error_of_the_loop_names_the_surface(oracle, family, mode):
    """surface.rs:850: a NaN err is the reference's error. The library reports it through its flag word — the march
    completes — as HEAT_N_NAN_NOMASS with the surface's number in the caller's descriptor, whichever copy of the loop met
    it; the other cluster never hears of it; a healthy upload marches clean again."""
    md, healthy, bad, s = nec.damaged(family)
    other = np.flatnonzero(np.arange(int(md["n_surfaces"])) % 2 == 1)
    n = np.diff(md["node_offset"])
    slots = np.concatenate([md["first_node_slot"][q] + np.arange(n[q]) for q in other] +
                           [np.asarray(md[k])[other] for k in ("hs_front_slot", "hs_back_slot", "flow_front_slot", "flow_back_slot")] +
                           [np.asarray(md["zone_slot"])[2:]]).astype(np.int64)
    with HeatBatch(md, **OPTIONS[mode]) as b:
        assert (b.n_fused_surfaces > 0) if mode == "resident" else (b.n_fused_surfaces == 0 or mode == "planned")
        clean = healthy.copy()
        b.upload_state(clean)
        b.march(clean, nec.WEATHER[:1])
        assert b.failed_surface() == (-1, 0)
        got = bad.copy()
        b.upload_state(got)
        b.march_resident(nec.WEATHER[:1])
        with pytest.raises(HeatError) as e:
            b.synchronize()
        assert e.value.code == HEAT_N_NAN_NOMASS, str(e.value)
        assert b.failed_surface() == (s, HEAT_N_NAN_NOMASS)
        assert "surface %d" % s in str(e.value)
        b.download_state(got)                                # the march completed: its state is there to be read
        assert np.all(np.isfinite(clean[slots]))
        assert np.array_equal(got[slots], clean[slots]), "a slot of the other cluster changed"
        again = healthy.copy()
        b.upload_state(again)
        b.march(again, nec.WEATHER[:1])                      # healthy again
        assert np.array_equal(again, clean)
