"""What a numerical failure reports, cluster-resident march against streamed march.

The resident march forms its failure flags (FLAG_UNREACHABLE, FLAG_NAN_HS; kernels.hip, `conv` of fast_tile_march) on the
good path of every sub-timestep, for flags that are zero in every good run — work that invites being moved (a cold block
behind one wave-uniform test of the coefficient was tried and measured slower: profiles/experiments/
r07_non_f64_switches.patch). Whatever form that code takes, it must not change what a failure reports: the status code, the
first failing surface and its kind (heat_batch_failed_surface), and a NaN must stay inside the cluster it arose in.

One small fuse_always model per branch of the zone phase and blocking factor, the first three from the table of
tests/ideal_variants_cases.py:
  wavefront   M16-nm0-4w   96 walls x 64 nodes, 16 per lane; 4 zones in a workgroup of 4 wavefronts: a wavefront per zone
  rows        zones32      192 walls x 8 nodes, 8 per lane (single-lane walls); 32 zones in one workgroup: a row per zone,
                           four buildings in ONE workgroup — three clusters beside the damaged one in the same LDS
  mixed       M4-mixed-4w  120 walls and windows, 4 per lane: small surfaces beside walls in a workgroup
  team        one building of 24 rooms, 288 walls x 32 nodes: a cluster larger than a workgroup, marched by a team
One chosen wall gets a NaN tilt coefficient (its natural-convection coefficients become NaN on the host, plan.cpp) or, in
a second case, a NaN initial front face temperature. Either is the reference's unreachable!() branch (convection.rs:104;
the oracle answers OR_ERR_UNREACHABLE = 4) and ALWAYS comes with a NaN coefficient (surface.rs:704-707), which is the
kind the library names first where both are seen (batch.hip, flags_to_status): HEAT_N_NAN_HS = 1.

This is a numerical condition the library reports through its flag word: the march completes, nothing faults.
  * a call of ONE sub-timestep: only the damaged wall fails, so the first failing surface is that wall, resident and
    streamed (no_fusion=True) alike, with the same status code and kind;
  * a call of three: the NaN reaches the wall's zones and their other walls. Resident and streamed raise the same
    code and kind, the surface named is one of the damaged wall's cluster, and every slot (node temperatures, coefficients,
    flows, zone temperatures) of every cluster that does not hold the damaged wall equals the undamaged run bit for bit.
"""
import functools

import numpy as np
import pytest

import helpers
import ideal_variants_cases as ivc
from heat_amd import HeatBatch, HeatError, modeldict as mdl
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT = 45.0
HEAT_N_NAN_HS, OR_ERR_UNREACHABLE = 1, 4


def _team_model():
    return mdl.partitioned_buildings(288, 32, rooms=24, dt=DT, seed=33)


# model -> (builder of (md, st), batch options, what the plan must hold)
MODELS = {
    "wavefront": (lambda: ivc.model_of("M16-nm0-4w"), ivc.options_of("M16-nm0-4w"), dict(lists={(13, 0): 2}, teams=0, most_zones=4)),
    "rows": (lambda: ivc.model_of("zones32"), ivc.options_of("zones32"), dict(lists={(7, 0): 1}, teams=0, most_zones=32)),
    "mixed": (lambda: ivc.model_of("M4-mixed-4w"), ivc.options_of("M4-mixed-4w"), dict(lists={(5, 2): 4}, teams=0)),
    "team": (_team_model, dict(fuse_always=True), dict(lists={}, teams=1)),
}
DAMAGES = ["tilt", "face"]


@functools.lru_cache(maxsize=None)
def model(name):
    md, st = MODELS[name][0]()
    assert md["n_surfaces"] <= 300
    return md, st


def clusters(md):
    """Component number of every zone and of every wall: zones joined by the walls that face two of them."""
    Z, S = int(md["n_zones"]), int(md["n_surfaces"])
    root = list(range(Z))

    def find(z):
        while root[z] != z:
            root[z] = root[root[z]]
            z = root[z]
        return z
    fz = np.where(np.asarray(md["front_kind"]) == mdl.SPACE, md["front_zone"], -1)
    bz = np.where(np.asarray(md["back_kind"]) == mdl.SPACE, md["back_zone"], -1)
    for a, b in zip(fz, bz):
        if a >= 0 and b >= 0:
            root[find(int(a))] = find(int(b))
    zone_c = np.array([find(z) for z in range(Z)])
    wall_c = np.array([zone_c[a] if a >= 0 else (zone_c[b] if b >= 0 else -1 - s) for s, (a, b) in enumerate(zip(fz, bz))])
    return zone_c, wall_c


def damaged_wall(md):
    """A wall of the most nodes (a wall of the fast path, not a small surface) facing a zone, from the middle of the model:
    neither the first surface nor one of the first cluster."""
    n = np.diff(md["node_offset"])
    _, wall_c = clusters(md)
    cand = np.flatnonzero((n == n.max()) & (wall_c >= 0))
    return int(cand[len(cand) // 2])


def damage(md, st, s, how):
    md, st = dict(md), st.copy()
    if how == "tilt":
        md["cos_tilt"] = np.array(md["cos_tilt"], dtype=np.float64)
        md["cos_tilt"][s] = np.nan
    else:
        st[md["first_node_slot"][s]] = np.nan
    return md, st


def slots_of(md, walls, zones):
    n = np.diff(md["node_offset"])
    node = np.concatenate([md["first_node_slot"][s] + np.arange(n[s]) for s in walls] or [np.zeros(0, np.int64)])
    scal = np.concatenate([np.asarray(md[k])[walls] for k in ("hs_front_slot", "hs_back_slot", "flow_front_slot", "flow_back_slot")])
    return np.concatenate([node, scal, np.asarray(md["zone_slot"])[zones]]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def marched(name, how, n_sub, streamed):
    """(status code, failed_surface(), final state, fused launches) of one march call of n_sub sub-timesteps."""
    md, st = model(name)
    if how is not None:
        md, st = damage(md, st, damaged_wall(md), how)
    opts = dict(MODELS[name][1])
    if streamed:
        opts = dict(opts, no_fusion=True, fuse_always=False)
    got = st.copy()
    with HeatBatch(md, **opts) as b:
        assert (b.n_fused_surfaces == 0) == streamed, (b.n_fused_surfaces, b.class_counts())
        b.upload_state(got)
        b.march_resident(mdl.weather_series(n_sub, DT))
        code = 0
        try:
            b.synchronize()
        except HeatError as e:
            code = e.code
        where = b.failed_surface()
        b.download_state(got)          # the march completed: its state is there to be read
        launches = b.n_fused_launches
    got.setflags(write=False)
    return code, where, got, launches


@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_models_reach_the_branches_meant(name):
    md, _ = model(name)
    plan = helpers.plan_lists(md, **MODELS[name][1])
    for key, want in MODELS[name][2].items():
        assert plan[key] == want, (key, plan)
    s = damaged_wall(md)
    zone_c, wall_c = clusters(md)
    assert 0 < s and wall_c[s] >= 0
    if name != "team":  # (the team's building is the whole model)
        assert len(set(zone_c)) > 1 and np.any(wall_c != wall_c[s])


@pytest.mark.parametrize("how", DAMAGES)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_oracle_takes_the_unreachable_branch(name, how):
    md, st = model(name)
    dmd, dst = damage(md, st, damaged_wall(md), how)
    rc, _ = orc.OracleModel(dmd).march(dst.copy(), mdl.weather_series(1, DT))
    assert rc == OR_ERR_UNREACHABLE, rc


@pytest.mark.parametrize("how", DAMAGES)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_one_sub_timestep_names_the_damaged_wall(name, how):
    md, _ = model(name)
    s = damaged_wall(md)
    res = marched(name, how, 1, False)
    stm = marched(name, how, 1, True)
    assert res[3] > 0 and stm[3] == 0, (res[3], stm[3])
    print("%s %s: resident code %d at %s, streamed code %d at %s, damaged wall %d" % (name, how, res[0], res[1], stm[0], stm[1], s))
    assert res[0] == stm[0] == HEAT_N_NAN_HS
    assert res[1] == stm[1] == (s, HEAT_N_NAN_HS)


@pytest.mark.parametrize("how", DAMAGES)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_three_sub_timesteps_keep_the_failure_in_its_cluster(name, how):
    md, _ = model(name)
    s = damaged_wall(md)
    zone_c, wall_c = clusters(md)
    res = marched(name, how, 3, False)
    stm = marched(name, how, 3, True)
    assert res[3] > 0
    print("%s %s: resident code %d at %s, streamed code %d at %s, damaged wall %d" % (name, how, res[0], res[1], stm[0], stm[1], s))
    assert res[0] == stm[0] == HEAT_N_NAN_HS
    assert res[1][1] == stm[1][1] == HEAT_N_NAN_HS
    for where in (res[1], stm[1]):
        assert wall_c[where[0]] == wall_c[s], (where, s)
    walls = np.flatnonzero(wall_c != wall_c[s])
    zones = np.flatnonzero(zone_c != wall_c[s])
    idx = slots_of(md, walls, zones)
    for streamed, run in ((False, res), (True, stm)):
        clean = marched(name, None, 3, streamed)
        assert clean[0] == 0 and clean[1] == (-1, 0)
        assert np.all(np.isfinite(clean[2][slots_of(md, np.arange(md["n_surfaces"]), np.arange(md["n_zones"]))]))
        assert np.array_equal(run[2][idx], clean[2][idx]), "a slot outside the damaged cluster changed (%s)" % ("streamed" if streamed else "resident")
    # and inside the damaged cluster the resident march leaves what the streamed march leaves: the same slots NaN
    inside = slots_of(md, np.flatnonzero(wall_c == wall_c[s]), np.flatnonzero(zone_c == wall_c[s]))
    assert np.array_equal(np.isnan(res[2][inside]), np.isnan(stm[2][inside]))
