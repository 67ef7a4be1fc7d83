"""The cluster-resident march on premultiplied stencil coefficients (kernels.hip: apply_PQ / rk4_horner_pq, fused_pq_form):
the instantiations without no-mass nodes and without gas cavities keep P_j = V_j U_j and Q_j = V_j U_{j-1} in the registers
of U and V, write the two face coefficients (Q_0 = V_0 hF on a wall's first lane, P_last = V_last hB at its last node) anew in
every sub-timestep and add the two sources in the first application only. The shapes below are the smallest where those slots
can go wrong, each held to the oracle at the project's rtol = atol = 1e-9 in ONE call of 1, 2 and 20 sub-timesteps:

  n32-tail    100 walls x 32 nodes in one zone, 16 per lane (`full`: the last node is node 15 of the last lane): four wavefronts,
              the fourth with 8 lanes in its layout; wall 31 ends on lane 63, wall 32 starts on lane 0 of the next wavefront
  n17 n20 n31 the last node inside its lane, at jl = 0, 3 and 14 (`!full`; n17: the last lane holds one node, first of the
              lane and last of the wall at once)
  n48 n64     three and four lanes per wall: a middle lane is neither first nor last, its Q_0 = V_0 U of the lane before
  n8-m8 n6-m8 single-lane walls at 8 per lane: both face slots and both sources on one lane, full and with jl = 5
  n8-m4 n6-m4 the same walls at 4 per lane (two lanes; jl = 3 and 1)
  boundaries  Outdoor and Space fronts, Space backs, one back in five facing an ambient temperature (it reads the FRONT face
              temperature), hs overrides on a share of the fronts and of the backs
  rows        partitioned_buildings with 8 rooms: 8 zones in a workgroup of 4 wavefronts, a row of 16 lanes per zone
  team        one building of 40 rooms, 480 walls x 32 nodes: a cluster larger than a workgroup, marched by a team
Every case asserts its plan ({(class, list): workgroups}, teams; classes 1 / 7 / 13 are the 4 / 8 / 16-node classes without
no-mass facings and without cavities, lists 0 / 1 the plain workgroups of 4 / 8 wavefronts), the batch's class_counts and
n_fused_launches, so that it provably runs a converted instantiation.

IDEAL: the M16-nm0-4w case of tests/ideal_variants_cases.py through the harness of tests/test_ideal_variants_gpu.py (the
IDEAL sibling of the headline's instantiation; the reference and the bounds are that file's).

NaN containment: make_plan refuses a NaN among the walls' conductances, so the NaN conductance is a FACE conductance — a
NaN tilt coefficient makes hs NaN (tests/test_resident_flags_gpu.py), and with it Q_0 or P_last, the source and every
temperature of that wall. 100 walls x 32 nodes in four zones share one workgroup; the damaged wall is the first or the last
of its zone, so that a healthy wall of another zone sits on the lanes right before or right behind it. Every slot of the
three other zones and their walls must equal the undamaged run bit for bit.
"""
import functools

import numpy as np
import pytest

import helpers
import ideal_variants_cases as ivc
import test_ideal_variants_gpu as tiv
from heat_amd import HeatBatch, HeatError, modeldict as mdl
from oracle import oracle as orc
from test_ideal_resident_gpu import hold_to_the_reference

pytestmark = pytest.mark.gpu

DT = 45.0
TOL = 1e-9
CALLS = [1, 2, 20]


def _uniform(S, n, Z):
    return lambda: mdl.uniform_massive(S, n, Z=Z, dt=DT)


def _boundaries():
    md, st = mdl.partitioned_buildings(96, 32, rooms=4, dt=DT, seed=5)
    helpers.ambient_backs(md, st, np.random.default_rng(77), 0.2)
    S = int(md["n_surfaces"])
    md["front_hs_fix"] = np.full(S, np.nan)       # (NaN: no override)
    md["back_hs_fix"] = np.full(S, np.nan)
    md["front_hs_fix"][3::7] = 7.5
    md["back_hs_fix"][5::11] = 3.25
    return md, st


# case -> (model, nodes per lane, {(class, list): workgroups}, teams, class_counts index of the walls)
CASES = {
    "n32-tail": (_uniform(100, 32, 1), 16, {(13, 0): 1}, 0, 2),
    "n17": (_uniform(40, 17, 2), 16, {(13, 0): 1}, 0, 2),
    "n20": (_uniform(40, 20, 2), 16, {(13, 0): 1}, 0, 2),
    "n31": (_uniform(40, 31, 2), 16, {(13, 0): 1}, 0, 2),
    "n48": (_uniform(40, 48, 2), 16, {(13, 0): 1}, 0, 2),
    "n64": (_uniform(40, 64, 2), 16, {(13, 0): 1}, 0, 2),
    "n8-m8": (_uniform(40, 8, 2), 8, {(7, 0): 1}, 0, 1),
    "n6-m8": (_uniform(40, 6, 2), 8, {(7, 0): 1}, 0, 1),
    "n8-m4": (_uniform(40, 8, 2), 4, {(1, 0): 1}, 0, 0),
    "n6-m4": (_uniform(40, 6, 2), 4, {(1, 0): 1}, 0, 0),
    "boundaries": (_boundaries, 16, {(13, 0): 2}, 0, 2),
    "rows": (lambda: mdl.partitioned_buildings(96, 32, rooms=8, dt=DT), 0, {(13, 0): 1}, 0, 2),
    "team": (lambda: mdl.partitioned_buildings(480, 32, rooms=40, dt=DT, seed=33), 0, {}, 1, 2),
}
CONVERTED = {(c, g2) for c in (1, 7, 13) for g2 in (0, 1)}


def options_of(name):
    return dict(nodes_per_lane=CASES[name][1], fuse_always=True)


@functools.lru_cache(maxsize=None)
def model(name):
    md, st = CASES[name][0]()
    assert md["n_surfaces"] <= 500
    return md, st


@functools.lru_cache(maxsize=None)
def reference(name, n_sub):
    """The oracle's state after n_sub sub-timesteps from the initial state; computed once, never written again."""
    md, st = model(name)
    ref = st.copy()
    rc, _ = orc.OracleModel(md).march(ref, mdl.weather_series(n_sub, DT))
    assert rc == 0
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_shapes_are_planned_as_meant(name):
    md, _ = model(name)
    plan = helpers.plan_lists(md, **options_of(name))
    assert plan["lists"] == CASES[name][2] and plan["teams"] == CASES[name][3] and plan["stream_tiles"] == 0, plan
    assert set(plan["lists"]) <= CONVERTED
    n = np.diff(md["node_offset"])
    if name == "boundaries":
        assert {mdl.OUTDOOR, mdl.SPACE} <= set(md["front_kind"]) and {mdl.SPACE, mdl.AMBIENT} <= set(md["back_kind"])
        assert np.isfinite(md["front_hs_fix"]).sum() >= 5 and np.isfinite(md["back_hs_fix"]).sum() >= 5
    elif name == "rows":
        assert plan["most_zones"] == 8, plan
    elif name == "team":
        assert md["n_surfaces"] == 480 and md["n_zones"] == 40
    else:
        assert np.all(n == int(name[1:3].rstrip("-")))


@pytest.mark.parametrize("n_sub", CALLS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_call_against_the_oracle(name, n_sub):
    md, st = model(name)
    S = int(md["n_surfaces"])
    ref = reference(name, n_sub)
    got = st.copy()
    with HeatBatch(md, **options_of(name)) as b:
        counts = [0] * 5
        counts[CASES[name][4]] = S
        assert b.class_counts() == counts and b.n_fused_surfaces == S, (b.class_counts(), b.n_fused_surfaces)
        b.upload_state(got)
        b.march(got, mdl.weather_series(n_sub, DT))
        launches = b.n_fused_launches
    if CASES[name][3]:
        assert launches > 0                        # (a team launch; no plain list beside it)
    else:
        assert launches == len(CASES[name][2])     # one launch per workgroup list of the call
    worst = {}
    for what, idx in (("nodes", mdl.node_slots(md)), ("hs_front", md["hs_front_slot"]), ("hs_back", md["hs_back_slot"]),
                      ("flow_front", md["flow_front_slot"]), ("flow_back", md["flow_back_slot"]), ("zones", md["zone_slot"])):
        idx = np.asarray(idx, dtype=np.int64)
        assert np.all(np.isfinite(ref[idx]))
        worst[what] = float(np.max(np.abs(got[idx] - ref[idx]) / (TOL + TOL * np.abs(ref[idx]))))
    nodes = np.asarray(mdl.node_slots(md), dtype=np.int64)
    print("%s, %d sub-timesteps: worst |dT| = %.3e K; worst |got - ref| / (atol + rtol |ref|) = %s" % (
        name, n_sub, float(np.max(np.abs(got[nodes] - ref[nodes]))), worst))
    for what, w in worst.items():
        assert w <= 1.0, (what, w)
    assert np.max(np.abs(ref[nodes] - st[nodes])) > 1e3 * TOL      # the call moved the walls


@pytest.mark.parametrize("n_sub,n_steps", ivc.CALLS)
def test_the_ideal_sibling_matches_its_cpu_reference(oracle, n_sub, n_steps):
    name = "M16-nm0-4w"
    assert set(ivc.plan_of(name)["lists"]) <= CONVERTED
    c, out, got = tiv.full_run(oracle, name, n_sub, n_steps)       # (asserts n_fused_launches = steps x lists)
    hold_to_the_reference(name, c.args[0], n_sub, c.args[8], c.ref, c.ref_state, out, got)


# ---- NaN containment ----
NAN_WALLS = [25, 49]        # first and last wall of zone 1 (walls 25..49)


@functools.lru_cache(maxsize=None)
def nan_model():
    md, st = mdl.uniform_massive(100, 32, Z=4, dt=DT)
    assert np.array_equal(md["back_zone"], np.arange(100) * 4 // 100) and np.all(md["front_kind"] == mdl.OUTDOOR)
    return md, st


@functools.lru_cache(maxsize=None)
def nan_marched(wall):
    md, st = nan_model()
    if wall is not None:
        md = dict(md)
        md["cos_tilt"] = np.array(md["cos_tilt"], dtype=np.float64)
        md["cos_tilt"][wall] = np.nan
    got = st.copy()
    with HeatBatch(md, nodes_per_lane=16, fuse_always=True) as b:
        assert b.class_counts() == [0, 0, 100, 0, 0] and b.n_fused_surfaces == 100
        b.upload_state(got)
        b.march_resident(mdl.weather_series(3, DT))
        code = 0
        try:
            b.synchronize()
        except HeatError as e:
            code = e.code
        where = b.failed_surface()
        b.download_state(got)                      # the march completed: its state is there to be read
        assert b.n_fused_launches == 1
    got.setflags(write=False)
    return code, where, got


@pytest.mark.parametrize("wall", NAN_WALLS)
def test_a_nan_face_conductance_stays_inside_its_zone(wall):
    md, st = nan_model()
    plan = helpers.plan_lists(md, nodes_per_lane=16, fuse_always=True)
    assert plan["lists"] == {(13, 0): 1} and plan["most_zones"] == 4, plan      # four clusters in ONE workgroup
    zone = int(md["back_zone"][wall])
    assert zone == 1 and md["back_zone"][wall - 1 if wall == 25 else wall + 1] != zone
    clean = nan_marched(None)
    assert clean[0] == 0 and clean[1] == (-1, 0)
    code, where, got = nan_marched(wall)
    assert code != 0 and md["back_zone"][where[0]] == zone, (code, where)
    n = np.diff(md["node_offset"])
    healthy = np.flatnonzero(md["back_zone"] != zone)
    slots = np.concatenate([np.concatenate([md["first_node_slot"][s] + np.arange(n[s]) for s in healthy])] +
                           [np.asarray(md[k])[healthy] for k in ("hs_front_slot", "hs_back_slot", "flow_front_slot", "flow_back_slot")] +
                           [np.asarray(md["zone_slot"])[np.arange(4) != zone]]).astype(np.int64)
    assert np.all(np.isfinite(clean[2][slots]))
    assert np.array_equal(got[slots], clean[2][slots]), "a slot outside the damaged zone changed"
    own = md["first_node_slot"][wall] + np.arange(n[wall])
    assert np.isnan(got[own]).any()                # and the damage is there
