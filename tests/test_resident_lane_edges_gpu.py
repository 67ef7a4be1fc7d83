"""The cluster-resident march at the smallest shapes where its lane exchange, its face terms and its outputs can go wrong,
each held to the oracle at the project's rtol = atol = 1e-9.

What the shapes are for (kernels.hip: dpp_rotate_f64 / dpp_add_f64 without a named `old` value, the face terms selected
straight into the RK4's effective conductances, SideOut written after the last sub-timestep of a call):
  tail-wavefront  100 walls x 32 nodes in one zone, 16 per lane: four wavefronts, the fourth with 8 lanes in its layout —
                  the rotates and the zone's DPP sums run over lanes without a wall
  wrap            33 walls x 32 nodes: wall 31 ends on lane 63 of the first wavefront, wall 32 starts on lane 0 of the
                  second — what the rotate wraps around from the other end of the wavefront must be replaced by zero
  inside-lane     20 nodes at 16 per lane: the last node sits inside its lane (`!full`, jl = 3)
  single-lane     8 nodes at 8 per lane: one lane owns both faces of its wall (kSingleLane)
  rows            partitioned_buildings(96, 32, rooms=4): 8 zones in a workgroup of 4 wavefronts, a row of 16 lanes per zone
  team            one building of 24 rooms, 288 walls x 32 nodes: a team of workgroups
Every case is marched in ONE call of 1, of 2 and of 20 sub-timesteps from the initial state, and beside the node and zone
temperatures the SideOut outputs (hs and heat flow of both sides), which belong to the call's last sub-timestep, are compared.
"""
import functools

import numpy as np
import pytest

import helpers
from heat_amd import HeatBatch, modeldict as mdl
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DT = 45.0
TOL = 1e-9
CALLS = [1, 2, 20]

# case -> (model, nodes per lane, {(class, list): workgroups}, teams)
CASES = {
    "tail-wavefront": (lambda: mdl.uniform_massive(100, 32, Z=1, dt=DT), 16, {(13, 0): 1}, 0),
    "wrap": (lambda: mdl.uniform_massive(33, 32, Z=1, dt=DT), 16, {(13, 0): 1}, 0),
    "inside-lane": (lambda: mdl.uniform_massive(40, 20, Z=2, dt=DT), 16, {(13, 0): 1}, 0),
    "single-lane": (lambda: mdl.uniform_massive(40, 8, Z=2, dt=DT), 8, {(7, 0): 1}, 0),
    "rows": (lambda: mdl.partitioned_buildings(96, 32, rooms=4, dt=DT), 0, {(13, 0): 1}, 0),
    "team": (lambda: mdl.partitioned_buildings(288, 32, rooms=24, dt=DT, seed=33), 0, {}, 1),
}


def options_of(name):
    return dict(nodes_per_lane=CASES[name][1], fuse_always=True)


@functools.lru_cache(maxsize=None)
def model(name):
    return CASES[name][0]()


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
    if name == "rows":
        assert plan["most_zones"] > 4, plan      # more zones than the workgroup has wavefronts: a row per zone
    if name in ("tail-wavefront", "wrap"):
        assert plan["most_zones"] == 1, plan


@pytest.mark.parametrize("n_sub", CALLS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_call_against_the_oracle(name, n_sub):
    md, st = model(name)
    ref = reference(name, n_sub)
    got = st.copy()
    with HeatBatch(md, **options_of(name)) as b:
        assert b.n_fused_surfaces == md["n_surfaces"], (b.n_fused_surfaces, b.class_counts())
        b.upload_state(got)
        b.march(got, mdl.weather_series(n_sub, DT))
        assert b.n_fused_launches > 0
    worst = {}
    for what, idx in (("nodes", mdl.node_slots(md)), ("hs_front", md["hs_front_slot"]), ("hs_back", md["hs_back_slot"]),
                      ("flow_front", md["flow_front_slot"]), ("flow_back", md["flow_back_slot"]), ("zones", md["zone_slot"])):
        idx = np.asarray(idx, dtype=np.int64)
        assert np.all(np.isfinite(ref[idx]))
        worst[what] = float(np.max(np.abs(got[idx] - ref[idx]) / (TOL + TOL * np.abs(ref[idx]))))
    print("%s, %d sub-timesteps: worst |got - ref| / (atol + rtol |ref|) = %s" % (name, n_sub, worst))
    for what, w in worst.items():
        assert w <= 1.0, (what, w)
    # the outputs are the last sub-timestep's, not an earlier one's: they differ from a call one sub-timestep shorter
    if n_sub > 1:
        before = reference(name, n_sub - 1)
        idx = np.asarray(md["flow_back_slot"], dtype=np.int64)
        assert np.max(np.abs(before[idx] - ref[idx])) > 1e3 * TOL * np.max(np.abs(ref[idx]))
