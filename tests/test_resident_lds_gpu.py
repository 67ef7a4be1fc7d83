"""The cluster-resident march at 16 nodes per lane against the CPU oracle, at the smallest shapes that reach what the
march keeps in registers and what it asks its LDS for: V = dt/C of a lane's nodes (full, partly filled and one-node
last lanes; no-mass facings, whose test reads V — in registers, or in LDS where fused_v_in_lds keeps it: teams with
facings), a side's place in its zone's list, the zone data of a wavefront's or a row's zone, and the zones' lists
(fewer than four passes of a wavefront, exactly four, eight; rows with a second pass of one element).

Every owned slot is held to the oracle at rtol = atol = 1e-9 (test_parity_gpu.assert_state_close), no-mass pass counts
are equal where walls have no-mass nodes, and every case asserts that the resident march really took all its walls.
"""
import numpy as np
import pytest

from heat_amd import HeatBatch
from heat_amd import modeldict as mdl
from test_parity_gpu import assert_state_close, run_both

pytestmark = pytest.mark.gpu

RESIDENT = dict(nodes_per_lane=16, fuse_always=True)


def zone_terms(md, seed):
    rng = np.random.default_rng(seed)
    Z = md["n_zones"]
    return rng.uniform(0., 60., Z), rng.uniform(0.1, 2., Z)


def assert_all_resident(md, **kw):
    with HeatBatch(md, **dict(RESIDENT, **kw)) as b:
        assert b.n_fused_surfaces == md["n_surfaces"], (b.n_fused_surfaces, b.class_counts())


def both_faces_in_the_room(md):
    """Every wall stands inside its zone: front and back face it, two entries of the zone's list per wall."""
    md["front_kind"] = np.full(md["n_surfaces"], mdl.SPACE, dtype=np.int32)
    md["front_zone"] = md["back_zone"].copy()


@pytest.mark.parametrize("n", [32, 20, 17])
def test_wall_depths_full_partly_filled_and_one_node_last_lanes(oracle, n):
    md, st = mdl.uniform_massive(200, n, Z=2, dt=45.0, seed=400 + n)
    w = mdl.weather_series(20, 45.0, wind_speed=4.5, wind_deg=200.0)
    a0, b0 = zone_terms(md, n)
    ref, got, _, _, counts = run_both(oracle, md, st, w, a0, b0, **RESIDENT)
    assert counts[3] + counts[4] == 0, counts
    assert_state_close(md, ref, got)
    assert_all_resident(md)


@pytest.mark.parametrize("n,which", [(32, "both"), (20, "back"), (17, "both")])
def test_no_mass_facings_whose_test_reads_V(oracle, n, which):
    S = 160
    md, st = mdl.uniform_massive(S, n, Z=2, dt=45.0, seed=500 + n)
    off = md["node_offset"]
    mass, u = md["mass"].copy(), md["uvalue"].copy()
    rng = np.random.default_rng(n)
    if which == "both":
        mass[off[:-1]] = 0.0
        u[off[:-1]] = rng.uniform(0.5, 3.0, S)
    mass[off[1:] - 1] = 0.0
    u[off[1:] - 2] = rng.uniform(0.5, 3.0, S)
    md["mass"], md["uvalue"] = mass, u
    md["front_emissivity"] = md["front_emissivity"] * 0.2
    md["back_emissivity"] = md["back_emissivity"] * 0.2
    w = mdl.weather_series(20, 45.0)
    a0, b0 = zone_terms(md, n)
    ref, got, iters, gpu_iters, counts = run_both(oracle, md, st, w, a0, b0, **RESIDENT)
    assert counts[3] + counts[4] == 0, counts
    assert iters == gpu_iters and iters > 0
    assert_state_close(md, ref, got)
    assert_all_resident(md)


@pytest.mark.parametrize("walls,two_faced", [(100, True), (100, False), (33, True), (128, True), (256, True)])
def test_zone_lists_of_less_than_four_passes_four_and_two_batches(oracle, walls, two_faced):
    """One zone per workgroup, a wavefront sums it: lists of 200 sides (the fourth pass partly filled), 100 (two passes),
    66, 256 (four full passes) and, in the workgroup of eight wavefronts, 512 (eight passes)."""
    md, st = mdl.uniform_massive(3 * walls, 32, Z=3, dt=45.0, seed=walls)
    if two_faced:
        both_faces_in_the_room(md)
        mdl.set_ir_from_air(md, st, 10.0)
    w = mdl.weather_series(20, 45.0, wind_speed=3.5, wind_deg=120.0)
    a0, b0 = zone_terms(md, walls)
    ref, got, _, _, _ = run_both(oracle, md, st, w, a0, b0, **RESIDENT)
    assert_state_close(md, ref, got)
    assert_all_resident(md)


def test_walls_that_face_no_zone(oracle):
    md, st = mdl.uniform_massive(150, 32, Z=3, dt=45.0, seed=5)
    md["back_kind"][:] = mdl.OUTDOOR
    md["front_kind"][::3] = mdl.AMBIENT
    md["front_ambient"][::3] = 17.5
    w = mdl.weather_series(20, 45.0)
    ref, got, _, _, _ = run_both(oracle, md, st, w, **RESIDENT)
    assert_state_close(md, ref, got)
    assert_all_resident(md)


@pytest.mark.parametrize("walls_per_room", [12, 9, 15])
def test_rows_of_16_lanes_one_pass_and_a_second_pass_of_one_element(oracle, walls_per_room):
    """Buildings of 8 rooms: more zones than wavefronts, a row of 16 lanes per zone. A room's list holds its walls' back
    sides and the front sides of the two partitions of the room before: 14, 11 and 17 entries — the last needs a
    second pass with one element."""
    per = 8 * walls_per_room
    md, st = mdl.partitioned_buildings(4 * per, 32, rooms=8, walls_per_room=walls_per_room, partitions_per_room=2,
                                       dt=45.0, seed=walls_per_room)
    w = mdl.weather_series(13, 45.0, wind_speed=3.5, wind_deg=120.0)
    a0, b0 = zone_terms(md, walls_per_room)
    ref, got, _, _, _ = run_both(oracle, md, st, w, a0, b0, **RESIDENT)
    assert_state_close(md, ref, got)
    assert_all_resident(md)


@pytest.mark.parametrize("clusters,n_sub,facings", [(2, 3, False), (3, 4, False), (2, 4, True)])
def test_teams_of_workgroups(oracle, clusters, n_sub, facings):
    """Buildings of 40 rooms do not fit a workgroup: teams of workgroups march them and exchange the partial sums of the
    zones they share (V in registers in the all-massive team variant; with no-mass facings the team variant keeps V
    in LDS, and its LDS size is the host's fused_lds_bytes)."""
    md, st = mdl.partitioned_buildings(clusters * 480, 32, rooms=40, dt=45.0, seed=40 + clusters)
    if facings:
        S, off = md["n_surfaces"], md["node_offset"]
        mass, u = md["mass"].copy(), md["uvalue"].copy()
        mass[off[1:] - 1] = 0.0
        u[off[1:] - 2] = np.random.default_rng(9).uniform(0.5, 3.0, S)
        md["mass"], md["uvalue"] = mass, u
    w = mdl.weather_series(n_sub, 45.0, wind_speed=2.5, wind_deg=75.0)
    a0, b0 = zone_terms(md, clusters)
    ref, got, iters, gpu_iters, _ = run_both(oracle, md, st, w, a0, b0, **RESIDENT)
    assert iters == gpu_iters and (iters > 0) == facings
    assert_state_close(md, ref, got)
    assert_all_resident(md)


def test_calls_of_two_three_and_twenty_sub_timesteps_in_a_row(oracle):
    """Consecutive calls on one batch (each takes the clusters in the opposite order of the call before): every call
    loads V, its sides' places and its zones' data anew."""
    md, st = mdl.uniform_massive(300, 32, Z=3, dt=45.0, seed=77)
    both_faces_in_the_room(md)
    mdl.set_ir_from_air(md, st, 10.0)
    w = mdl.weather_series(27, 45.0, wind_speed=3.0, wind_deg=30.0)
    a0, b0 = zone_terms(md, 77)
    ref = st.copy()
    rc, _ = oracle.OracleModel(md).march(ref, w, a0, b0)
    assert rc == 0
    got = st.copy()
    with HeatBatch(md, **RESIDENT) as b:
        assert b.n_fused_surfaces == md["n_surfaces"]
        b.upload_state(got)
        b.march(got, w[:2], a0, b0)
        b.march(got, w[2:5], a0, b0)
        b.march(got, w[5:25], a0, b0)
        b.march(got, w[25:], a0, b0)
        assert b.n_fused_launches >= 4
    assert_state_close(md, ref, got)
