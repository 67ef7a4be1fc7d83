"""The zone balance of the cluster-resident march (fused_zone_phase, no teams) at the smallest shapes that reach every
path of it: the wavefront that owns a zone reads the zone's data and the first two gather passes of its list together
(lists of one pass, of exactly 64 entries, of two passes, of 128 entries, and longer ones that run the loop behind
the two passes), several zones with a wavefront each and a wavefront left without one, the rows of 16 lanes (one
16-entry pass, two, and the zone loop run twice at kFusedMaxZones zones), the switch between the two branches, a zone
whose |b| stays under 1e-9 and keeps its temperature, a partly filled last lane, and persistent workgroups on the queue.

Walls of 32 nodes at 16 nodes per lane (two lanes a wall) unless noted, fuse_always; every case asserts that the resident
march took all its walls. 7 sub-timesteps with non-zero a0 and b0, the march cut into calls of 3 + 1 + 3. Held to the
oracle at the project's RTOL = ATOL = 1e-9 and to the same model with no_fusion=True at rtol = atol = 1e-11
(both as in test_parity_gpu)."""
import numpy as np
import pytest

from heat_amd import HeatBatch
from heat_amd import modeldict as mdl
from test_parity_gpu import assert_state_close

pytestmark = pytest.mark.gpu

RESIDENT = dict(nodes_per_lane=16, fuse_always=True)


def zone_terms(md, seed):
    rng = np.random.default_rng(seed)
    Z = md["n_zones"]
    return rng.uniform(1., 60., Z), rng.uniform(0.1, 2., Z)


def both_faces_in_the_room(md, st):
    """Every wall stands inside its zone: front and back face it, two entries of the zone's list per wall."""
    md["front_kind"] = np.full(md["n_surfaces"], mdl.SPACE, dtype=np.int32)
    md["front_zone"] = md["back_zone"].copy()
    mdl.set_ir_from_air(md, st, 10.0)


def march_in_calls(md, st, w, a0, b0, cuts, **opts):
    got = st.copy()
    with HeatBatch(md, **opts) as b:
        n_fused = b.n_fused_surfaces
        b.upload_state(got)
        for lo, hi in zip((0,) + cuts, cuts + (len(w),)):
            b.march(got, w[lo:hi], a0, b0)
    return got, n_fused


def check(oracle, md, st, a0, b0, n_sub=7, cuts=(3, 4), wind_speed=3.5, against_oracle=True):
    w = mdl.weather_series(n_sub, float(md["dt"]), wind_speed=wind_speed, wind_deg=120.0)
    got, n_fused = march_in_calls(md, st, w, a0, b0, cuts, **RESIDENT)
    assert n_fused == md["n_surfaces"]
    if against_oracle:
        ref = st.copy()
        rc, _ = oracle.OracleModel(md).march(ref, w, a0, b0)
        assert rc == 0
        assert_state_close(md, ref, got)
    streamed, n_streamed_fused = march_in_calls(md, st, w, a0, b0, cuts, nodes_per_lane=16, no_fusion=True)
    assert n_streamed_fused == 0
    assert np.allclose(got, streamed, rtol=1e-11, atol=1e-11)
    return got


@pytest.mark.parametrize("walls", [1, 63, 64, 65, 100, 128])
def test_one_zone_a_wavefront_sums_it_gather_boundaries(oracle, walls):
    """One pass (1, 63), the 64-entry edge, two passes (65, 100) and the full list of the unrolled part (128)."""
    md, st = mdl.uniform_massive(walls, 32, Z=1, dt=45.0, seed=600 + walls)
    a0, b0 = zone_terms(md, walls)
    check(oracle, md, st, a0, b0)


@pytest.mark.parametrize("walls,zones", [(120, 4), (90, 3), (120, 3)])
def test_several_zones_one_per_wavefront(oracle, walls, zones):
    """Four zones of 30 walls on four wavefronts; three zones of 30 (90 walls fill three wavefronts: the workgroup's fourth
    has neither walls nor a zone); three zones of 40 on four wavefronts with walls: the fourth has no zone of its own."""
    md, st = mdl.uniform_massive(walls, 32, Z=zones, dt=45.0, seed=610 + zones + walls)
    a0, b0 = zone_terms(md, zones)
    check(oracle, md, st, a0, b0)


def test_lists_of_more_than_128_entries_run_the_loop_behind_the_two_passes(oracle):
    """65 walls whose front and back both face the one zone: 128 entries from 64 walls and two more, 130."""
    md, st = mdl.uniform_massive(65, 32, Z=1, dt=45.0, seed=620)
    both_faces_in_the_room(md, st)
    a0, b0 = zone_terms(md, 620)
    check(oracle, md, st, a0, b0)


@pytest.mark.parametrize("zones,walls_per_zone", [(8, 10), (7, 17), (32, 3)])
def test_rows_of_16_lanes(oracle, zones, walls_per_zone):
    """More zones than wavefronts, a row of 16 lanes per zone: one 16-entry pass (10 walls), two passes per row (17), and
    32 zones (more than the 16 rows of four wavefronts: the zone loop runs twice, at the kFusedMaxZones cap)."""
    md, st = mdl.uniform_massive(zones * walls_per_zone, 32, Z=zones, dt=45.0, seed=630 + zones)
    a0, b0 = zone_terms(md, zones)
    check(oracle, md, st, a0, b0)


@pytest.mark.parametrize("zones,walls_per_zone", [(4, 20), (5, 20), (4, 25)])
def test_switch_between_a_wavefront_and_a_row_per_zone(oracle, zones, walls_per_zone):
    """Around the switch between the two branches. Walls take two lanes, so 4 zones of 20 walls are three wavefronts
    (one zone more than wavefronts: rows), 5 zones of 20 four wavefronts (rows again), and 4 zones of 25 four wavefronts
    with four zones: as many zones as wavefronts, a wavefront each."""
    md, st = mdl.uniform_massive(zones * walls_per_zone, 32, Z=zones, dt=45.0, seed=640 + zones + walls_per_zone)
    a0, b0 = zone_terms(md, zones)
    check(oracle, md, st, a0, b0)


def test_a_zone_with_b_under_1e_9_keeps_its_temperature(oracle):
    """Walls of 1e-12 m2 and b0 = 0: |b| <= 1e-9, the zone's future temperature is its current one (ft = tc), as the
    oracle's. The zone beside it has ordinary walls. No wind: a forced coefficient goes with sqrt(perimeter / area)."""
    md, st = mdl.uniform_massive(60, 32, Z=2, dt=45.0, seed=650)
    tiny = md["back_zone"] == 0
    md["area"] = np.where(tiny, 1e-12, md["area"])
    md["perimeter"] = np.where(tiny, 4e-6, md["perimeter"])
    a0, b0 = zone_terms(md, 650)
    b0[0] = 0.0
    got = check(oracle, md, st, a0, b0, wind_speed=0.0)
    zs = np.asarray(md["zone_slot"])
    assert got[zs[0]] == st[zs[0]]
    assert got[zs[1]] != st[zs[1]]


def test_a_partly_filled_last_lane(oracle):
    """The 100-wall zone with walls of 20 nodes: 16 nodes in the first lane of a wall, 4 in the second."""
    md, st = mdl.uniform_massive(100, 20, Z=1, dt=45.0, seed=660)
    a0, b0 = zone_terms(md, 660)
    check(oracle, md, st, a0, b0)


def test_persistent_workgroups_on_the_queue():
    """600 zones of 100 walls in one call of 12 sub-timesteps: more blocks than the chip holds at once, so persistent
    workgroups take them from the work queue. Against the streamed march only."""
    md, st = mdl.uniform_massive(60000, 32, Z=600, dt=45.0, seed=670)
    a0, b0 = zone_terms(md, 670)
    check(None, md, st, a0, b0, n_sub=12, cuts=(), against_oracle=False)
