"""Worker of tests/test_resident_prio_queue_gpu.py (needs a GPU):   python resident_prio_queue_worker.py CASE OUT.npy

One case per process, under the parent's time limit: the library reads HEAT_AMD_FUSED_ROOM and HEAT_AMD_FUSED_PERSIST once, and a march that
never came back would otherwise take the whole suite with it. The worker builds the case's model, marches it
cluster-resident (16 nodes per lane; walls of 8 nodes: 4), asserts that every wall was marched resident, holds the
downloaded state to the oracle's march at rtol = atol = 1e-9, saves it to OUT.npy and prints one JSON line followed by "RESIDENT OK". The fused
launches are on stderr (HEAT_AMD_TRACE); the parent reads them there.

Cases (where the zone work runs at raised priority, and who draws from the work queue):
  chain               200 walls x 32 nodes, 2 zones: a wavefront per zone; wavefronts with and without a zone
  fewzones            70 walls, 1 zone: three wavefronts, the last partly filled, one zone
  rows-W              buildings of 8 rooms x W walls: a row of 16 lanes per zone, wavefronts whose rows hold no zone
  small               rooms with windows and thin partitions: small-surface wavefronts in the workgroups
  teams-ROOMS-N-W-NSUB  two buildings of ROOMS rooms x W walls of N nodes, marched by teams in one call of NSUB sub-timesteps
  queue-NSUB          ten clusters in blocks of 4, 1, 4, 3, 4, 1, 4, 3, 4 and 3 working wavefronts, two calls of NSUB
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from heat_amd import HeatBatch, modeldict as mdl
from oracle import oracle as orc
from team_rounds_worker import assert_state_close, zone_terms

DT = 45.0
RESIDENT = dict(nodes_per_lane=16, fuse_always=True)
# walls of 32 nodes take two lanes: 120 walls fill four wavefronts (the last partly), 96 three, 32 one. The planner joins
# neighbouring clusters up to four wavefronts (256 lanes): beside 240 lanes nothing fits, so every cluster is a block.
QUEUE_CLUSTERS = [120, 32, 120, 96, 120, 32, 120, 96, 120, 96]


def model_of(case):
    p = case.split("-")
    if p[0] == "chain":
        return mdl.uniform_massive(200, 32, Z=2, dt=DT, seed=61), [7]
    if p[0] == "fewzones":
        return mdl.uniform_massive(70, 32, Z=1, dt=DT, seed=62), [4]
    if p[0] == "rows":
        per = 8 * int(p[1])
        return mdl.partitioned_buildings(4 * per, 32, rooms=8, walls_per_room=int(p[1]), partitions_per_room=2, dt=DT,
                                         seed=63), [5]
    if p[0] == "small":
        return mdl.rooms_with_windows(700, Z=35, dt=DT, seed=24), [3, 4]
    if p[0] == "teams":
        rooms, n, per_room, n_sub = int(p[1]), int(p[2]), int(p[3]), int(p[4])
        return mdl.partitioned_buildings(2 * rooms * per_room, n, rooms=rooms, walls_per_room=per_room, dt=DT, seed=64), [n_sub]
    if p[0] == "queue":
        S = sum(QUEUE_CLUSTERS)
        md, st = mdl.uniform_massive(S, 32, Z=len(QUEUE_CLUSTERS), dt=DT, seed=65)
        md["back_zone"] = np.repeat(np.arange(len(QUEUE_CLUSTERS), dtype=np.int32), QUEUE_CLUSTERS)
        mdl.set_ir_from_air(md, st, 10.0)
        return (md, st), [int(p[1]), int(p[1])]
    raise SystemExit("unknown case " + case)


def options_of(case, md):
    if case == "small":
        return dict(fuse_always=True)
    if int(md["node_offset"][1]) <= 8:
        return dict(nodes_per_lane=4, fuse_always=True)
    return RESIDENT


def main():
    case, out_path = sys.argv[1], sys.argv[2]
    (md, st), calls = model_of(case)
    w = mdl.weather_series(sum(calls), DT, wind_speed=3.5, wind_deg=120.0)
    a0, b0 = zone_terms(md, 5)
    ref = st.copy()
    rc, iters = orc.OracleModel(md).march(ref, w, a0, b0)
    assert rc == 0 and np.all(np.isfinite(ref))
    got = st.copy()
    opts = options_of(case, md)
    with HeatBatch(md, **opts) as b:
        n_fused = b.n_fused_surfaces
        b.upload_state(got)
        k = 0
        for n in calls:
            b.march_resident(w[k:k + n], a0, b0)
            k += n
        b.synchronize()
        b.download_state(got)
        gpu_iters = b.nomass_iterations()
        launches = b.n_fused_launches
    np.save(out_path, got)
    print(json.dumps(dict(case=case, surfaces=md["n_surfaces"], fused_surfaces=n_fused, n_fused_launches=launches,
                          iters=iters, gpu_iters=gpu_iters)), flush=True)
    if case == "small":
        assert n_fused > md["n_surfaces"] // 2, (n_fused, md["n_surfaces"])   # (rooms of short walls are streamed)
    else:
        assert n_fused == md["n_surfaces"], (n_fused, md["n_surfaces"])       # every wall was marched resident
    assert launches >= len(calls)
    assert gpu_iters == iters, (gpu_iters, iters)
    assert_state_close(md, ref, got)
    print("RESIDENT OK", flush=True)


if __name__ == "__main__":
    main()
