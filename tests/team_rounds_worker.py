"""Worker of tests/test_team_rounds_gpu.py (needs a GPU):   python team_rounds_worker.py CASE OUT.npy

One case per process: the library reads HEAT_AMD_TEAM_ROOM (and HEAT_AMD_NO_TEAMS, HEAT_AMD_TRACE) once, so the parent sets
them in the child's environment. The worker builds the case's model, marches it on the device in calls of 1, 3, 2, 5 and 4
sub-timesteps (odd and even lengths, consecutive calls in opposite cluster order, a call of one sub-timestep), saves the
downloaded state to OUT.npy, holds it to the oracle's march of the same 15 sub-timesteps at rtol = atol = 1e-9 with equal
no-mass pass counts, and prints one JSON line of figures followed by "TEAM OK". The team launches themselves are on stderr
(HEAT_AMD_TRACE); the parent reads them there.

Cases:
  rounds-ROOMS-N-plain|faced   five buildings of ROOMS rooms, walls of N nodes (faced: no-mass facings on every third wall)
  uneven-plain|faced[-graph]   buildings of 40, 24, 32, 40, 20, 28 and 36 rooms in one batch (graph: use_graph=True)
  sites                        the same buildings, each a weather site of its own
  wrap                         two buildings of 24 rooms, 1030 calls of two sub-timesteps (the launch number in the tag wraps)
  refuse-nsub | refuse-room    a call the teams cannot march is refused with the device state untouched
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from heat_amd import HeatBatch, HeatError, modeldict as mdl
from helpers import faced_buildings, uneven_buildings, uneven_parts
from oracle import oracle as orc

RTOL = ATOL = 1e-9
CALLS = (1, 3, 2, 5, 4)
DT = 45.0
UNEVEN_ROOMS = [40, 24, 32, 40, 20, 28, 36]
UNEVEN_NODES = 20


def assert_state_close(md, ref, got):
    owned = np.zeros(len(ref), dtype=bool)
    for name, idx in (("nodes", mdl.node_slots(md)), ("hs_front", md["hs_front_slot"]), ("hs_back", md["hs_back_slot"]),
                      ("flow_front", md["flow_front_slot"]), ("flow_back", md["flow_back_slot"]),
                      ("zones", md["zone_slot"])):
        r, g = ref[idx], got[idx]
        owned[idx] = True
        assert np.all(np.isfinite(g)), name
        err = np.abs(r - g) / (ATOL + RTOL * np.abs(r))
        assert err.max() <= 1.0, "%s: worst |diff| %.3e at %d (ref %.17g, got %.17g)" % (
            name, np.abs(r - g).max(), int(err.argmax()), r[err.argmax()], g[err.argmax()])
    assert np.array_equal(ref[~owned], got[~owned], equal_nan=True)  # slots the path does not own are untouched


def zone_terms(md, seed):
    rng = np.random.default_rng(seed)
    Z = md["n_zones"]
    return rng.uniform(0., 60., Z), rng.uniform(0.1, 2., Z)


def weather(n_sub):
    return mdl.weather_series(n_sub, DT, wind_speed=3.5, wind_deg=120.0)


def march_in_calls(b, w, a0, b0, calls):
    k = 0
    for n in calls:
        b.march_resident(w[k:k + n], a0, b0)
        k += n
    assert k == len(w)
    b.synchronize()


def model_of(case):
    p = case.split("-")
    if p[0] == "rounds":
        rooms, n = int(p[1]), int(p[2])
        md, st = mdl.partitioned_buildings(5 * rooms * 12, n, rooms=rooms, dt=DT, seed=rooms + n)
    elif p[0] == "wrap":
        md, st = mdl.partitioned_buildings(2 * 24 * 12, 9, rooms=24, dt=DT, seed=33)
    else:
        md, st = uneven_buildings(UNEVEN_NODES, UNEVEN_ROOMS, seed=60)
    if "faced" in p:
        md, st = faced_buildings(md, st, every=3, seed=len(case))
    return md, st


def run_against_oracle(case, out_path):
    md, st = model_of(case)
    calls = (2,) * 1030 if case == "wrap" else CALLS
    w = weather(sum(calls))
    a0, b0 = zone_terms(md, 5)
    ref = st.copy()
    rc, iters = orc.OracleModel(md).march(ref, w, a0, b0)
    assert rc == 0 and np.all(np.isfinite(ref))
    got = st.copy()
    t0 = time.perf_counter()
    with HeatBatch(md, use_graph="graph" in case.split("-")) as b:
        n_fused = b.n_fused_surfaces
        b.upload_state(got)
        march_in_calls(b, w, a0, b0, calls)
        b.download_state(got)
        gpu_iters = b.nomass_iterations()
        launches = b.n_fused_launches
    seconds = time.perf_counter() - t0
    np.save(out_path, got)
    print(json.dumps(dict(case=case, surfaces=md["n_surfaces"], fused_surfaces=n_fused, n_fused_launches=launches,
                          iters=iters, gpu_iters=gpu_iters, march_seconds=seconds)), flush=True)
    if "HEAT_AMD_NO_TEAMS" not in os.environ:
        assert n_fused == md["n_surfaces"] and launches >= len(calls), (n_fused, launches)
    assert gpu_iters == iters, (gpu_iters, iters)
    assert iters > 0 or "faced" not in case
    assert_state_close(md, ref, got)


def run_sites(out_path):
    """Every building a weather site: a team meets another site's weather from round to round; each site is held to the
    oracle's march of its own model under its own weather (as tests/test_sites_gpu.py does)."""
    parts = uneven_parts(UNEVEN_NODES, UNEVEN_ROOMS, seed=60)
    md, site = mdl.concat([m for m, _ in parts])
    st = np.concatenate([s for _, s in parts])
    K = len(parts)
    w = mdl.weather_sites(sum(CALLS), DT, K, seed=7)
    a0, b0 = zone_terms(md, 5)
    z_off = np.concatenate(([0], np.cumsum([m["n_zones"] for m, _ in parts])))
    refs, iters = [], 0
    for k, (m, s) in enumerate(parts):
        r = s.copy()
        rc, it = orc.OracleModel(m).march(r, np.ascontiguousarray(w[:, k, :]), a0[z_off[k]:z_off[k + 1]], b0[z_off[k]:z_off[k + 1]])
        assert rc == 0
        refs.append(r)
        iters += it
    ref = np.concatenate(refs)
    got = st.copy()
    with HeatBatch(md, sites=site) as b:
        assert b.n_sites == K
        b.upload_state(got)
        march_in_calls(b, w, a0, b0, CALLS)
        b.download_state(got)
        gpu_iters = b.nomass_iterations()
        launches = b.n_fused_launches
    np.save(out_path, got)
    print(json.dumps(dict(case="sites", surfaces=md["n_surfaces"], n_fused_launches=launches, iters=iters, gpu_iters=gpu_iters)),
          flush=True)
    assert gpu_iters == iters
    assert_state_close(md, ref, got)


def run_refusal(case, out_path):
    """A call the teams cannot march is refused before anything of it is launched: the plain resident workgroup of the
    20-room building must not have marched either, so the device state is the uploaded one bit for bit."""
    md, st = model_of("uneven-plain")
    a0, b0 = zone_terms(md, 5)
    w = weather(sum(CALLS))
    with HeatBatch(md) as b:
        b.upload_state(st)
        try:
            if case == "refuse-nsub":
                b.march_resident(weather(4096), a0, b0)     # the sub-timestep field of the tag holds 4095
            else:
                b.march_resident(w[:3], a0, b0)             # legal, but the room the parent set holds no team of six
            raise AssertionError("the call was not refused")
        except HeatError as e:
            message = str(e)
        b.synchronize()
        after = np.full_like(st, np.nan)
        b.download_state(after)
        np.save(out_path, after)
        owned = np.isfinite(after)                          # (download_state writes the slots the path owns)
        moved = int(np.count_nonzero(after[owned] != st[owned]))
        print(json.dumps(dict(case=case, message=message, slots_moved=moved, slots_owned=int(owned.sum()))), flush=True)
        assert ("4095" if case == "refuse-nsub" else "not one team") in message, message
        assert owned.sum() >= md["n_zones"] + len(mdl.node_slots(md))
        assert moved == 0, "%d state slots moved by a refused call" % moved
        if case == "refuse-nsub":                           # the batch is as good as new: a legal march matches the oracle
            ref = st.copy()
            rc, iters = orc.OracleModel(md).march(ref, w, a0, b0)
            assert rc == 0
            got = st.copy()
            march_in_calls(b, w, a0, b0, CALLS)
            b.download_state(got)
            assert b.nomass_iterations() == iters
            assert_state_close(md, ref, got)


def main():
    case, out_path = sys.argv[1], sys.argv[2]
    if case == "sites":
        run_sites(out_path)
    elif case.startswith("refuse-"):
        run_refusal(case, out_path)
    else:
        run_against_oracle(case, out_path)
    print("TEAM OK", flush=True)


if __name__ == "__main__":
    main()
