"""Child process of tests/test_sites_host.py: the planner (heat_amd/csrc/plan.cpp, built by g++ with AddressSanitizer +
UBSan) over the generators with random weather-site assignments, every plan verified by heat_plan_check_sites (every
tile, cluster-resident workgroup and team of one site). Started with LD_PRELOAD=libasan; any sanitizer report aborts it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heat_amd import binding, modeldict as mdl  # noqa: E402
from tests.helpers import random_zone_graph_model  # noqa: E402

OPTS = (dict(), dict(no_fusion=True), dict(fuse_always=True), dict(fuse_always=True, nodes_per_lane=4),
        dict(fuse_always=True, nodes_per_lane=8), dict(nodes_per_lane=16), dict(no_palette=True), dict(force_general=True))


def cluster_sites(md, n_sites, rng):
    """A site per zone-connected cluster (what a stock of separate buildings has), plus a few surfaces moved to another
    site (mixed-site clusters: legal, streamed)."""
    Z = int(md["n_zones"])
    parent = np.arange(max(Z, 1))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    fk, bk, fz, bz = md["front_kind"], md["back_kind"], md["front_zone"], md["back_zone"]
    for s in range(int(md["n_surfaces"])):
        if fk[s] == mdl.SPACE and bk[s] == mdl.SPACE:
            a, b = find(int(fz[s])), find(int(bz[s]))
            parent[max(a, b)] = min(a, b)
    zone_site = rng.integers(0, n_sites, max(Z, 1))
    site = np.empty(int(md["n_surfaces"]), dtype=np.int32)
    for s in range(len(site)):
        z = int(bz[s]) if bk[s] == mdl.SPACE else (int(fz[s]) if fk[s] == mdl.SPACE else -1)
        site[s] = zone_site[find(z)] if z >= 0 else rng.integers(0, n_sites)
    moved = rng.random(len(site)) < 0.03
    site[moved] = rng.integers(0, n_sites, int(moved.sum()))
    return site


def main(path):
    L = binding.load_host_library(path)
    rng = np.random.default_rng(2026)
    n_plans = 0
    models = [random_zone_graph_model(seed)[0] for seed in range(12)]
    models += [gen(**kw)[0] for gen, kw in (
        (mdl.ragged_mixed, dict(S=2000, Z=30)), (mdl.clustered_massive, dict(S=2000, Z=80)),
        (mdl.rooms_with_windows, dict(S=1500, Z=100)), (mdl.glazing_cavity, dict(S=300, Z=4)),
        (mdl.partitioned_buildings, dict(S=1920, n=12)), (mdl.uniform_massive, dict(S=2000, n=32, Z=30)))]
    for md in models:
        S = int(md["n_surfaces"])
        ref = {i: binding.plan_check(md, lib=L, **o) for i, o in enumerate(OPTS)}
        for i, o in enumerate(OPTS):  # one site: the plan of a batch without sites
            assert binding.plan_check_sites(md, 1, np.zeros(S, np.int32), lib=L, **o) == ref[i]
            n_plans += 1
        for n_sites in (2, 7, 300):
            for site in (rng.integers(0, n_sites, S).astype(np.int32), cluster_sites(md, n_sites, rng)):
                for o in OPTS:
                    summary = binding.plan_check_sites(md, n_sites, site, lib=L, **o)
                    assert sum(summary[:5]) == S
                    n_plans += 1
    # joined models, sites listed model after model and alternately
    parts = [mdl.clustered_massive(300, Z=12, seed=1)[0], mdl.rooms_with_windows(200, Z=8)[0],
             mdl.glazing_cavity(60, Z=2)[0], mdl.partitioned_buildings(192, 10)[0]]
    for interleave in (False, True):
        md, site = mdl.concat(parts, interleave=interleave)
        for o in OPTS:
            binding.plan_check_sites(md, len(parts), site, lib=L, **o)
            n_plans += 1
    print("sites host check: %d plans verified" % n_plans)


if __name__ == "__main__":
    main(sys.argv[1])
