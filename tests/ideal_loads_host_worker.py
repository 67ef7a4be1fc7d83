"""Child process of tests/test_ideal_loads_host.py: heat_ideal_loads_check (heat_amd/csrc/plan.cpp, built by g++ with
AddressSanitizer + UBSan) over the generators — random ideal loads accepted, every kind of bad load refused with its code
and its number, the load_of_zone table built and verified. Started with LD_PRELOAD=libasan; any sanitizer report aborts it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heat_amd import binding, modeldict as mdl  # noqa: E402
from tests.helpers import random_zone_graph_model  # noqa: E402

NC = 7


def code_of(fn):
    try:
        fn()
    except binding.HeatError as e:
        return e.code, str(e)
    return 0, ""


def random_ideal(rng, Z, n):
    heat = rng.integers(-1, NC, n)
    cool = np.where(heat < 0, rng.integers(0, NC, n), rng.integers(-1, NC, n))
    cap = lambda: np.where(rng.random(n) < 0.3, np.inf, rng.random(n) * 2000.0)
    return dict(zone=rng.permutation(Z)[:n], heat_chan=heat, cool_chan=cool, heat_cap=cap() if n % 2 else None, cool_cap=cap())


def changed(ideal, key, i, value):
    out = dict(ideal)
    a = np.array(out[key], dtype=np.float64 if key.endswith("cap") else np.int64)
    a[i] = value
    out[key] = a
    return out


def main(path):
    L = binding.load_host_library(path)
    rng = np.random.default_rng(12)
    models = [random_zone_graph_model(seed)[0] for seed in range(6)]
    models += [mdl.ragged_mixed(500, Z=12)[0], mdl.rooms_with_windows(400, Z=30)[0], mdl.partitioned_buildings(192, 10)[0]]
    n_checks = 0
    for md in models:
        Z = int(md["n_zones"])
        series = dict(weather=np.zeros((3, 2, 3)), n_sub=2, channel=np.zeros((3, NC)))
        for n in sorted({1, max(1, Z // 2), Z}):
            ideal = random_ideal(rng, Z, n)
            binding.ideal_loads_check(md, lib=L, ideal=ideal, **series)
            n_checks += 1
            i = int(rng.integers(0, n))
            bad = [("zone", Z, -4), ("zone", -1, -4), ("heat_chan", NC, -4), ("heat_chan", -2, -4), ("cool_chan", NC + 5, -4),
                   ("cool_cap", -1.0, -1), ("cool_cap", np.nan, -1)]
            if ideal["heat_cap"] is not None:
                bad += [("heat_cap", -1e-300, -1), ("heat_cap", np.nan, -1)]
            if n > 1:
                bad.append(("zone", int(ideal["zone"][(i + 1) % n]), -1))  # a second load on a zone
            for key, value, want in bad:
                c, msg = code_of(lambda: binding.ideal_loads_check(md, lib=L, ideal=changed(ideal, key, i, value), **series))
                # (the second load on a zone is named by the later of the two)
                dup = key == "zone" and want == -1
                assert c == want and "ideal load %d" % (max(i, (i + 1) % n) if dup else i) in msg, (key, value, c, msg)
                n_checks += 1
            neither = changed(changed(ideal, "heat_chan", i, -1), "cool_chan", i, -1)
            c, msg = code_of(lambda: binding.ideal_loads_check(md, lib=L, ideal=neither, **series))
            assert c == -4 and "ideal load %d" % i in msg, (c, msg)
            n_checks += 1
        binding.ideal_loads_check(md, lib=L, ideal={}, **series)
        n_checks += 1
    print("ideal loads host check: %d checks" % n_checks)


if __name__ == "__main__":
    main(sys.argv[1])
