"""Child process of tests/test_series_host.py: heat_series_check (heat_amd/csrc/plan.cpp, built by g++ with
AddressSanitizer + UBSan) over the generators — every slot this path owns accepted as a probe, every other slot and every
bad argument refused with its code. Started with LD_PRELOAD=libasan; any sanitizer report aborts it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heat_amd import binding, modeldict as mdl  # noqa: E402
from tests.helpers import random_zone_graph_model  # noqa: E402


def owned_slots(md):
    return np.concatenate([mdl.node_slots(md), md["hs_front_slot"], md["hs_back_slot"], md["flow_front_slot"],
                           md["flow_back_slot"], md["zone_slot"]])


def code_of(fn):
    try:
        fn()
    except binding.HeatError as e:
        return e.code, str(e)
    return 0, ""


def main(path):
    L = binding.load_host_library(path)
    rng = np.random.default_rng(7)
    models = [random_zone_graph_model(seed)[0] for seed in range(6)]
    models += [mdl.ragged_mixed(500, Z=12)[0], mdl.rooms_with_windows(400, Z=30)[0], mdl.glazing_cavity(120, Z=3)[0],
               mdl.partitioned_buildings(192, 10)[0]]
    n_checks = 0
    for md in models:
        S, n_state = int(md["n_surfaces"]), int(md["n_state"])
        own = owned_slots(md)
        w = np.zeros((6, 2, 3))
        ch = rng.random((6, 5))
        chan = rng.integers(-1, 5, (4, S)).astype(np.int32)
        gain = rng.random((4, S))
        face = np.where(chan[2] >= 0, 1, 0).astype(np.uint8) | np.where(chan[3] >= 0, 2, 0).astype(np.uint8)
        kw = dict(weather=w, n_sub=2, channel=ch, solar_front=(chan[0], gain[0]), solar_back=chan[1],
                  ir_front=(chan[2], gain[2]), ir_back=(chan[3], gain[3]), ir_own_face=face,
                  zone_a0=rng.random((6, int(md["n_zones"]))), zone_b0=rng.random((6, int(md["n_zones"]))))
        binding.series_check(md, lib=L, probes=rng.permutation(own), **kw)
        n_checks += 1
        others = np.setdiff1d(np.arange(-3, n_state + 3), own)
        for bad in rng.choice(others, 12):
            c, msg = code_of(lambda: binding.series_check(md, lib=L, probes=[own[0], bad, own[1]], **kw))
            assert c == -4 and "probe 1" in msg, (bad, c, msg)
            n_checks += 1
        q = int(rng.integers(0, S))
        bad_chan = chan.copy()
        bad_chan[1, q] = 5
        c, msg = code_of(lambda: binding.series_check(md, lib=L, **dict(kw, solar_back=bad_chan[1])))
        assert c == -4 and "surface %d" % q in msg, msg
        n_checks += 1
    print("series host check: %d checks" % n_checks)


if __name__ == "__main__":
    main(sys.argv[1])
