"""Child process of tests/test_series_report_host.py: heat_series_report_check (heat_amd/csrc/plan.cpp, built by g++ with
AddressSanitizer + UBSan) over the generators — reports whose groups are empty, of one entry, around one segment and of
many segments, with and without weights, are accepted (the check builds the group tables and verifies them against the
offsets); every kind of bad report is refused with its code and the number of the group or entry. Started with
LD_PRELOAD=libasan; any sanitizer report aborts it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heat_amd import binding, modeldict as mdl  # noqa: E402
from tests.helpers import random_zone_graph_model  # noqa: E402

NC = 4
SEGMENT, ROW = 1024, 64  # plan.hpp: kGroupSegment, kGroupRowEntries


def code_of(fn):
    try:
        fn()
    except binding.HeatError as e:
        return e.code, str(e)
    return 0, ""


def all_slots(md):
    return np.concatenate([mdl.node_slots(md), md["hs_front_slot"], md["hs_back_slot"], md["flow_front_slot"],
                           md["flow_back_slot"], md["zone_slot"]]).astype(np.int64)


def main(path):
    L = binding.load_host_library(path)
    rng = np.random.default_rng(13)
    models = [random_zone_graph_model(seed)[0] for seed in range(4)]
    models += [mdl.ragged_mixed(500, Z=12)[0], mdl.rooms_with_windows(400, Z=30)[0]]
    n_checks = 0
    for md in models:
        Z = int(md["n_zones"])
        pool = all_slots(md)
        series = dict(weather=np.zeros((3, 2, 3)), n_sub=2, channel=np.zeros((3, NC)), probes=md["zone_slot"])
        loads = dict(thermostats=dict(sensor_zone=[0], target_zone=[Z - 1], heat_chan=[0], cool_chan=[-1], heat_power=[1.0],
                                      cool_power=[0.0], band=[0.5]))
        sizes = [0, 1, 7, ROW - 1, ROW, ROW + 1, SEGMENT - 1, SEGMENT, SEGMENT + 1, 5 * SEGMENT + 17, 0, 3]
        for weighted in (False, True):
            groups = []
            for n in sizes:
                slots = pool[rng.integers(0, len(pool), n)]          # (with repeats: a slot may enter a group twice)
                groups.append((slots, rng.normal(size=n)) if weighted else slots)
            Q = Z + len(groups)
            report = dict(groups=groups, stats=binding.Q_STATS, limits=dict(lo=rng.normal(size=Q), hi=rng.normal(size=Q)),
                          thermostat_stats=binding.TH_STATS, group_trace=True)
            binding.series_report_check(md, lib=L, report=report, loads=loads, **series)
            binding.series_report_check(md, lib=L, report=dict(report, groups=groups[::-1]), loads=loads, **series)
            n_checks += 2
            n_entries = sum(sizes)
            i = int(rng.integers(0, n_entries))
            flat = np.concatenate([g[0] if weighted else g for g in groups])
            off = np.concatenate([[0], np.cumsum(sizes)])
            weights = np.concatenate([g[1] for g in groups]) if weighted else np.ones(n_entries)
            for slot, weight, want in ((int(md["solar_front_slot"][0]), 1.0, -4), (-7, 1.0, -4), (int(md["n_state"]), 1.0, -4),
                                       (None, np.nan, -1), (None, -np.inf, -1)):
                s2, w2 = flat.copy(), weights.copy()
                if slot is not None:
                    s2[i] = slot
                w2[i] = weight if slot is None else w2[i]
                bad = dict(report, groups=dict(offset=off, slot=s2, weight=w2))
                c, msg = code_of(lambda: binding.series_report_check(md, lib=L, report=bad, loads=loads, **series))
                assert c == want and "group entry %d" % i in msg, (slot, weight, c, msg)
                n_checks += 1
            g = int(rng.integers(1, len(sizes)))
            off2 = off.copy()
            off2[g + 1] = off2[g] - 1
            r, keep = binding.make_report(n_probes=Z, groups=dict(offset=off, slot=flat))
            r.group_offset = off2.ctypes.data_as(binding._i64p)
            desc, dkeep = binding.make_desc(md)
            s, skeep = binding.make_series(**series)
            assert L.heat_series_report_check(binding.C.byref(desc), binding.C.byref(s), None, binding.C.byref(r)) == -1
            assert ("group %d" % g) in L.heat_last_error().decode()
            n_checks += 1
        c, msg = code_of(lambda: binding.series_report_check(md, lib=L, report=dict(thermostat_stats=("switches",)), **series))
        assert c == -1 and "thermostat" in msg
        binding.series_report_check(md, lib=L, report={}, **series)
        n_checks += 2
    print("series report host check: %d checks" % n_checks)


if __name__ == "__main__":
    main(sys.argv[1])
