"""Child process of tests/test_sky_host.py: heat_sky_check (heat_amd/csrc/plan.cpp, built by g++ with AddressSanitizer +
UBSan) over the generators — random skies accepted (also with sites, without steps, with an all-zero mode and then without
normals and records), every kind of bad sky refused with its code and its surface. Started with LD_PRELOAD=libasan; any
sanitizer report aborts it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heat_amd import binding, modeldict as mdl  # noqa: E402
from tests.helpers import random_zone_graph_model  # noqa: E402

NC, N_STEPS = 7, 3
INPUTS = ("solar_front", "solar_back", "ir_front", "ir_back")


def code_of(fn):
    try:
        fn()
    except binding.HeatError as e:
        return e.code, str(e)
    return 0, ""


def random_case(rng, S, n_sites):
    """A series whose channels drive some inputs, and a sky on some of the others."""
    mode = rng.integers(0, 16, S).astype(np.uint8)
    mode[rng.random(S) < 0.3] = 0
    series = dict(weather=np.zeros((N_STEPS, 2, n_sites, 3)), n_sub=2, channel=np.zeros((N_STEPS, NC)))
    for bit, name in enumerate(INPUTS):
        chan = rng.integers(-1, NC, S).astype(np.int32)
        chan[(mode >> bit & 1) != 0] = -1
        if bit != 1:                                     # (one input without a channel array at all)
            series[name] = (chan, rng.random(S)) if bit % 2 else chan
    sky = dict(record=rng.normal(size=(N_STEPS, n_sites, 8)), mode=mode, normals=tuple(rng.normal(size=(3, S))))
    return series, sky


def main(path):
    L = binding.load_host_library(path)
    rng = np.random.default_rng(21)
    models = [random_zone_graph_model(seed)[0] for seed in range(6)]
    models += [mdl.ragged_mixed(500, Z=12)[0], mdl.rooms_with_windows(400, Z=30)[0], mdl.partitioned_buildings(192, 10)[0]]
    n_checks = 0
    for i, md in enumerate(models):
        S = int(md["n_surfaces"])
        n_sites = 1 + i % 3
        series, sky = random_case(rng, S, n_sites)
        used = np.flatnonzero(sky["mode"])
        assert len(used) and len(used) < S
        binding.sky_check(md, sky, n_sites=n_sites, lib=L, **series)
        binding.sky_check(md, dict(sky, normals=None), n_sites=n_sites, lib=L, **series)          # the model's normals
        binding.sky_check(md, dict(sky, record=None, normals=None, mode=np.zeros(S, np.uint8)), n_sites=n_sites, lib=L, **series)
        binding.sky_check(md, dict(sky, record=None), n_sites=n_sites, lib=L, **dict(series, weather=np.zeros((0, n_sites, 3)), channel=np.zeros((0, NC))))
        n_checks += 4
        q = int(used[rng.integers(0, len(used))])
        bit = int(np.flatnonzero([sky["mode"][q] >> a & 1 for a in range(4)])[0])

        def normals_with(axis, value):
            n = [a.copy() for a in sky["normals"]]
            n[axis][q] = value
            return n

        def mode_with(value):
            m = sky["mode"].copy()
            m[q] = value
            return m

        def channel_on(name):
            v = series.get(name)
            chan = (v[0] if isinstance(v, tuple) else v).copy() if v is not None else np.full(S, -1, np.int32)
            chan[q] = NC - 1
            return (chan, v[1]) if isinstance(v, tuple) else chan

        bad = [(dict(sky, mode=mode_with(16 + int(rng.integers(0, 240)))), series, -1),
               (dict(sky, normals=normals_with(int(rng.integers(0, 3)), np.nan)), series, -1),
               (dict(sky, normals=normals_with(int(rng.integers(0, 3)), -np.inf)), series, -1),
               (sky, dict(series, **{INPUTS[bit]: channel_on(INPUTS[bit])}), -4)]
        for k, s, want in bad:
            c, msg = code_of(lambda: binding.sky_check(md, k, n_sites=n_sites, lib=L, **s))
            assert c == want and "surface %d:" % q in msg, (want, c, msg)
            n_checks += 1
        # a NULL record with steps to march: the first surface that takes something from the sky is named
        c, msg = code_of(lambda: binding.sky_check(md, dict(sky, record=None), n_sites=n_sites, lib=L, **series))
        assert c == -1 and "surface %d:" % used[0] in msg, (c, msg)
        n_checks += 1
    print("sky host check: %d checks" % n_checks)


if __name__ == "__main__":
    main(sys.argv[1])
