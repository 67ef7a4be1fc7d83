"""Series march (heat_batch_march_series) against the per-call path, on the headline model (1 M walls x 32 nodes, 10 000
zones): 64 channels, every surface driven on all four inputs, probes = all zones; n_sub = 2 and 20. Three legs, alternated
in one process, host clock around work that ends in a synchronisation:
  A  per-call drop-in: heat_batch_march_ex(SURFACE_SCALARS | ZONE_TEMPERATURES) per step, numpy writing the inputs into the
     caller's state between the calls (reported with and without the time numpy takes: a compiled host writes faster)
  B  march_resident alone, same n_sub, nothing driven, one synchronisation at the end: the floor
  C  march_series: one call for all steps, schedules uploaded inside the clock
Prints ms per step of each, C / A and C - B (also without the set-up of the call, from a series of one step), and writes profiles/series_march.json.
  python tools/series.py [S] [steps] [rounds] [--out=FILE]
  python tools/series.py --one-series [S] [steps]    one warm-up series and one more of n_sub = 2, nothing else (to run
                                                     under rocprofv3 --kernel-trace --stats)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from heat_amd import HeatBatch, modeldict as mdl
ONE = "--one-series" in sys.argv
OUT = next((a[6:] for a in sys.argv[1:] if a.startswith("--out=")), None)
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(ARGS[0]) if len(ARGS) > 0 else 1_000_000
STEPS = int(ARGS[1]) if len(ARGS) > 1 else 100
ROUNDS = int(ARGS[2]) if len(ARGS) > 2 else 3
N_CHANNELS = 64
KEYS = ("solar_front", "solar_back", "ir_front", "ir_back")

md, st0 = mdl.uniform_massive(S, n=32, Z=max(1, S // 100), dt=45.0)
rng = np.random.default_rng(1)
channel = np.concatenate([rng.uniform(0.0, 600.0, (STEPS, N_CHANNELS // 2)), rng.uniform(300.0, 450.0, (STEPS, N_CHANNELS // 2))], axis=1)
drives = {k: ((rng.integers(0, N_CHANNELS // 2, S) + (N_CHANNELS // 2 if i >= 2 else 0)).astype(np.int32), rng.uniform(0.5, 1.5, S))
          for i, k in enumerate(KEYS)}
probes = md["zone_slot"]


def leg_a(b, state, w, n_sub, steps):
    """(ms per step in the calls alone, ms per step with numpy's writes)"""
    in_calls, t_all = 0.0, time.perf_counter()
    for k in range(steps):
        for key in KEYS:
            chan, gain = drives[key]
            state[md[key + "_slot"]] = gain * channel[k, chan]
        t0 = time.perf_counter()
        b.march(state, w[k], outputs=b.OUT_SCALARS | b.OUT_ZONES)
        in_calls += time.perf_counter() - t0
    return in_calls * 1e3 / steps, (time.perf_counter() - t_all) * 1e3 / steps


def leg_b(b, w, steps):
    b.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        b.march_resident(w[k])
    b.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def leg_c(b, w, n_sub, steps):
    b.synchronize()
    t0 = time.perf_counter()
    trace, failed = b.march_series(w[:steps], n_sub, channel=channel[:steps], probes=probes, **drives)
    dt = time.perf_counter() - t0
    assert failed == -1 and np.all(np.isfinite(trace))
    return dt * 1e3 / steps


result = dict(model="uniform_massive(%d, 32, Z=%d)" % (S, md["n_zones"]), channels=N_CHANNELS, steps=STEPS, rounds=ROUNDS,
              probes=int(len(probes)), legs={})
with HeatBatch(md) as b:
    state = st0.copy()
    b.upload_state(state)
    for n_sub in ((2,) if ONE else (2, 20)):
        w = mdl.weather_series(STEPS * n_sub, 45.0).reshape(STEPS, n_sub, 3)
        leg_c(b, w, n_sub, min(STEPS, 10))  # warm-up
        if ONE:
            print("one series: %.3f ms per step" % leg_c(b, w, n_sub, STEPS))
            continue
        leg_b(b, w, 5)
        leg_a(b, state, w, n_sub, 3)
        a, a_np, bb, c, c1 = [], [], [], [], []
        for r in range(ROUNDS):
            x, y = leg_a(b, state, w, n_sub, min(STEPS, 50))
            a.append(x), a_np.append(y)
            bb.append(leg_b(b, w, STEPS))
            c.append(leg_c(b, w, n_sub, STEPS))
            c1.append(leg_c(b, w, n_sub, 1))  # a series of ONE step: the set-up of a call (tables built and uploaded) + a step
        A, A_np, B, Cc, C1 = float(np.median(a)), float(np.median(a_np)), float(np.median(bb)), float(np.median(c)), float(np.median(c1))
        steady = (Cc * STEPS - C1) / (STEPS - 1) - B  # what a step costs over the floor once the call is set up
        result["legs"]["n_sub=%d" % n_sub] = dict(
            A_per_call_ms=A, A_with_numpy_writes_ms=A_np, B_resident_ms=B, C_series_ms=Cc, C_over_A=Cc / A, C_minus_B_ms=Cc - B,
            C_series_of_one_step_ms=C1, C_minus_B_without_setup_ms=steady, all_rounds=dict(A=a, A_with_numpy=a_np, B=bb, C=c, C_one_step=c1))
        print("n_sub %2d: A per-call %.3f ms/step (%.3f with numpy's writes), B resident %.3f, C series %.3f -> C / A = %.3f, "
              "C - B = %.3f ms (%.3f without the call's set-up: a series of one step takes %.2f ms; %d steps, median of %d rounds)" % (
                  n_sub, A, A_np, B, Cc, Cc / A, Cc - B, steady, C1, STEPS, ROUNDS), flush=True)
if not ONE:
    out = OUT or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "series_march.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out)
