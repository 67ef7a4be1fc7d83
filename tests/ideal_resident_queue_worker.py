"""Worker of tests/test_ideal_resident_gpu.py, the work queue (needs a GPU):   python ideal_resident_queue_worker.py NSUB OUT.npz [CASE]
(CASE, for tests/test_ideal_variants_gpu.py: a case of tests/ideal_variants_cases.py in place of the ten clusters — see variant().)

One case per process, under the parent's time limit: the library reads HEAT_AMD_FUSED_ROOM and HEAT_AMD_FUSED_PERSIST once,
and a march that never came back would otherwise take the whole suite with it. The worker builds the ten clusters of
tests/resident_prio_queue_worker.py (blocks of 4, 1, 4, 3, 4, 1, 4, 3, 4 and 3 working wavefronts), puts ideal loads on nine
of its ten zones — heating, cooling and both, some capacities small enough to saturate — and marches two consecutive ideal
series of N_STEPS steps of NSUB sub-timesteps resident, the second resumed from the first. It asserts that the batch was
eligible and every wall resident, that the loads acted and saturated in part, and that the accumulators are a plain loop
over the returned rows; it saves trace, ideal_q, accumulators and the final state to OUT.npz and prints "IDEAL RESIDENT OK".
The fused launches are on stderr (HEAT_AMD_TRACE); the parent reads them there and compares the arrays of two children."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_STEPS = 3  # steps of each of the two series


def main():
    import numpy as np

    from heat_amd import HeatBatch, modeldict as mdl
    from ideal_loads_ref import accumulate
    from resident_prio_queue_worker import DT, RESIDENT, model_of

    n_sub, out_path = int(sys.argv[1]), sys.argv[2]
    if len(sys.argv) > 3:
        return variant(sys.argv[3], n_sub, out_path)
    (md, st), _ = model_of("queue-%d" % n_sub)
    Z = int(md["n_zones"])
    n_steps = 2 * N_STEPS
    w = mdl.weather_series(n_steps * n_sub, DT, wind_speed=3.5, wind_deg=120.0).reshape(n_steps, n_sub, 3)
    t_mid = float(np.median(st[md["zone_slot"]]))
    # channels: a heating setpoint above the zones, a cooling setpoint below them, both with a step change
    late = np.arange(n_steps) >= N_STEPS + 1
    channel = np.stack([np.where(late, t_mid + 6.0, t_mid + 3.0), np.where(late, t_mid - 5.0, t_mid - 2.0)], axis=1)
    zone = np.array([z for z in range(Z) if z != 4], dtype=np.int32)[::-1].copy()       # nine of ten zones, not in order
    n = len(zone)
    kind = np.arange(n) % 3                                                           # heating only, cooling only, both
    ideal = dict(zone=zone, heat_chan=np.where(kind != 1, 0, -1).astype(np.int32), cool_chan=np.where(kind == 1, 1, -1).astype(np.int32),
                 heat_cap=np.where(np.arange(n) % 2 == 0, 400.0, np.inf), cool_cap=np.where(np.arange(n) % 4 == 1, 300.0, np.inf))
    ideal["cool_chan"][kind == 2] = -1                                                  # (heating above cooling: "both" heats only here)
    got = st.copy()
    with HeatBatch(md, ideal_resident=True, **RESIDENT) as b:
        assert b.ideal_resident == 1 and b.n_fused_surfaces == md["n_surfaces"]
        b.upload_state(got)
        kw = lambda s: dict(channel=channel[s], probes=md["zone_slot"])
        first = b.march_series(w[:N_STEPS], n_sub, ideal=ideal, **kw(slice(0, N_STEPS)))
        second = b.march_series(w[N_STEPS:], n_sub, ideal=dict(ideal, resume=first["ideal"], step_base=N_STEPS), **kw(slice(N_STEPS, None)))
        b.download_state(got)
        launches = b.n_fused_launches
    assert first["failed_step"] == -1 and second["failed_step"] == -1
    assert launches == n_steps, launches                                                # one list, one launch per step
    ideal_q = np.concatenate([first["ideal_q"], second["ideal_q"]])
    trace = np.concatenate([first["trace"], second["trace"]])
    acc = second["ideal"]
    assert (ideal_q > 0).any() and (ideal_q < 0).any()
    sat = acc["n_sat_heating"] + acc["n_sat_cooling"]
    assert 0 < sat.sum() < n * n_steps * n_sub and (sat == 0).any()
    want = accumulate(ideal_q)
    for k in want:
        assert np.array_equal(want[k], acc[k]), k
    assert np.array_equal(trace[:, 4] != trace[:, 4], np.zeros(n_steps, dtype=bool))    # (the zone without a load floats, finite)
    np.savez(out_path, trace=trace, ideal_q=ideal_q, state=got, **{k: np.asarray(v) for k, v in acc.items()})
    print("IDEAL RESIDENT OK", flush=True)


def variant(name, n_sub, out_path):
    """A case of tests/ideal_variants_cases.py (its model, its loads, an ideal load on every zone placed from the CPU
    reference) instead of the ten clusters: one workgroup list of another instantiation, more blocks than the room the
    parent leaves. The same two series, the second resumed from the first; the same assertions and the same OUT.npz, plus
    the thermostats' applied powers and modes."""
    import numpy as np

    import ideal_variants_cases as ivc
    from heat_amd import HeatBatch
    from ideal_loads_ref import accumulate
    from oracle import oracle
    from test_series_gpu import series_kwargs

    oracle.lib()
    n_steps = 2 * N_STEPS
    c = ivc.build(oracle, name, n_steps, n_sub)
    md, st, channel, drives, probes, a0, b0, loads, ideal, w = c.args
    n = len(ideal["zone"])
    got = st.copy()
    with HeatBatch(md, ideal_resident=True, **c.opts) as b:
        assert b.ideal_resident == 1 and b.n_fused_surfaces == md["n_surfaces"]
        b.upload_state(got)
        kw = lambda s: series_kwargs(channel, drives, probes, a0, b0, steps=s)
        first = b.march_series(w[:N_STEPS], n_sub, loads=loads, ideal=ideal, **kw(slice(0, N_STEPS)))
        loads2 = dict(loads, thermostats=dict(loads["thermostats"], mode=first["modes"]))
        second = b.march_series(w[N_STEPS:], n_sub, loads=loads2, ideal=dict(ideal, resume=first["ideal"], step_base=N_STEPS),
                                **kw(slice(N_STEPS, None)))
        b.download_state(got)
        launches = b.n_fused_launches
    assert first["failed_step"] == -1 and second["failed_step"] == -1
    assert launches == n_steps, launches                                                # one list, one launch per step
    ideal_q, trace, applied = (np.concatenate([first[k], second[k]]) for k in ("ideal_q", "trace", "applied"))
    acc = second["ideal"]
    assert (ideal_q > 0).any() and (ideal_q < 0).any()
    sat = acc["n_sat_heating"] + acc["n_sat_cooling"]
    assert 0 < sat.sum() < n * n_steps * n_sub and (sat == 0).any()
    want = accumulate(ideal_q)
    for k in want:
        assert np.array_equal(want[k], acc[k]), k
    assert np.all(np.isfinite(trace))
    np.savez(out_path, trace=trace, ideal_q=ideal_q, applied=applied, modes=second["modes"], state=got, **{k: np.asarray(v) for k, v in acc.items()})
    print("IDEAL RESIDENT OK", flush=True)


if __name__ == "__main__":
    main()
