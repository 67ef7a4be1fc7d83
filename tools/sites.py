"""Weather sites (heat_batch_create_sites): what one sub-timestep costs when the headline model (1 M walls x 32 nodes,
10 000 zones) is split over 1 / 16 / 256 / 4 096 weather sites, against the same batch without sites — streamed and by
the planner's choice (cluster-resident) — and 16 separate batches of 62 500 walls against one 16-site batch of the same
walls, marched the same way (march_resident, 20 sub-timesteps per call). Then the head of a call on its own: the host's
conversion of the records (heat_batch_set_weather up to its launch) and their copy to the device (from the launch to the
end of the head's work), by the library's choice (DMA from 32 768 records) and by the head kernel alone (HEAT_AMD_WEATHER_KERNEL_COPY, in a child
process).   python tools/sites.py [S] [calls]      python tools/sites.py --weather-only [S]"""
import os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from heat_amd import HeatBatch, modeldict as mdl
WEATHER_ONLY = "--weather-only" in sys.argv
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(ARGS[0]) if len(ARGS) > 0 else 1_000_000
CALLS = int(ARGS[1]) if len(ARGS) > 1 else 10
N_SUB = 20


def weather_cost(md, st, site, n_sites, reps=30):
    """Median microseconds of heat_batch_set_weather (host: conversion, transpose, launch) and of the wait that follows
    it (device: the weather copy and the head kernel, plus one synchronisation round trip)."""
    w = mdl.weather_series(N_SUB, 45.0) if n_sites is None else mdl.weather_sites(N_SUB, 45.0, n_sites, seed=1)
    host, dev = [], []
    with HeatBatch(md, sites=site) as b:
        b.upload_state(st)
        for r in range(reps + 3):
            b.synchronize()
            t0 = time.perf_counter()
            b.set_weather(w)
            t1 = time.perf_counter()
            b.synchronize()
            t2 = time.perf_counter()
            if r >= 3:
                host.append((t1 - t0) * 1e6)
                dev.append((t2 - t1) * 1e6)
    return float(np.median(host)), float(np.median(dev))


if WEATHER_ONLY:
    md, st = mdl.uniform_massive(S, n=32, Z=max(1, S // 100), dt=45.0)
    zone = np.asarray(md["back_zone"], dtype=np.int64)
    Z = int(md["n_zones"])
    mode = "kernel copy" if os.environ.get("HEAT_AMD_WEATHER_KERNEL_COPY") else "default"
    for n_sites in (None, 16, 256, 4096):
        site = None if n_sites is None else (zone * n_sites // Z).astype(np.int32)
        h, d = weather_cost(md, st, site, n_sites)
        print("head of a call, %-11s sites %-5s (%7d records): host %7.1f us, device + sync %7.1f us" % (
            mode, "none" if n_sites is None else n_sites, N_SUB * (n_sites or 1), h, d), flush=True)
    sys.exit(0)


def per_substep(b, w, calls):
    """Wall time per sub-timestep of march_resident calls of N_SUB (two warm-up calls), and the event timing of one
    whole streamed sub-timestep (heat_batch_set_timing) when the batch streams."""
    for _ in range(2):
        b.march_resident(w)
    b.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        b.march_resident(w)
    b.synchronize()
    return (time.perf_counter() - t0) / (calls * N_SUB) * 1e6


def event_substep(b, w):
    b.set_timing(1)
    b.march_resident(w)
    b.synchronize()
    b.get_timing()  # (the first timed call: cleared)
    b.march_resident(w)
    surf_us, sub_us, n = b.get_timing()
    b.set_timing(0)
    return sub_us


md, st = mdl.uniform_massive(S, n=32, Z=max(1, S // 100), dt=45.0)
zone = np.asarray(md["back_zone"], dtype=np.int64)
Z = int(md["n_zones"])
print("%d walls x 32 nodes, %d zones, %d sub-timesteps per call" % (S, Z, N_SUB))
rows = []
for n_sites in (None, 1, 16, 256, 4096):
    site = None if n_sites is None else (zone * n_sites // Z).astype(np.int32)  # whole buildings (zone blocks) per site
    w = mdl.weather_series(N_SUB, 45.0) if n_sites is None else mdl.weather_sites(N_SUB, 45.0, n_sites, seed=1)
    res = {}
    for label, kw in (("streamed", dict(no_fusion=True)), ("planner", dict())):
        with HeatBatch(md, use_graph=True, sites=site, **kw) as b:
            b.upload_state(st)
            res[label] = per_substep(b, w, CALLS)
            res[label + "_ev"] = event_substep(b, w) if label == "streamed" else float("nan")
            res[label + "_fused"] = b.n_fused_surfaces
    rows.append((n_sites, res))
    base = rows[0][1]
    print("sites %-5s | streamed %7.1f us/sub (%+5.1f %%), events %7.1f us | planner %7.1f us/sub (%+5.1f %%), %d fused" % (
        "none" if n_sites is None else n_sites, res["streamed"], 100 * (res["streamed"] / base["streamed"] - 1),
        res["streamed_ev"], res["planner"], 100 * (res["planner"] / base["planner"] - 1), res["planner_fused"]), flush=True)

# 16 batches of S / 16 walls against one 16-site batch of the same walls (each batch's own weather)
K = 16
per = S // K
w16 = mdl.weather_sites(N_SUB, 45.0, K, seed=2)
parts = []
for k in range(K):
    m, s = mdl.uniform_massive(per, n=32, Z=max(1, per // 100), dt=45.0, seed=1000 + k)
    parts.append((m, s))
joined, site = mdl.concat([m for m, _ in parts])
jstate = np.concatenate([s for _, s in parts])
for label, kw in (("streamed", dict(no_fusion=True)), ("planner", dict())):
    batches = [HeatBatch(m, use_graph=True, **kw) for m, _ in parts]
    for b, (_, s) in zip(batches, parts):
        b.upload_state(s)
    for _ in range(2):
        for k, b in enumerate(batches):
            b.march_resident(w16[:, k, :])
    for b in batches:
        b.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        for k, b in enumerate(batches):
            b.march_resident(w16[:, k, :])
    for b in batches:
        b.synchronize()
    sep = (time.perf_counter() - t0) / (CALLS * N_SUB) * 1e6
    for b in batches:
        b.close()
    with HeatBatch(joined, use_graph=True, sites=site, **kw) as b:
        b.upload_state(jstate)
        one = per_substep(b, w16, CALLS)
    print("%d batches of %d walls, %-8s: %7.1f us/sub  | one %d-site batch: %7.1f us/sub (%.2fx)" % (
        K, per, label, sep, K, one, sep / one), flush=True)

# the head of a call on its own, with both copies (fresh child processes: the switch is read once per process)
me = [sys.executable, os.path.abspath(__file__), "--weather-only", str(S)]
for env in ({}, {"HEAT_AMD_WEATHER_KERNEL_COPY": "1"}):
    out = subprocess.run(me, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    print(out.stdout, end="", flush=True)
    if out.returncode != 0:
        print(out.stderr[-2000:])
        sys.exit(out.returncode)
