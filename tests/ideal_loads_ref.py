"""The CPU definition of the ideal loads of a series (include/heat_amd.h, heat_ideal_loads), for tests/test_ideal_loads_gpu.py:
per sub-timestep OracleModel.iterate_surfaces (model.rs:102-180), OracleModel.zones_abc with the step's a0 / b0
(model.rs:489-597), then the rule of the header — one rounded operation per line, math.exp — and the zone temperatures
written. The zone loads of the step (gains, flows, thermostats) come from test_zone_loads_gpu.host_rule, evaluated first.

Besides the results it returns what the test's bounds are made of, all from the reference's own values:
  scale[k, i]   S = |a| + |b| (|setpoint| + |tc|) / D, the size of the terms `need` is a difference of, as the maximum over
                the step's sub-timesteps (|a| alone where the rule does not reach the division)
  margin        the smallest |need - capacity| / S over every sub-timestep that compared the two: where it is far above
                1e-9 the saturation counts cannot depend on rounding."""
import math

import numpy as np

from test_series_gpu import term_row, write_inputs
from test_zone_loads_gpu import host_rule, n_thermostats, start_modes


def rule(a, b, cz, tc, dt, h, c, heats, cools, heat_cap, cool_cap):
    """One zone, one sub-timestep. Returns (ft, q, saturated: 0 / +1 / -1, S, |need - cap| / S or inf)."""
    q, ft, sat, margin = 0.0, tc, 0, math.inf
    S = abs(a)
    if abs(b) > 1e-9:
        r = a / b
        nbdt = (-b) * dt
        E = math.exp(nbdt / cz)
        dE = (tc - r) * E
        free = r + dE
        ft = free
        D = 1.0 - E
        if D > 0.0:
            tcE = tc * E
            sp = [x for x, on in ((h, heats), (c, cools)) if on and x == x]
            if sp:
                S = abs(a) + abs(b) * (max(abs(x) for x in sp) + abs(tc)) / D
            if heats and free < h:
                num = b * (h - tcE)
                need = num / D - a
                margin = abs(need - heat_cap) / S if math.isfinite(heat_cap) else math.inf
                q = heat_cap if need > heat_cap else need
                if not q > 0.0:
                    q = 0.0
                if q > 0.0:
                    if q == need:
                        ft = h
                    else:
                        a2 = a + q
                        r2 = a2 / b
                        d2 = (tc - r2) * E
                        ft = r2 + d2
                        sat = 1
            elif cools and free > c:
                num = b * (c - tcE)
                need = num / D - a
                margin = abs(need + cool_cap) / S if math.isfinite(cool_cap) else math.inf
                cap = -cool_cap
                q = cap if need < cap else need
                if not q < 0.0:
                    q = 0.0
                if q < 0.0:
                    if q == need:
                        ft = c
                    else:
                        a2 = a + q
                        r2 = a2 / b
                        d2 = (tc - r2) * E
                        ft = r2 + d2
                        sat = -1
    return ft, q, sat, S, margin


def caps_of(ideal, n):
    hc = ideal.get("heat_cap")
    cc = ideal.get("cool_cap")
    return (np.full(n, np.inf) if hc is None else np.asarray(hc, dtype=np.float64),
            np.full(n, np.inf) if cc is None else np.asarray(cc, dtype=np.float64))


def cpu_series(oracle, md, state, weather, n_sub, channel, drives, probes, loads, ideal, a0=None, b0=None):
    """Marches `state` in place. weather [n_steps, n_sub, 3]. Returns a dict: trace, ideal_q, n_sat_heating, n_sat_cooling,
    applied, modes, scale [n_steps, n_loads], margin, acting (sub-timesteps with q != 0), n_heat / n_cool (with q > 0 / < 0),
    q_sub [n_steps, n_sub, n_loads] (the power of every sub-timestep: ideal_q is its sum over the step)."""
    m = oracle.OracleModel(md)
    zone_slot = md["zone_slot"]
    Z, dt = int(md["n_zones"]), float(md["dt"])
    n_steps = len(channel)
    zone = np.asarray(ideal["zone"], dtype=np.int64)
    N = len(zone)
    hch = np.asarray(ideal.get("heat_chan") if ideal.get("heat_chan") is not None else np.full(N, -1), dtype=np.int64)
    cch = np.asarray(ideal.get("cool_chan") if ideal.get("cool_chan") is not None else np.full(N, -1), dtype=np.int64)
    hcap, ccap = caps_of(ideal, N)
    loads = loads or {}
    modes = start_modes(loads)
    out = dict(trace=np.zeros((n_steps, len(probes))), ideal_q=np.zeros((n_steps, N)), n_sat_heating=np.zeros(N, np.int64),
               n_sat_cooling=np.zeros(N, np.int64), applied=np.zeros((n_steps, n_thermostats(loads))), scale=np.zeros((n_steps, N)),
               margin=math.inf, n_heat=0, n_cool=0, n_free=0, q_sub=np.zeros((n_steps, n_sub, N)))
    for k in range(n_steps):
        za, zb, out["applied"][k] = host_rule(state[zone_slot], channel[k], term_row(a0, k), term_row(b0, k), loads, modes)
        write_inputs(md, state, k, channel, drives)
        for s in range(n_sub):
            t_out, wdir, wspeed = weather[k, s]
            tc = state[zone_slot].copy()
            rc, _ = m.iterate_surfaces(state, float(wdir), float(wspeed), float(t_out))
            assert rc == 0
            a, b, cz = m.zones_abc(state, za, zb)
            with np.errstate(all="ignore"):
                r = a / b
                ft = np.where(np.abs(b) > 1e-9, r + (tc - r) * np.exp(-b * dt / cz), tc)
            for i in range(N):
                z = zone[i]
                h = channel[k, hch[i]] if hch[i] >= 0 else math.nan
                c = channel[k, cch[i]] if cch[i] >= 0 else math.nan
                f, q, sat, S, margin = rule(float(a[z]), float(b[z]), float(cz[z]), float(tc[z]), dt, float(h), float(c), hch[i] >= 0,
                                            cch[i] >= 0, float(hcap[i]), float(ccap[i]))
                ft[z] = f
                out["ideal_q"][k, i] = out["ideal_q"][k, i] + q
                out["q_sub"][k, s, i] = q
                out["scale"][k, i] = max(out["scale"][k, i], S)
                out["margin"] = min(out["margin"], margin)
                out["n_sat_heating"][i] += sat > 0
                out["n_sat_cooling"][i] += sat < 0
                out["n_heat"] += q > 0
                out["n_cool"] += q < 0
                out["n_free"] += q == 0
            assert not np.isnan(ft).any()
            state[zone_slot] = ft
        out["trace"][k] = state[probes]
    out["modes"] = modes
    return out


def accumulate(ideal_q, step_base=0, start=None):
    """The accumulators of the header as a plain loop over ideal_q rows (n_sat_* excluded: they count sub-timesteps)."""
    n = ideal_q.shape[1]
    acc = start or dict(sum_heating=np.zeros(n), sum_cooling=np.zeros(n), peak_heating=np.full(n, -np.inf),
                        step_peak_heating=np.full(n, -1, np.int64), peak_cooling=np.full(n, np.inf),
                        step_peak_cooling=np.full(n, -1, np.int64))
    acc = {k: np.array(v) for k, v in acc.items()}
    for k, v in enumerate(ideal_q):
        for i in range(n):
            if v[i] > 0:
                acc["sum_heating"][i] = acc["sum_heating"][i] + v[i]
            if v[i] < 0:
                acc["sum_cooling"][i] = acc["sum_cooling"][i] + v[i]
            if v[i] > acc["peak_heating"][i]:
                acc["peak_heating"][i], acc["step_peak_heating"][i] = v[i], step_base + k
            if v[i] < acc["peak_cooling"][i]:
                acc["peak_cooling"][i], acc["step_peak_cooling"][i] = v[i], step_base + k
    return acc
