"""Air paths of a series on the host (include/heat_amd.h, heat_air_paths): the rule the device applies to every path at every
step, in numpy, and a convenience that builds the two paths of a doorway. No device, no library.

apply() IS the contract's rule, line for line — every product and sum one rounded f64 operation in the header's order (numpy
never fuses a multiply-add) — and so the reference of the tests: a host that applies it to the zone temperatures between
heat_batch_march_ex calls, behind the zone loads' rule, gets the bits of heat_batch_march_series_air.
The reference has no counterpart: it marks the mixing of air between zones and leaves it unimplemented (model.rs:546,592-593)."""
import numpy as np

KEYS = ("target", "source", "temp_chan", "volume_chan", "volume_gain", "open_chan", "sense", "band", "min_delta")


def n_paths(air):
    return 0 if not air or air.get("target") is None else len(np.atleast_1d(air["target"]))


def apply(T, row, a0, b0, air, state, control_T=None):
    """One step of the rule. Returns (a0, b0, q); `state` ([n_paths] uint8, 0 closed / 1 open) is updated in place.
    T      the zone temperatures at the start of the step
    row    the step's channel row
    a0, b0 the zone terms so far (the series' own row with the zone loads added), or None: zeros; they are copied
    air    a dict of arrays, [n_paths] each: target, source (-1: supply air at row[temp_chan]), temp_chan (optional without
           a source of -1), volume_chan, volume_gain (optional: 1), open_chan (optional / -1: uncontrolled, always open),
           sense (+1 cooling / -1 heating), band, min_delta (the three read only where controlled)
    control_T  what a controlled path senses for e = s * (control_T[target] - set): None is T itself (today's rule); with a
           comfort term the step's control temperatures (comfort.control_temperatures). g, dT and q keep T: the air that
           moves is air.
    np.add.at adds unbuffered, in the order of its index array: per target zone the caller's order; closed paths add nothing.
    open = state == 1 for a controlled path after the call; an uncontrolled path is open and its state byte is left alone."""
    T = np.asarray(T, dtype=np.float64)
    row = np.asarray(row, dtype=np.float64)
    Z = len(T)
    a0 = np.zeros(Z) if a0 is None else np.array(a0, dtype=np.float64)
    b0 = np.zeros(Z) if b0 is None else np.array(b0, dtype=np.float64)
    n = n_paths(air)
    if n == 0:
        return a0, b0, np.zeros(0)
    target = np.asarray(air["target"], dtype=np.int64).reshape(-1)
    source = np.asarray(air["source"], dtype=np.int64).reshape(-1)

    def given(key, default, dtype):
        return np.full(n, default, dtype) if air.get(key) is None else np.asarray(air[key], dtype=dtype).reshape(-1)

    temp_chan, open_chan = given("temp_chan", -1, np.int64), given("open_chan", -1, np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tt = T[target]
        tc = tt if control_T is None else np.asarray(control_T, dtype=np.float64)[target]
        ts = np.where(source >= 0, T[np.maximum(source, 0)], row[np.maximum(temp_chan, 0)] if len(row) else np.nan)
        ctl = open_chan >= 0
        if ctl.any():
            s = given("sense", 1, np.float64)
            d = given("band", 0.0, np.float64) / 2.0
            min_delta = given("min_delta", 0.0, np.float64)
            setpoint = row[np.maximum(open_chan, 0)]
            e = s * (tc - setpoint)
            g = s * (tt - ts)
            opens = ctl & (e > d) & (g > min_delta)
            closes = ctl & ~opens & (state == 1) & ((e < -d) | (g <= 0.0))
            state[opens], state[closes] = 1, 0
        is_open = ~ctl | (state == 1)
        v = row[np.asarray(air["volume_chan"], dtype=np.int64).reshape(-1)]
        if air.get("volume_gain") is not None:
            v = np.asarray(air["volume_gain"], dtype=np.float64).reshape(-1) * v
        tk = ts + 273.15
        rho = 101325. * 28.97 / (8314.46261815324 * tk)
        cp = 1002.7370 + 1.2324e-2 * tk
        m = (rho * v) * cp
        mt = m * ts
        np.add.at(a0, target[is_open], mt[is_open])
        np.add.at(b0, target[is_open], m[is_open])
        dt = ts - tt
        q = np.where(is_open, m * dt, 0.0)
    return a0, b0, q


def accumulate(q, state, before, air, sum_q, steps_open, switches):
    """The accumulators of one step, in place: sum_q += q; steps_open += open; switches += (state != before)."""
    open_chan = air.get("open_chan")
    ctl = np.zeros(len(q), bool) if open_chan is None else np.asarray(open_chan).reshape(-1) >= 0
    sum_q += q
    steps_open += (~ctl | (state == 1)).astype(np.int64)
    switches += (state != before).astype(np.int64)


def doorway(zone_a, zone_b, volume_chan, volume_gain=None):
    """The two uncontrolled paths of a balanced exchange between two zones (a -> b and b -> a at the same volume flow): a
    dict of apply()'s and make_air_paths' arguments. zone_a, zone_b, volume_chan (and volume_gain) are scalars or equally
    long arrays; the paths of doorway j are j and n + j. A convenience, not part of the contract."""
    a = np.atleast_1d(np.asarray(zone_a, dtype=np.int32))
    b = np.atleast_1d(np.asarray(zone_b, dtype=np.int32))
    chan = np.broadcast_to(np.asarray(volume_chan, dtype=np.int32), a.shape)
    out = dict(target=np.concatenate([b, a]), source=np.concatenate([a, b]), volume_chan=np.concatenate([chan, chan]))
    if volume_gain is not None:
        gain = np.broadcast_to(np.asarray(volume_gain, dtype=np.float64), a.shape)
        out["volume_gain"] = np.concatenate([gain, gain])
    return out


def concat(*parts):
    """Joins path lists (dicts as apply() takes them) into one, filling what a part leaves out with the neutral value."""
    neutral = dict(temp_chan=-1, volume_gain=1.0, open_chan=-1, sense=1, band=0.0, min_delta=0.0)
    dtype = dict(target=np.int32, source=np.int32, temp_chan=np.int32, volume_chan=np.int32, volume_gain=np.float64,
                 open_chan=np.int32, sense=np.int8, band=np.float64, min_delta=np.float64)
    out = {}
    for key in KEYS:
        cols = []
        for p in parts:
            n = n_paths(p)
            cols.append(np.full(n, neutral[key], dtype[key]) if p.get(key) is None else np.asarray(p[key], dtype=dtype[key]).reshape(-1))
        out[key] = np.concatenate(cols) if cols else np.zeros(0, dtype[key])
    return out
