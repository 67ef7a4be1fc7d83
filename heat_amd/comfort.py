"""Comfort of a series on the host (include/heat_amd.h, heat_comfort): the rule the device applies to every sensor at every
step, in numpy, and a convenience that builds one sensor per zone from the model's areas. No device, no library.

operative(), control_temperatures() and accumulate() ARE the contract's rule, line for line — every product and sum one
rounded f64 operation in the header's order (numpy never fuses a multiply-add) — and so the reference of the tests: a host that
applies them to the state it downloads between heat_batch_march_ex calls, and hands the control temperatures to the thermostat
rule, to air_paths.apply(control_T=) and to blinds.apply in place of the zone temperatures, gets the bits of
heat_batch_march_series_comfort. The reference has no comfort model."""
import numpy as np

SPACE = 0   # modeldict.SPACE: a side that faces a zone
ACC = ("n_occupied", "sum_operative", "min_operative", "step_min", "max_operative", "step_max", "n_below", "deg_below", "n_above",
       "deg_above", "max_above", "step_max_above")
_INT = ("n_occupied", "step_min", "step_max", "n_below", "n_above", "step_max_above")
_START = dict(n_occupied=0, sum_operative=0.0, min_operative=np.inf, step_min=-1, max_operative=-np.inf, step_max=-1, n_below=0,
              deg_below=0.0, n_above=0, deg_above=0.0, max_above=-np.inf, step_max_above=-1)


def n_sensors(sensors):
    return 0 if not sensors or sensors.get("zone") is None else len(np.atleast_1d(sensors["zone"]))


def n_entries(sensors):
    return 0 if not sensors or sensors.get("en_sensor") is None else len(np.atleast_1d(sensors["en_sensor"]))


def fresh(n, keys=ACC):
    """The accumulators of n sensors as the library starts them with resume == 0: sums and counts 0, min = +inf, max = -inf,
    max_above = -inf, steps = -1."""
    return {k: np.full(n, _START[k], np.int64 if k in _INT else np.float64) for k in keys}


def face_slots(md, sensors):
    """The state slot of every entry's face node, [n_entries]: the first node of the surface (en_side 0) or its last
    (en_side 1). T_face of operative() is state[face_slots(md, sensors)]."""
    if n_entries(sensors) == 0:
        return np.zeros(0, np.int64)
    q = np.asarray(sensors["en_surface"], dtype=np.int64).reshape(-1)
    side = np.asarray(sensors["en_side"], dtype=np.int64).reshape(-1)
    first = np.asarray(md["first_node_slot"], dtype=np.int64)
    n = np.diff(np.asarray(md["node_offset"], dtype=np.int64))
    return first[q] + np.where(side > 0, n[q] - 1, 0)


def _given(sensors, key, default, dtype):
    n = n_sensors(sensors)
    return np.full(n, default, dtype) if sensors.get(key) is None else np.asarray(sensors[key], dtype=dtype).reshape(-1)


def _closest(margin, key, distances):
    v = distances[~np.isnan(distances)]
    if len(v):
        margin[key] = min(margin.get(key, np.inf), float(v.min()))


def operative(T_face, T_zone, sensors):
    """The mean radiant and the operative temperature of every sensor. Returns (mrt, top), [n_sensors] each.
    T_face   [n_entries] the temperature of every entry's face node at the start of the step, in the caller's entry order
    T_zone   the zone temperatures at the start of the step
    sensors  a dict of arrays: zone [n_sensors], air_weight (optional: 0.5), control (optional: 0), en_sensor, en_surface,
             en_side, en_weight [n_entries], occ_chan, lo_chan, hi_chan (optional / -1: always occupied / no limit)
    np.add.at adds unbuffered, in the order of its index array: per sensor the caller's order, from r = 0.0."""
    n = n_sensors(sensors)
    T_zone = np.asarray(T_zone, dtype=np.float64).reshape(-1)
    r = np.zeros(n)
    with np.errstate(invalid="ignore", over="ignore"):
        if n_entries(sensors):
            x = np.asarray(sensors["en_weight"], dtype=np.float64).reshape(-1) * np.asarray(T_face, dtype=np.float64).reshape(-1)
            np.add.at(r, np.asarray(sensors["en_sensor"], dtype=np.int64).reshape(-1), x)
        a = _given(sensors, "air_weight", 0.5, np.float64)
        xa = a * T_zone[np.asarray(sensors["zone"], dtype=np.int64).reshape(-1)] if n else np.zeros(0)
        b = 1.0 - a
        xr = b * r
        top = xa + xr
    return r, top


def control_temperatures(T_zone, top, sensors):
    """Tc [n_zones]: the operative temperature of the zone's control sensor (control == 1), else the zone temperature."""
    Tc = np.array(T_zone, dtype=np.float64).reshape(-1)
    if n_sensors(sensors):
        ctl = _given(sensors, "control", 0, np.uint8) == 1
        Tc[np.asarray(sensors["zone"], dtype=np.int64).reshape(-1)[ctl]] = np.asarray(top, dtype=np.float64)[ctl]
    return Tc


def accumulate(top, row, sensors, acc, K, margin=None):
    """The statistics of one step, in place, on the accumulators `acc` holds (a dict with any of ACC; fresh() starts them).
    top     [n_sensors] operative() of the step;  row: the step's channel row;  K: step_base + k
    margin  None, or a dict whose "limit" becomes the smallest |top - limit| over the comparisons with a limit made so far,
            and "extremum" the smallest distance of a value from the extremum it was compared with (how far the counts and
            the steps are from depending on rounding)
    Returns (occupied, below, above), [n_sensors] bool each."""
    n = n_sensors(sensors)
    top = np.asarray(top, dtype=np.float64).reshape(-1)
    row = np.asarray(row, dtype=np.float64).reshape(-1)
    row = row if len(row) else np.full(1, np.nan)          # (nothing reads it then: a value to index)
    oc, lc, hc = (_given(sensors, k, -1, np.int64) for k in ("occ_chan", "lo_chan", "hi_chan"))
    has = lambda k: acc.get(k) is not None
    with np.errstate(invalid="ignore", over="ignore"):
        occ = (oc < 0) | (row[np.maximum(oc, 0)] > 0.0)
        if has("n_occupied"):
            acc["n_occupied"] += occ.astype(np.int64)
        if has("sum_operative"):
            acc["sum_operative"][occ] = acc["sum_operative"][occ] + top[occ]
        for ext, step, better in (("min_operative", "step_min", np.less), ("max_operative", "step_max", np.greater)):
            if has(ext):
                if margin is not None:
                    _closest(margin, "extremum", np.abs(top - acc[ext])[occ])
                m = occ & better(top, acc[ext])
                acc[ext][m] = top[m]
                if has(step):
                    acc[step][m] = K
        lo, hi = row[np.maximum(lc, 0)], row[np.maximum(hc, 0)]
        below = occ & (lc >= 0) & (top < lo)
        above = occ & (hc >= 0) & (top > hi)
        if has("n_below"):
            acc["n_below"] += below.astype(np.int64)
        d = lo - top
        if has("deg_below"):
            acc["deg_below"][below] = acc["deg_below"][below] + d[below]
        if has("n_above"):
            acc["n_above"] += above.astype(np.int64)
        d = top - hi
        if has("deg_above"):
            acc["deg_above"][above] = acc["deg_above"][above] + d[above]
        if has("max_above"):
            if margin is not None:
                _closest(margin, "extremum", np.abs(d - acc["max_above"])[above])
            m = above & (d > acc["max_above"])
            acc["max_above"][m] = d[m]
            if has("step_max_above"):
                acc["step_max_above"][m] = K
        if margin is not None:
            _closest(margin, "limit", np.abs(top - lo)[occ & (lc >= 0)])
            _closest(margin, "limit", np.abs(top - hi)[occ & (hc >= 0)])
    assert len(occ) == n
    return occ, below, above


def by_area(md, air_weight=0.5, weight=None, control=False):
    """One sensor per zone over the sides that face that zone: a dict of operative()'s and make_comfort's arguments.
    An entry's weight is w A / sum(w A) over its sensor, A the surface's area and w `weight` ([n_surfaces], or a pair of them
    for the front and the back side; None: 1 — an emissivity, say). A zone no side faces gets a sensor without entries
    (its mean radiant temperature is 0.0: give such a zone air_weight 1). Sensor z stands in zone z; control: every sensor
    is its zone's control temperature. A convenience, not part of the contract."""
    S, Z = int(md["n_surfaces"]), int(md["n_zones"])
    area = np.asarray(md["area"], dtype=np.float64)
    if weight is None:
        w = (np.ones(S), np.ones(S))
    elif isinstance(weight, tuple):
        w = tuple(np.broadcast_to(np.asarray(v, dtype=np.float64), (S,)) for v in weight)
    else:
        w = (np.broadcast_to(np.asarray(weight, dtype=np.float64), (S,)),) * 2
    surf, side, zone, wa = [], [], [], []
    for s_, (kind, zkey) in enumerate((("front_kind", "front_zone"), ("back_kind", "back_zone"))):
        on = np.flatnonzero(np.asarray(md[kind]) == SPACE)
        surf.append(on), side.append(np.full(len(on), s_, np.uint8)), zone.append(np.asarray(md[zkey], dtype=np.int64)[on])
        wa.append(w[s_][on] * area[on])
    surf, side, zone, wa = (np.concatenate(v) for v in (surf, side, zone, wa))
    order = np.argsort(surf, kind="stable")                # a surface's front before its back, surfaces in the model's order
    surf, side, zone, wa = surf[order], side[order], zone[order], wa[order]
    total = np.zeros(Z)
    np.add.at(total, zone, wa)
    return dict(zone=np.arange(Z, dtype=np.int32), air_weight=np.broadcast_to(np.asarray(air_weight, dtype=np.float64), (Z,)).copy(),
                control=np.full(Z, 1 if control else 0, np.uint8), en_sensor=zone.astype(np.int32), en_surface=surf.astype(np.int64),
                en_side=side.astype(np.uint8), en_weight=wa / total[zone])
