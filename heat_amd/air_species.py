"""Air species of a series on the host (include/heat_amd.h, heat_air_species): the rule the device applies to every demand vent
and to every (species, zone) at every step, in numpy, and conveniences that build and join the lists. No device, no library.

apply() IS the contract's rule, line for line — every product, quotient and sum one rounded f64 operation in the header's order
(numpy never fuses a multiply-add) — and so the reference of the tests: a host that applies it between heat_batch_march_ex calls,
behind the zone loads', the air paths' and the air handlers' rules, gets the bits of heat_batch_march_series_species.
The reference has no counterpart (zone.rs, model.rs:500-597); the air properties are its own (gas.rs:49,165-179)."""
import numpy as np

SOURCE_KEYS = ("src_zone", "src_species", "src_chan", "src_factor")
VENT_KEYS = ("vent_zone", "vent_species", "vent_temp_chan", "vent_enable_chan", "vent_v_min", "vent_v_max", "vent_c_lo", "vent_c_hi")
LANE_ACC = ("n_occupied", "sum_conc", "max_conc", "step_max", "n_above", "excess_above")
VENT_ACC = ("sum_volume", "sum_q", "steps_saturated")
ACC = LANE_ACC + VENT_ACC
INT_ACC = ("n_occupied", "step_max", "n_above", "steps_saturated")
ROWS = ("conc_rows", "vent_v", "vent_q")
_NEUTRAL = dict(src_factor=1.0, vent_enable_chan=-1)
_DTYPE = dict(src_zone=np.int32, src_species=np.int32, src_chan=np.int32, src_factor=np.float64, vent_zone=np.int32,
              vent_species=np.int32, vent_temp_chan=np.int32, vent_enable_chan=np.int32, vent_v_min=np.float64, vent_v_max=np.float64,
              vent_c_lo=np.float64, vent_c_hi=np.float64)
_FLOW_KEYS = ("zone", "volume_chan", "temp_chan", "volume_gain")


def _count(species, key):
    return 0 if not species or species.get(key) is None else len(np.atleast_1d(species[key]))


def n_species(species):
    if not species or species.get("outdoor_chan") is None or np.asarray(species["outdoor_chan"]).size == 0:
        return 0
    return int(np.atleast_2d(species["outdoor_chan"]).shape[0])


def n_sources(species):
    return _count(species, "src_zone")


def n_vents(species):
    return _count(species, "vent_zone")


def per_zone(outdoor_chan, n_zones):
    """outdoor_chan of a heat_air_species, [n_species][n_zones], from one channel per species (-1: the outside air holds none):
    every zone of the model stands in the same outside air."""
    chan = np.atleast_1d(np.asarray(outdoor_chan, dtype=np.int32))
    return np.ascontiguousarray(np.broadcast_to(chan[:, None], (len(chan), int(n_zones))))


def fresh(species, n_zones, conc=None):
    """What a run carries at its start: the concentrations (zeros, or `conc` copied) and the accumulators as resume == 0
    leaves them on the device: sums and counts 0, max_conc -inf, step_max -1."""
    S, V = n_species(species), n_vents(species)
    acc = dict(conc=np.zeros((S, n_zones)) if conc is None else np.array(conc, dtype=np.float64).reshape(S, n_zones))
    for key in LANE_ACC:
        acc[key] = np.zeros((S, n_zones), np.int64 if key in INT_ACC else np.float64)
    acc["max_conc"][:] = -np.inf
    acc["step_max"][:] = -1
    for key in VENT_ACC:
        acc[key] = np.zeros(V, np.int64 if key in INT_ACC else np.float64)
    return acc


def _given(d, key, n, default, dtype):
    return np.full(n, default, dtype) if d.get(key) is None else np.asarray(d[key], dtype=dtype).reshape(-1)


def _flows(loads):
    flows = (loads or {}).get("flows")
    if flows is None:
        return {}
    return flows if isinstance(flows, dict) else dict(zip(_FLOW_KEYS, flows))


def apply(T, C, row, a0, b0, species, vol, h, loads=None, air=None, air_state=None, handlers=None):
    """One step of the rule. Returns (a0, b0, rows); `C` ([n_species, n_zones], the concentrations) is updated in place.
    T        the zone AIR temperatures at the start of the step
    row      the step's channel row
    a0, b0   the zone terms so far (the series' own row with the loads, the paths and the handlers added), or None: zeros; copied
    species  a dict of arrays: outdoor_chan [n_species, n_zones]; SOURCE_KEYS [n_sources] (src_factor optional: 1); VENT_KEYS
             [n_vents] (vent_enable_chan optional: -1); limit_chan, occ_chan are accumulate()'s
    vol, h   the zone volumes, m3; the step's length (float(n_sub) * dt), s
    loads, air, handlers   the dicts the zone loads', the air paths' and the air handlers' rules take, or None; air_state: the
             paths' state bytes AFTER this step's air_paths.apply
    rows     conc (the concentrations at the START of the step), vent_v, vent_q [n_vents] — the step's rows — and saturated
    np.add.at adds unbuffered, in the order of its index array: per zone the caller's order."""
    T = np.asarray(T, dtype=np.float64)
    row = np.asarray(row, dtype=np.float64)
    vol = np.asarray(vol, dtype=np.float64)
    Z = len(T)
    a0 = np.zeros(Z) if a0 is None else np.array(a0, dtype=np.float64)
    b0 = np.zeros(Z) if b0 is None else np.array(b0, dtype=np.float64)
    S, NV, NQ = n_species(species), n_vents(species), n_sources(species)
    if S == 0:
        return a0, b0, dict(conc=np.zeros((0, Z)), vent_v=np.zeros(0), vent_q=np.zeros(0), saturated=np.zeros(0, bool))
    start = C.copy()
    h = float(h)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        # ---- the demand vents ----
        vz = _given(species, "vent_zone", NV, 0, np.int64)
        if NV:
            vs = _given(species, "vent_species", NV, 0, np.int64)
            ec = _given(species, "vent_enable_chan", NV, -1, np.int64)
            v_min, v_max = _given(species, "vent_v_min", NV, 0.0, np.float64), _given(species, "vent_v_max", NV, 0.0, np.float64)
            c_lo, c_hi = _given(species, "vent_c_lo", NV, 0.0, np.float64), _given(species, "vent_c_hi", NV, 0.0, np.float64)
            c = start[vs, vz]
            x = c - c_lo
            span = c_hi - c_lo
            f = x / span
            f = np.where(f < 0.0, 0.0, f)
            f = np.where(f > 1.0, 1.0, f)
            saturated = f == 1.0
            dv = v_max - v_min
            y = f * dv
            V = v_min + y
            enabled = (ec < 0) | (row[np.maximum(ec, 0)] > 0)
            V = np.where(enabled, V, 0.0)
            saturated = saturated & enabled
            t_in = row[_given(species, "vent_temp_chan", NV, 0, np.int64)]
            tk = t_in + 273.15
            rho = 101325. * 28.97 / (8314.46261815324 * tk)
            cp = 1002.7370 + 1.2324e-2 * tk
            m = (rho * V) * cp
            mt = m * t_in
            np.add.at(a0, vz[enabled], mt[enabled])
            np.add.at(b0, vz[enabled], m[enabled])
            dT = t_in - T[vz]
            q = np.where(enabled, m * dT, 0.0)
        else:
            V, q, saturated = np.zeros(0), np.zeros(0), np.zeros(0, bool)
        # ---- the concentrations ----
        oc = np.asarray(species["outdoor_chan"], dtype=np.int64).reshape(S, Z)
        co = np.where(oc >= 0, row[np.maximum(oc, 0)] if len(row) else np.nan, 0.0)
        Ssum = np.zeros((S, Z))
        if NQ:
            sz, ss = _given(species, "src_zone", NQ, 0, np.int64), _given(species, "src_species", NQ, 0, np.int64)
            x = row[_given(species, "src_chan", NQ, 0, np.int64)]
            if species.get("src_factor") is not None:
                x = np.asarray(species["src_factor"], dtype=np.float64).reshape(-1) * x
            np.add.at(Ssum, (ss, sz), x)
        # the inflows in the rule's order: the zone every one enters, its volume flow, and the zone it comes from (-1: outside)
        zone, volume, source = [], [], []
        fl = _flows(loads)
        if fl.get("zone") is not None:
            v = row[np.asarray(fl["volume_chan"], dtype=np.int64).reshape(-1)]
            if fl.get("volume_gain") is not None:
                v = np.asarray(fl["volume_gain"], dtype=np.float64).reshape(-1) * v
            zone.append(np.asarray(fl["zone"], dtype=np.int64).reshape(-1)), volume.append(v), source.append(np.full(len(v), -1))
        if air and air.get("target") is not None and len(np.atleast_1d(air["target"])):
            n = len(np.atleast_1d(air["target"]))
            ctl = _given(air, "open_chan", n, -1, np.int64) >= 0
            is_open = ~ctl | (np.asarray(air_state).reshape(-1) == 1)
            v = row[np.asarray(air["volume_chan"], dtype=np.int64).reshape(-1)]
            if air.get("volume_gain") is not None:
                v = np.asarray(air["volume_gain"], dtype=np.float64).reshape(-1) * v
            zone.append(np.asarray(air["target"], dtype=np.int64).reshape(-1)[is_open]), volume.append(v[is_open])
            source.append(np.asarray(air["source"], dtype=np.int64).reshape(-1)[is_open])
        if handlers and handlers.get("br_unit") is not None and len(np.atleast_1d(handlers["br_unit"])):
            n = len(np.atleast_1d(handlers["br_unit"]))
            supplies = (_given(handlers, "br_kind", n, 3, np.int64) & 1) == 1
            v = row[np.asarray(handlers["br_volume_chan"], dtype=np.int64).reshape(-1)]
            if handlers.get("br_volume_gain") is not None:
                v = np.asarray(handlers["br_volume_gain"], dtype=np.float64).reshape(-1) * v
            zone.append(np.asarray(handlers["br_zone"], dtype=np.int64).reshape(-1)[supplies]), volume.append(v[supplies])
            source.append(np.full(int(supplies.sum()), -1))
        zone.append(vz), volume.append(V), source.append(np.full(NV, -1))
        zone, volume, source = np.concatenate(zone), np.concatenate(volume), np.concatenate(source)
        F, G = np.zeros((S, Z)), np.zeros((S, Z))
        for s in range(S):
            ci = np.where(source >= 0, start[s, np.maximum(source, 0)], co[s, zone])
            g = volume * ci
            np.add.at(F[s], zone, volume)
            np.add.at(G[s], zone, g)
        p = Ssum + G
        hp = h * p
        vc = vol[None, :] * start
        num = vc + hp
        hF = h * F
        den = vol[None, :] + hF
        C[...] = num / den
    return a0, b0, dict(conc=start, vent_v=V, vent_q=q, saturated=saturated)


def accumulate(rows, acc, species, row, K):
    """The accumulators of one step, in place, from the rows apply() returned; K = step_base + k. acc["conc"] is not touched:
    apply() steps it."""
    row = np.asarray(row, dtype=np.float64)
    c = rows["conc"]
    S, Z = c.shape
    if S == 0:
        return
    with np.errstate(invalid="ignore"):
        occ = np.full(Z, -1, np.int64) if species.get("occ_chan") is None else np.asarray(species["occ_chan"], dtype=np.int64).reshape(-1)
        occupied = np.broadcast_to((occ < 0) | (row[np.maximum(occ, 0)] > 0), (S, Z))
        acc["n_occupied"] += occupied
        acc["sum_conc"][occupied] = acc["sum_conc"][occupied] + c[occupied]
        higher = occupied & (c > acc["max_conc"])
        acc["max_conc"][higher] = c[higher]
        acc["step_max"][higher] = K
        lim = np.full(S, -1, np.int64) if species.get("limit_chan") is None else np.asarray(species["limit_chan"], dtype=np.int64).reshape(-1)
        limit = np.broadcast_to(row[np.maximum(lim, 0)][:, None], (S, Z))
        above = occupied & (lim >= 0)[:, None] & (c > limit)
        acc["n_above"] += above
        acc["excess_above"][above] = acc["excess_above"][above] + (c - limit)[above]
    acc["sum_volume"] += rows["vent_v"]
    acc["sum_q"] += rows["vent_q"]
    acc["steps_saturated"] += rows["saturated"]


def concat(*parts):
    """Joins the source and vent lists of species dicts (as apply() takes them) into one, filling what a part leaves out with
    the neutral value; outdoor_chan, limit_chan and occ_chan are those of the first part that has them."""
    out = {}
    for key in ("outdoor_chan", "limit_chan", "occ_chan"):
        first = next((p[key] for p in parts if p.get(key) is not None), None)
        if first is not None:
            out[key] = np.asarray(first, dtype=np.int32)
    for keys, count in ((SOURCE_KEYS, n_sources), (VENT_KEYS, n_vents)):
        for key in keys:
            cols = [np.full(count(p), _NEUTRAL[key], _DTYPE[key]) if p.get(key) is None else np.asarray(p[key], dtype=_DTYPE[key]).reshape(-1)
                    for p in parts if count(p)]
            out[key] = np.concatenate(cols) if cols else np.zeros(0, _DTYPE[key])
    return out
