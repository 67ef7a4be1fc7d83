"""Air handlers of a series on the host (include/heat_amd.h, heat_air_handlers): the rule the device applies to every unit and
branch at every step, in numpy, and conveniences that build and join units. No device, no library.

apply() IS the contract's rule, line for line — every product, quotient and sum one rounded f64 operation in the header's order
(numpy never fuses a multiply-add) — and so the reference of the tests: a host that applies it to the zone temperatures between
heat_batch_march_ex calls, behind the zone loads' and the air paths' rules, gets the bits of heat_batch_march_series_handlers.
The reference has no counterpart (heating_cooling.rs is a todo!(), model.rs:522-544 knows scheduled flows only); the air
properties are its own (gas.rs:49,165-179)."""
import numpy as np

UNIT_KEYS = ("outdoor_chan", "eff_chan", "eff_gain", "bypass_chan", "bypass_band", "bypass_min_delta", "heat_chan", "cool_chan",
             "heat_cap", "cool_cap")
BRANCH_KEYS = ("br_unit", "br_zone", "br_volume_chan", "br_volume_gain", "br_kind")
UNIT_ACC = ("sum_recovered", "sum_heating", "sum_cooling", "steps_bypass", "switches", "steps_heat_saturated", "steps_cool_saturated")
ACC = UNIT_ACC + ("sum_branch_q",)
ROWS = ("supply_t", "recovered", "coil_q", "branch_q")
_NEUTRAL = dict(eff_chan=-1, eff_gain=1.0, bypass_chan=-1, bypass_band=0.0, bypass_min_delta=0.0, heat_chan=-1, cool_chan=-1,
                heat_cap=np.inf, cool_cap=np.inf, br_volume_gain=1.0, br_kind=3)
_DTYPE = dict(outdoor_chan=np.int32, eff_chan=np.int32, eff_gain=np.float64, bypass_chan=np.int32, bypass_band=np.float64,
              bypass_min_delta=np.float64, heat_chan=np.int32, cool_chan=np.int32, heat_cap=np.float64, cool_cap=np.float64,
              br_unit=np.int32, br_zone=np.int32, br_volume_chan=np.int32, br_volume_gain=np.float64, br_kind=np.uint8)


def n_units(handlers):
    return 0 if not handlers or handlers.get("outdoor_chan") is None else len(np.atleast_1d(handlers["outdoor_chan"]))


def n_branches(handlers):
    return 0 if not handlers or handlers.get("br_unit") is None else len(np.atleast_1d(handlers["br_unit"]))


def fresh(handlers, bypass=None):
    """What a run carries at its start: the bypass bytes (all recovering, or `bypass` copied) and the accumulators at zero."""
    U, B = n_units(handlers), n_branches(handlers)
    acc = dict(bypass=np.zeros(U, np.uint8) if bypass is None else np.array(bypass, dtype=np.uint8))
    for key in UNIT_ACC:
        acc[key] = np.zeros(U, np.float64 if key.startswith("sum_") else np.int64)
    acc["sum_branch_q"] = np.zeros(B)
    return acc


def apply(T, row, a0, b0, handlers, bypass):
    """One step of the rule. Returns (a0, b0, rows); `bypass` ([n_units] uint8, 0 recovering / 1 bypassed) is updated in place.
    T        the zone AIR temperatures at the start of the step (a unit senses air, never a control temperature)
    row      the step's channel row
    a0, b0   the zone terms so far (the series' own row with the zone loads and the air paths added), or None: zeros; copied
    handlers a dict of arrays: [n_units] outdoor_chan, eff_chan, eff_gain, bypass_chan, bypass_band, bypass_min_delta,
             heat_chan, cool_chan, heat_cap, cool_cap (all but the first optional) and [n_branches] br_unit, br_zone,
             br_volume_chan, br_volume_gain, br_kind (the last two optional: 1, 3)
    rows     supply_t, recovered, coil_q [n_units], branch_q [n_branches] — the step's rows — and, for accumulate() and the
             tests, bypass_before, bypass, extract_t, heat_active, cool_active, heat_saturated, cool_saturated
    np.add.at adds unbuffered, in the order of its index array: per unit and per zone the caller's order."""
    T = np.asarray(T, dtype=np.float64)
    row = np.asarray(row, dtype=np.float64)
    Z = len(T)
    a0 = np.zeros(Z) if a0 is None else np.array(a0, dtype=np.float64)
    b0 = np.zeros(Z) if b0 is None else np.array(b0, dtype=np.float64)
    U, B = n_units(handlers), n_branches(handlers)
    if U == 0:
        empty = np.zeros(0)
        return a0, b0, dict(supply_t=empty, recovered=empty, coil_q=empty, branch_q=empty)

    def given(key, n):
        v = handlers.get(key)
        return np.full(n, _NEUTRAL[key], _DTYPE[key]) if v is None else np.asarray(v, dtype=_DTYPE[key]).reshape(-1)

    def chan_of(key):
        c = given(key, U).astype(np.int64)
        return c >= 0, row[np.maximum(c, 0)] if len(row) else np.full(U, np.nan)

    unit = (np.asarray(handlers["br_unit"], dtype=np.int64).reshape(-1) if B else np.zeros(0, np.int64))
    zone = (np.asarray(handlers["br_zone"], dtype=np.int64).reshape(-1) if B else np.zeros(0, np.int64))
    kind = given("br_kind", B)
    ext, sup = (kind & 2) != 0, (kind & 1) != 0
    before = bypass.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        To = row[np.asarray(handlers["outdoor_chan"], dtype=np.int64).reshape(-1)]
        V = given("br_volume_gain", B) * (row[np.asarray(handlers["br_volume_chan"], dtype=np.int64).reshape(-1)] if B else np.zeros(0))
        x = V * T[zone]
        st, sv = np.zeros(U), np.zeros(U)
        np.add.at(st, unit[ext], x[ext])
        np.add.at(sv, unit[ext], V[ext])
        Te = np.divide(st, sv, out=To.copy(), where=sv > 0.0)
        eta = given("eff_gain", U).copy()
        has, value = chan_of("eff_chan")
        eta = np.where(has, eta * value, eta)
        eta = np.where(eta < 0.0, 0.0, eta)
        eta = np.where(eta > 1.0, 1.0, eta)
        ctl, setpoint = chan_of("bypass_chan")
        if ctl.any():
            d = given("bypass_band", U) / 2.0
            e = Te - setpoint
            g = Te - To
            opens = ctl & (e > d) & (g > given("bypass_min_delta", U))
            closes = ctl & ~opens & (bypass == 1) & ((e < -d) | (g <= 0.0))
            bypass[opens], bypass[closes] = 1, 0
            eta = np.where(ctl & (bypass == 1), 0.0, eta)
        dT = Te - To
        r = eta * dT
        Tr = To + r
        Tk = Tr + 273.15
        rho = 101325. * 28.97 / (8314.46261815324 * Tk)
        cp = 1002.7370 + 1.2324e-2 * Tk
        m = np.where(sup, (rho[unit] * V) * cp[unit], 0.0)
        M = np.zeros(U)
        np.add.at(M, unit[sup], m[sup])
        recovered = M * r
        has_heat, heat_set = chan_of("heat_chan")
        has_cool, cool_set = chan_of("cool_chan")
        heat_cap, cool_cap = given("heat_cap", U), given("cool_cap", U)
        heat = has_heat & (Tr < heat_set)
        cool = ~heat & has_cool & (Tr > cool_set)
        need_h = M * (heat_set - Tr)
        need_c = M * (Tr - cool_set)
        heat_ok, cool_ok = heat & (need_h <= heat_cap), cool & (need_c <= cool_cap)
        heat_sat, cool_sat = heat & ~heat_ok, cool & ~cool_ok
        Ts = np.where(heat_ok, heat_set, np.where(heat_sat, Tr + heat_cap / M, np.where(cool_ok, cool_set, np.where(cool_sat, Tr - cool_cap / M, Tr))))
        q = np.where(heat_ok, need_h, np.where(heat_sat, heat_cap, np.where(cool_ok, 0.0 - need_c, np.where(cool_sat, 0.0 - cool_cap, 0.0))))
        mt = m * Ts[unit]
        np.add.at(a0, zone[sup], mt[sup])
        np.add.at(b0, zone[sup], m[sup])
        dz = Ts[unit] - T[zone]
        bq = np.where(sup, m * dz, 0.0)
    return a0, b0, dict(supply_t=Ts, recovered=recovered, coil_q=q, branch_q=bq, bypass_before=before, bypass=bypass.copy(), extract_t=Te,
                        heat_active=heat, cool_active=cool, heat_saturated=heat_sat, cool_saturated=cool_sat)


def accumulate(rows, acc):
    """The accumulators of one step, in place (acc: a dict as fresh() gives; a key that is absent is not maintained)."""
    if len(rows["supply_t"]) == 0:
        return
    q = rows["coil_q"]
    with np.errstate(invalid="ignore", over="ignore"):
        for key, add in (("sum_recovered", rows["recovered"]), ("sum_heating", np.where(q > 0.0, q, 0.0)), ("sum_cooling", np.where(q < 0.0, q, 0.0))):
            if key in acc:
                # (the device adds only where the condition holds: x + 0.0 is x but for x = -0.0, which no sum of these reaches)
                acc[key] += add
        if "sum_branch_q" in acc:
            acc["sum_branch_q"] += rows["branch_q"]
    for key, add in (("steps_bypass", rows["bypass"]), ("switches", rows["bypass"] != rows["bypass_before"]),
                     ("steps_heat_saturated", rows["heat_saturated"]), ("steps_cool_saturated", rows["cool_saturated"])):
        if key in acc:
            acc[key] += add.astype(np.int64)


def concat(*parts):
    """Joins handler dicts (as apply() takes them) into one: the units and the branches one after the other, br_unit moved to
    the units' new numbers, what a part leaves out filled with the neutral value."""
    out = {}
    for key in UNIT_KEYS:
        cols = [np.full(n_units(p), _NEUTRAL[key], _DTYPE[key]) if p.get(key) is None else np.asarray(p[key], dtype=_DTYPE[key]).reshape(-1)
                for p in parts]
        out[key] = np.concatenate(cols) if cols else np.zeros(0, _DTYPE[key])
    base = np.concatenate([[0], np.cumsum([n_units(p) for p in parts])]).astype(np.int64)
    for key in BRANCH_KEYS:
        cols = []
        for i, p in enumerate(parts):
            if p.get(key) is None:
                col = np.full(n_branches(p), _NEUTRAL[key], _DTYPE[key]) if key in _NEUTRAL else np.zeros(0, _DTYPE[key])
            else:
                col = np.asarray(p[key], dtype=_DTYPE[key]).reshape(-1)
            cols.append(col + base[i] if key == "br_unit" else col)
        out[key] = (np.concatenate(cols) if cols else np.zeros(0)).astype(_DTYPE[key])
    return out


def balanced(zones, volume_chan, outdoor_chan, volume_gain=None, eff_gain=None, eff_chan=None, bypass_chan=None, bypass_band=0.0,
             bypass_min_delta=0.0, heat_chan=None, cool_chan=None, heat_cap=None, cool_cap=None):
    """ONE unit that supplies and extracts the same zones at the same volume flows (every branch of kind 3): a dict of apply()'s
    and make_air_handlers' arguments. zones: the zones; volume_chan (and volume_gain): a scalar or one per zone. A convenience,
    not part of the contract."""
    z = np.atleast_1d(np.asarray(zones, dtype=np.int32))
    out = dict(outdoor_chan=np.array([outdoor_chan], np.int32), br_unit=np.zeros(len(z), np.int32), br_zone=z,
               br_volume_chan=np.broadcast_to(np.asarray(volume_chan, dtype=np.int32), z.shape).copy(), br_kind=np.full(len(z), 3, np.uint8))
    if volume_gain is not None:
        out["br_volume_gain"] = np.broadcast_to(np.asarray(volume_gain, dtype=np.float64), z.shape).copy()
    for key, v in (("eff_gain", eff_gain), ("eff_chan", eff_chan), ("heat_chan", heat_chan), ("cool_chan", cool_chan), ("heat_cap", heat_cap),
                   ("cool_cap", cool_cap)):
        if v is not None:
            out[key] = np.array([v], _DTYPE[key])
    if bypass_chan is not None:
        out.update(bypass_chan=np.array([bypass_chan], np.int32), bypass_band=np.array([bypass_band], np.float64),
                   bypass_min_delta=np.array([bypass_min_delta], np.float64))
    return out
