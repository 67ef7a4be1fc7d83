"""Openings of a series on the host (include/heat_amd.h, heat_openings): the rule the device applies to every opening at the head
of every step, in numpy, and conveniences that give the coefficients of three published forms and join lists. No device, no
library.

apply() IS the contract's rule, line for line — every sum, product, quotient and the root one rounded f64 operation in the
header's order (numpy never fuses a multiply-add, and numpy.sqrt is correctly rounded) — and so the reference of the tests: a
host that applies it to the step's channel row before the other terms' rules, between heat_batch_march_ex calls, gets the bits
of heat_batch_march_series_openings. The reference has no counterpart (model.rs:546,592-593 take the volumes as given numbers)."""
import numpy as np

G = 9.81  # m/s2, as the reference's Rayleigh number takes it (gas.rs:82-152)
INT_KEYS = ("zone_a", "zone_b", "temp_chan", "wind_chan", "frac_chan", "out_chan")
REAL_KEYS = ("area", "cw", "cs", "ca", "c0")
KEYS = INT_KEYS + REAL_KEYS
ACC = ("sum_v", "max_v", "step_max")
_NEUTRAL = dict(temp_chan=-1, wind_chan=-1, frac_chan=-1, cw=0.0, cs=0.0, ca=0.0, c0=0.0)


def n_openings(op):
    return 0 if not op or op.get("zone_a") is None else len(np.atleast_1d(op["zone_a"]))


def _given(op, key, n):
    dtype = np.int64 if key in INT_KEYS else np.float64
    return np.full(n, _NEUTRAL[key], dtype) if op.get(key) is None else np.asarray(op[key], dtype=dtype).reshape(-1)


def fresh(op):
    """The accumulators as resume == 0 leaves them on the device: sums 0, max_v -inf, step_max -1."""
    n = n_openings(op)
    return dict(sum_v=np.zeros(n), max_v=np.full(n, -np.inf), step_max=np.full(n, -1, np.int64))


def apply(T, row, op):
    """One step of the rule. Returns (row_with_derived_columns, V): a copy of `row` with V[i] stored at out_chan[i], and V
    [n_openings], the step's row of opening_v.
    T     the zone AIR temperatures at the start of the step
    row   the step's channel row (not written)
    op    a dict of arrays: zone_a, zone_b, out_chan, area [n]; temp_chan, wind_chan, frac_chan (optional: -1), cw, cs, ca, c0
          (optional: 0)"""
    T = np.asarray(T, dtype=np.float64)
    out = np.array(row, dtype=np.float64)
    row = np.asarray(row, dtype=np.float64)
    n = n_openings(op)
    if n == 0:
        return out, np.zeros(0)
    za, zb = _given(op, "zone_a", n), _given(op, "zone_b", n)
    tc, wc, fc, oc = _given(op, "temp_chan", n), _given(op, "wind_chan", n), _given(op, "frac_chan", n), _given(op, "out_chan", n)
    area, cw, cs, ca, c0 = (_given(op, k, n) for k in REAL_KEYS)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Ta = T[za]
        Tb = np.where(zb >= 0, T[np.maximum(zb, 0)], row[np.maximum(tc, 0)] if len(row) else np.nan)
        d = Ta - Tb
        ad = np.abs(d)
        sm = Ta + Tb
        tm = sm * 0.5
        tk = tm + 273.15
        r = ad / tk
        st = cs * r
        sa = ca * ad
        u = np.where(wc >= 0, row[np.maximum(wc, 0)] if len(row) else np.nan, 0.0)
        u2 = u * u
        w = cw * u2
        x = w + st
        x2 = x + sa
        y = x2 + c0
        y = np.where(y < 0.0, 0.0, y)
        U = np.sqrt(y)
        f = np.where(fc >= 0, row[np.maximum(fc, 0)] if len(row) else np.nan, 1.0)
        f = np.where(f < 0.0, 0.0, f)
        f = np.where(f > 1.0, 1.0, f)
        af = area * f
        V = af * U
    out[oc] = V
    return out, V


def accumulate(V, acc, K):
    """The accumulators of one step, in place, from the V apply() returned; K = step_base + k."""
    with np.errstate(invalid="ignore"):
        if "sum_v" in acc:
            acc["sum_v"][:] = acc["sum_v"] + V
        if "max_v" in acc:
            higher = V > acc["max_v"]
            acc["max_v"][higher] = V[higher]
            if "step_max" in acc:
                acc["step_max"][higher] = K


def concat(*parts):
    """Joins the lists of opening dicts (as apply() takes them) into one, filling what a part leaves out with the neutral value
    (a channel -1, a coefficient 0)."""
    out = {}
    for key in KEYS:
        if key not in _NEUTRAL and all(p.get(key) is None for p in parts):
            continue  # (a list nobody has given yet: out_chan, where the caller numbers the derived channels afterwards)
        dtype = np.int32 if key in INT_KEYS else np.float64
        cols = [np.full(n_openings(p), _NEUTRAL[key], dtype) if p.get(key) is None else np.asarray(p[key], dtype=dtype).reshape(-1)
                for p in parts if n_openings(p)]
        out[key] = np.concatenate(cols) if cols else np.zeros(0, dtype)
    return out


def wind_and_stack(area, cd, cw_open, dh):
    """The coefficients of EnergyPlus' ZoneVentilation:WindandStackOpenArea (Engineering Reference, "Ventilation by Wind and
    Stack with Open Area"; ASHRAE Fundamentals 2009, ch. 16, eq. 37 and 38) in superposition form:
        Qw = cw_open A F u,   Qs = cd A F sqrt(2 g dh |Tz - To| / T),   Q = sqrt(Qw^2 + Qs^2)
           = A F sqrt(cw_open^2 u^2 + cd^2 2 g dh |dT| / T)
    area: the open area A, m2; cd: the discharge coefficient of the stack term; cw_open: the opening effectiveness (0.5 - 0.6
    perpendicular wind, 0.25 - 0.35 diagonal); dh: the height from the midpoint of the lower opening to the neutral pressure
    level, m. The rule takes T as the mean of both sides in K. Returns dict(area, cw, cs): cw = cw_open^2, cs = cd^2 2 g dh,
    applied to `area` as it is; F is the opening's frac_chan."""
    area, cd, cw_open, dh = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (area, cd, cw_open, dh)))
    return dict(area=area.copy(), cw=cw_open * cw_open, cs=cd * cd * 2.0 * G * dh)


def single_sided(area, height):
    """The coefficients of de Gids and Phaff's single-sided ventilation (W. de Gids, H. Phaff, "Ventilation rates and energy
    consumption due to open windows", Air Infiltration Review 4(1), 1982; EN 15242:2007, 6.4.2.3):
        Q = (A / 2) sqrt(0.001 u^2 + 0.0035 H |dT| + 0.01)
    area: the open area A, m2; height: the opening's height H, m; u: the meteorological wind speed, m/s. Returns
    dict(area, cw, ca, c0): area / 2, cw = 0.001, ca = 0.0035 H, c0 = 0.01."""
    area, height = np.asarray(area, dtype=np.float64), np.asarray(height, dtype=np.float64)
    one = np.ones_like(area * height)
    return dict(area=area / 2.0 * one, cw=0.001 * one, ca=0.0035 * height * one, c0=0.01 * one)


def doorway(width, height, cd):
    """The coefficients of buoyancy-driven exchange through a doorway between two rooms (W. G. Brown, K. R. Solvason, "Natural
    convection through rectangular openings in partitions — 1: vertical partitions", Int. J. Heat Mass Transfer 5, 1962):
        Q = (cd W H / 3) sqrt(g H |dT| / T)
    the volume flow EACH way, T the mean of both rooms in K. width, height: of the doorway, m; cd: the discharge coefficient
    (0.4 - 0.8). Returns dict(area, cs): area = cd W H / 3, cs = g H. One opening serves both directions: name its derived
    channel as the volume_chan of both paths of air_paths.doorway."""
    width, height, cd = (np.asarray(v, dtype=np.float64) for v in (width, height, cd))
    one = np.ones_like(width * height * cd)
    return dict(area=cd * width * height / 3.0 * one, cs=G * height * one)
