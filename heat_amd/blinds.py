"""Blinds of a series on the host (include/heat_amd.h, heat_blinds): the rule the device applies to every blind at every step,
in numpy. No device, no library.

incident_on() and apply() ARE the contract's rule, line for line — every product and sum one rounded f64 operation in the
header's order (numpy never fuses a multiply-add), min and max written as the comparisons the header gives — and so the
reference of the tests: a host that downloads the zone temperatures between heat_batch_march_ex calls, applies the rule and
passes the effective factors to sky.incident(..., shade=) and solar_gains.transmitted(..., shade=) gets the bits of
heat_batch_march_series_blinds.
The reference has no counterpart: it has no solar geometry at all, let alone one that moves."""
import numpy as np

from .sky import SUN_X, SUN_Y, SUN_Z, BEAM, DIFFUSE, GROUND, circumsolar_ratio

KEYS = ("shade", "beam_closed", "diffuse_closed", "ground_closed", "pos_chan", "irr_close", "irr_open", "zone", "set_chan", "band",
        "enable_chan")


def _max(a, b):
    return np.where(b > a, b, a)      # the FIRST operand where the comparison is false: a NaN first operand stays


def _min(a, b):
    return np.where(b < a, b, a)


def n_blinds(blinds):
    return 0 if not blinds or blinds.get("shade") is None else len(np.atleast_1d(blinds["shade"]))


def shade_factors(shades):
    """(fd, fg) of every shade: its constant diffuse and ground factor, ones where the shades give none."""
    n = len(np.asarray(shades["surface"]).reshape(-1))
    fd = np.ones(n) if shades.get("diffuse_factor") is None else np.asarray(shades["diffuse_factor"], dtype=np.float64).reshape(-1)
    fg = np.ones(n) if shades.get("ground_factor") is None else np.asarray(shades["ground_factor"], dtype=np.float64).reshape(-1)
    return fd, fg


def incident_on(shades, record, sunlit, site=None, aniso=None):
    """I: what an unblinded sky-driven side in every shade's plane receives, W/m2.
    shades  a dict of binding.make_shades' arguments (surface, normal, diffuse_factor, ground_factor are read)
    record  [n_sites, 8] the step's records, or [n_steps, n_sites, 8]
    sunlit  [n_shades] the step's geometric sunlit fractions (shading.sunlit), or [n_steps, n_shades]
    site    [n_surfaces] the site of every surface; None: one site
    aniso   None, or (circ, horiz, band) of heat_sky_aniso: circ and horiz [n_sites] the step's pairs, or [n_steps, n_sites],
            as the records; band [n_shades] (shade_band)
    Returns [n_shades], or [n_steps, n_shades]. A shade reads the record of ITS surface's site."""
    r = np.asarray(record, dtype=np.float64)
    f = np.asarray(sunlit, dtype=np.float64)
    surface = np.asarray(shades["surface"], dtype=np.int64).reshape(-1)
    at = np.zeros(len(surface), np.int64) if site is None else np.asarray(site, dtype=np.int64)[surface]
    r = r[..., at, :]
    nx, ny, nz = (np.asarray(a, dtype=np.float64) for a in shades["normal"])
    fd, fg = shade_factors(shades)
    with np.errstate(invalid="ignore", over="ignore"):
        c = (nx * r[..., SUN_X] + ny * r[..., SUN_Y]) + nz * r[..., SUN_Z]
        fs = 0.5 + 0.5 * nz
        fg_ = 0.5 - 0.5 * nz
        bm = np.where(c > 0.0, r[..., BEAM] * c, 0.0)
        if aniso is not None:
            circ = np.asarray(aniso[0], dtype=np.float64)[..., at]
            horiz = np.asarray(aniso[1], dtype=np.float64)[..., at]
            band = np.asarray(aniso[2], dtype=np.float64)
            rb = circumsolar_ratio(c, r[..., SUN_Z])
            iso = 1.0 - circ
            cs = (r[..., DIFFUSE] * circ) * rb
            sun = bm + cs
            dv = (r[..., DIFFUSE] * fs) * iso
            hv = (r[..., DIFFUSE] * horiz) * band
            dv = dv + hv
            gv = r[..., GROUND] * fg_
            sun = sun * f
            dv = dv * fd
            gv = gv * fg
            return (sun + dv) + gv
        bm = bm * f
        dv = (r[..., DIFFUSE] * fs) * fd
        gv = (r[..., GROUND] * fg_) * fg
        return (bm + dv) + gv


def apply(I, T, row, blinds, state, sunlit, shades, margin=None):
    """One step of the rule. Returns (position [n_blinds], f' [n_shades], fd' [n_shades], fg' [n_shades]); `state` ([n_blinds]
    uint8, 0 open / 1 closed) is updated in place — the bytes of scheduled blinds are left alone.
    I       [n_shades] incident_on() of the step
    T       the zone temperatures at the start of the step
    row     the step's channel row
    blinds  a dict of arrays, [n_blinds] each: shade, beam_closed, diffuse_closed, ground_closed, pos_chan (optional / -1:
            controlled), irr_close, irr_open (read where controlled), zone (optional / -1: no room condition), set_chan, band
            (read where zone >= 0), enable_chan (optional / -1: always enabled)
    sunlit  [n_shades] the step's geometric sunlit fractions;  shades: the dict incident_on() takes (for fd, fg)
    margin  None, or a dict whose "I" and "T" become the smallest |I - threshold| and |T - (set +- d)| over the comparisons
            made so far (how far the decisions are from depending on rounding)
    The three factors feed sky.incident(..., shade=) and solar_gains.transmitted(..., shade=) as they are: index them with the
    consumers' shade numbers. A shade without a blind keeps (f, fd, fg)."""
    f = np.asarray(sunlit, dtype=np.float64)
    fd, fg = shade_factors(shades)
    n = n_blinds(blinds)
    if n == 0:
        return np.zeros(0), f.copy(), fd.copy(), fg.copy()
    I = np.asarray(I, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    row = np.asarray(row, dtype=np.float64).reshape(-1)
    T = T if len(T) else np.full(1, np.nan)             # (nothing reads them then: a value to index)
    row = row if len(row) else np.full(1, np.nan)
    j = np.asarray(blinds["shade"], dtype=np.int64).reshape(-1)

    def given(key, default, dtype):
        return np.full(n, default, dtype) if blinds.get(key) is None else np.asarray(blinds[key], dtype=dtype).reshape(-1)

    pos_chan, zone, enable_chan = given("pos_chan", -1, np.int64), given("zone", -1, np.int64), given("enable_chan", -1, np.int64)
    Ib = I[j]
    with np.errstate(invalid="ignore", over="ignore"):
        scheduled = pos_chan >= 0
        p = row[np.maximum(pos_chan, 0)]
        p = _max(p, 0.0)
        p = _min(p, 1.0)
        ctl = ~scheduled
        if ctl.any():
            irr_close, irr_open = given("irr_close", 0.0, np.float64), given("irr_open", 0.0, np.float64)
            enabled = (enable_chan < 0) | (row[np.maximum(enable_chan, 0)] > 0.0)
            gated = ctl & (zone >= 0)
            tz = T[np.maximum(zone, 0)]
            setpoint = row[np.maximum(given("set_chan", -1, np.int64), 0)]
            d = given("band", 0.0, np.float64) / 2.0
            hi = setpoint + d
            lo = setpoint - d
            hot = ~gated | (tz > hi)
            cool = gated & (tz < lo)
            off = ctl & ~enabled
            closes = ctl & enabled & (Ib > irr_close) & hot
            was_closed = state == 1
            opens = ctl & enabled & ~closes & was_closed & ((Ib < irr_open) | cool)
            if margin is not None:
                live = ctl & enabled
                m_i = [np.abs(Ib - irr_close)[live], np.abs(Ib - irr_open)[live & ~closes & was_closed]]
                m_t = [np.abs(tz - hi)[live & gated], np.abs(tz - lo)[live & gated & ~closes & was_closed]]
                for key, parts in (("I", m_i), ("T", m_t)):
                    for v in parts:
                        v = v[~np.isnan(v)]
                        if len(v):
                            margin[key] = min(margin.get(key, np.inf), float(v.min()))
            state[off], state[closes], state[opens] = 0, 1, 0
        p = np.where(scheduled, p, state.astype(np.float64))
        q = 1.0 - p
        kb = q + p * np.asarray(blinds["beam_closed"], dtype=np.float64).reshape(-1)
        kd = q + p * np.asarray(blinds["diffuse_closed"], dtype=np.float64).reshape(-1)
        kg = q + p * np.asarray(blinds["ground_closed"], dtype=np.float64).reshape(-1)
        f2, fd2, fg2 = f.copy(), fd.copy(), fg.copy()
        f2[j] = f[j] * kb
        fd2[j] = fd[j] * kd
        fg2[j] = fg[j] * kg
    return p, f2, fd2, fg2


def accumulate(p, state, before, sum_position, steps_closed, switches):
    """The accumulators of one step, in place: sum_position += p; steps_closed += (p > 0); switches += (state != before)."""
    with np.errstate(invalid="ignore"):
        sum_position += p
        steps_closed += (p > 0.0).astype(np.int64)
    switches += (state != before).astype(np.int64)
