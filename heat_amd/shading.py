"""Shades of a series on the host (include/heat_amd.h, heat_shades): the rule the device applies to every shade at every step,
in numpy, and two conveniences that build a shade's axes and a horizon profile. No device, no library.

sunlit() IS the contract's rule, line for line — every product, sum and quotient one rounded f64 operation in the header's
order (numpy never fuses a multiply-add), min and max written as the comparisons the header gives — and so the reference of
the tests: a host that passes its result to sky.incident(..., shade=) and solar_gains.transmitted(..., shade=) and writes
their values into the solar slots between heat_batch_march_ex calls gets the bits of heat_batch_march_series_shaded.
The reference has no counterpart: solar geometry lives in another SIMPLE crate."""
import numpy as np

from .sky import SUN_X, SUN_Y, SUN_Z

TAN_22_5 = 0.41421356237309503
GEOMETRY = ("overhang_depth", "overhang_gap", "fin_pos_depth", "fin_pos_gap", "fin_neg_depth", "fin_neg_gap")


def _max(a, b):
    return np.where(b > a, b, a)      # the FIRST operand where the comparison is false: a NaN first operand stays


def _min(a, b):
    return np.where(b < a, b, a)


def sector_of(sx, sy):
    """The 22.5 degree sector of the horizon the sun stands in, counter-clockwise from east, in [0, 16) whatever sx and sy hold."""
    sx, sy = np.asarray(sx, dtype=np.float64), np.asarray(sy, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ax, ay = np.abs(sx), np.abs(sy)
        m = (ay > TAN_22_5 * ax).astype(np.int64) + (ay > ax) + (TAN_22_5 * ay > ax)
        return np.where(sx >= 0.0, np.where(sy >= 0.0, m, 15 - m), np.where(sy >= 0.0, 7 - m, 8 + m))


def sunlit(record, normal, right, up, width, height, overhang_depth=0.0, overhang_gap=0.0, fin_pos_depth=0.0, fin_pos_gap=0.0,
           fin_neg_depth=0.0, fin_neg_gap=0.0, horizon=None, horizon_tan2=None, details=False):
    """The sunlit fraction f of the beam on every shade.
    record   [..., 8]: heat_sky_record fields (sky.FIELDS) of the shade's site, broadcast against the shades
    normal, right, up   (x, y, z) each, arrays or scalars: n, u (to the right seen from outside), v (upward); u = v x n
    width, height and the six depths and gaps: m, arrays or scalars
    horizon  the shade's profile number, -1 / None: none;  horizon_tan2 [n_horizons, 16]
    Returns an array of the broadcast shape; with details=True a dict of every intermediate of the rule beside f."""
    r = np.asarray(record, dtype=np.float64)
    sx, sy, sz = r[..., SUN_X], r[..., SUN_Y], r[..., SUN_Z]
    nx, ny, nz = (np.asarray(a, dtype=np.float64) for a in normal)
    ux, uy, uz = (np.asarray(a, dtype=np.float64) for a in right)
    vx, vy, vz = (np.asarray(a, dtype=np.float64) for a in up)
    W, H = np.asarray(width, dtype=np.float64), np.asarray(height, dtype=np.float64)
    od, og, pd, pg, nd, ng = (np.asarray(a, dtype=np.float64) for a in (overhang_depth, overhang_gap, fin_pos_depth, fin_pos_gap,
                                                                         fin_neg_depth, fin_neg_gap))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = (nx * sx + ny * sy) + nz * sz
        us = (ux * sx + uy * sy) + uz * sz
        vs = (vx * sx + vy * sy) + vz * sz
        drop = (od * vs) / c
        sh = drop - og
        sh = _max(sh, 0.0)
        sh = _min(sh, H)
        fv = np.where(vs > 0.0, (H - sh) / H, 1.0)
        ap = (pd * us) / c
        wp = ap - pg
        wp = _max(wp, 0.0)
        wp = _min(wp, W)
        nu = -us
        an = (nd * nu) / c
        wn = an - ng
        wn = _max(wn, 0.0)
        wn = _min(wn, W)
        sw = np.where(us > 0.0, wp, np.where(us < 0.0, wn, 0.0))
        fh = (W - sw) / W
        f = fv * fh
        sector = sector_of(sx, sy) + np.zeros(f.shape, np.int64)
        lit = np.ones(f.shape, bool)
        if horizon is not None:
            p = np.asarray(horizon, dtype=np.int64) + np.zeros(f.shape, np.int64)
            tan2 = np.asarray(horizon_tan2 if horizon_tan2 is not None else np.zeros((0, 16)), dtype=np.float64).reshape(-1, 16)
            if (p >= 0).any():
                h2 = sx * sx + sy * sy
                z2 = sz * sz
                lit = (p < 0) | ((sz > 0.0) & (z2 > tan2[np.maximum(p, 0), sector] * h2))
                f = np.where(lit, f, 0.0)
        f = np.where(c > 0.0, f, 0.0)
    if details:
        return dict(f=f, c=c + np.zeros(f.shape), us=us + np.zeros(f.shape), vs=vs + np.zeros(f.shape), drop=drop + np.zeros(f.shape),
                    sh=sh + np.zeros(f.shape), wp=wp + np.zeros(f.shape), wn=wn + np.zeros(f.shape), sector=sector, lit=lit)
    return f


def frame_of(normal):
    """(u, v) of a plane with outward normal (x, y, z) — arrays or scalars; z up — each a tuple (x, y, z): u the in-plane
    horizontal axis, to the right seen from outside, v the in-plane upward axis, u = v x n. A wall or tilted plane has
    u = (-ny, nx, 0) / |(nx, ny)|; a horizontal plane (nx = ny = 0), which has no such axis, gets u = (1, 0, 0) for a roof and
    (-1, 0, 0) for a soffit. The normal need not be a unit vector; u and v are. A convenience — the library takes whatever
    axes the caller gives."""
    nx, ny, nz = (np.asarray(a, dtype=np.float64) for a in normal)
    length = np.sqrt(nx * nx + ny * ny + nz * nz)
    nx, ny, nz = nx / length, ny / length, nz / length
    h = np.sqrt(nx * nx + ny * ny)
    flat = h == 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        ux = np.where(flat, np.where(nz >= 0.0, 1.0, -1.0), -ny / h)
        uy = np.where(flat, 0.0, nx / h)
    uz = np.zeros(np.shape(ux))
    # v = n x u (so that u = v x n)
    vx = ny * uz - nz * uy
    vy = nz * ux - nx * uz
    vz = nx * uy - ny * ux
    return (ux, uy, uz), (vx, vy, vz)


def horizon_tan2(elevations_deg):
    """[..., 16] elevations of the obstruction in degrees (sector 0: azimuths [0, 22.5) degrees counter-clockwise from east)
    -> tan^2 of them, the table heat_shades::horizon_tan2 takes. Elevations are in [0, 90)."""
    e = np.asarray(elevations_deg, dtype=np.float64)
    if e.shape[-1] != 16:
        raise ValueError("a horizon profile has 16 sectors, not %s" % (e.shape,))
    if ((e < 0.0) | (e >= 90.0)).any():
        raise ValueError("horizon elevations are in [0, 90) degrees")
    t = np.tan(np.radians(e))
    return t * t
