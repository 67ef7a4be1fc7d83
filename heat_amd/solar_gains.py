"""Solar gains of a series on the host (include/heat_amd.h, heat_solar_gains): the rule the device applies to every aperture
and every receiver at every step, in numpy, and a convenience that builds the entry list of the common case. No device, no
library.

transmitted() and received() ARE the contract's rule, line for line — every product and sum one rounded f64 operation in the
header's order (numpy never fuses a multiply-add) — and so the reference of the tests: a host that writes received()'s values
into the solar slots between heat_batch_march_ex calls gets the bits of heat_batch_march_series_gains.
The reference has no counterpart: window-transmitted solar is computed in another SIMPLE crate."""
import numpy as np

from . import modeldict as mdl
from .sky import SUN_X, SUN_Y, SUN_Z, BEAM, DIFFUSE, GROUND, circumsolar_ratio


def transmitted(record, normal, coef, tau_diffuse, scale, shade=None, aniso=None):
    """The power (W) every aperture transmits: (Pb, Pd), beam and diffuse + ground-reflected.
    record       [..., 8]: heat_sky_record fields (sky.FIELDS) of the aperture's site, broadcast against the apertures
    normal       (x, y, z) of the outward normal of the side that sees the sky, arrays or scalars
    coef         [..., 6]: the beam transmittance as a polynomial in the cosine of incidence, constant term first
    tau_diffuse  the hemispherical transmittance
    scale        area x frame or shading factor, m2
    shade        None, or (f, fd, fg) of shaded apertures (heat_shades): the step's sunlit fraction from shading.sunlit and
                 the shade's diffuse and ground factor, broadcast like the apertures
    aniso        None, or (circ, horiz, band) of heat_sky_aniso: the coefficient pair of the record's site at the step and the
                 band of the aperture, broadcast like the apertures
    Returns two arrays of the broadcast shape; P = Pb + Pd is what transmitted[k][a] and ap_sum take."""
    r = np.asarray(record, dtype=np.float64)
    nx, ny, nz = (np.asarray(a, dtype=np.float64) for a in normal)
    coef = np.asarray(coef, dtype=np.float64)
    tau_diffuse = np.asarray(tau_diffuse, dtype=np.float64)
    scale = np.asarray(scale, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        c = (nx * r[..., SUN_X] + ny * r[..., SUN_Y]) + nz * r[..., SUN_Z]
        fs = 0.5 + 0.5 * nz
        fg = 0.5 - 0.5 * nz
        t = coef[..., 5]
        for j in range(4, -1, -1):
            t = t * c
            t = t + coef[..., j]
        ib = r[..., BEAM] * c
        if aniso is not None:
            circ, horiz, band = (np.asarray(a, dtype=np.float64) for a in aniso)
            rb = circumsolar_ratio(c, r[..., SUN_Z])
            iso = 1.0 - circ
            pbm = (ib * t) * scale
            ics = (r[..., DIFFUSE] * circ) * rb
            pcs = (ics * t) * scale
            ps = pbm + pcs
            dd = (r[..., DIFFUSE] * fs) * iso
            hv = (r[..., DIFFUSE] * horiz) * band
            dd = dd + hv
            gg = r[..., GROUND] * fg
            if shade is not None:
                f, fd, fgr = (np.asarray(a, dtype=np.float64) for a in shade)
                ps = ps * f
                dd = dd * fd
                gg = gg * fgr
            pb = np.where(c > 0.0, ps, 0.0)
            idf = dd + gg
            return pb, (idf * tau_diffuse) * scale
        pb = np.where(c > 0.0, (ib * t) * scale, 0.0)
        if shade is not None:
            f, fd, fgr = (np.asarray(a, dtype=np.float64) for a in shade)
            pb = np.where(c > 0.0, pb * f, 0.0)
            idf = (r[..., DIFFUSE] * fs) * fd + (r[..., GROUND] * fg) * fgr
        else:
            idf = r[..., DIFFUSE] * fs + r[..., GROUND] * fg
        pd = (idf * tau_diffuse) * scale
    return pb, pd


def received(pb, pd, en_surface, en_side, en_aperture, en_beam, en_diffuse, n_surfaces):
    """The raw solar value (before the gain) of every side: [..., 2, n_surfaces] (side 0 front, 1 back), and which sides
    have entries, [2, n_surfaces] of bool — the others are not written by the device.
    pb, pd  [..., n_apertures] from transmitted(); the entries as heat_solar_gains has them, in the caller's order:
            v = 0.0;  per entry of the receiver:  v = v + en_beam[i] * Pb[a_i];  v = v + en_diffuse[i] * Pd[a_i]"""
    pb, pd = np.asarray(pb, dtype=np.float64), np.asarray(pd, dtype=np.float64)
    S = int(n_surfaces)
    key = np.asarray(en_side, dtype=np.int64) * S + np.asarray(en_surface, dtype=np.int64)
    ap = np.asarray(en_aperture, dtype=np.int64)
    eb, ed = np.asarray(en_beam, dtype=np.float64), np.asarray(en_diffuse, dtype=np.float64)
    v = np.zeros(pb.shape[:-1] + (2 * S,))
    has = np.zeros(2 * S, dtype=bool)
    has[key] = True
    # entry j of every receiver at once: the chain of one receiver stays sequential in the caller's order
    order = np.argsort(key, kind="stable")
    k = key[order]
    start = np.flatnonzero(np.r_[True, k[1:] != k[:-1]]) if len(k) else np.zeros(0, np.int64)
    rank = np.arange(len(k)) - np.repeat(start, np.diff(np.r_[start, len(k)]))
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(rank.max()) + 1 if len(k) else 0):
            i = order[rank == j]
            at = key[i]
            x = v[..., at] + eb[i] * pb[..., ap[i]]
            v[..., at] = x + ed[i] * pd[..., ap[i]]
    return v.reshape(pb.shape[:-1] + (2, S)), has.reshape(2, S)


def distribute_by_area(md, aperture_surfaces):
    """The entry list of the common case: every side that faces the zone behind a window receives that window's beam and
    diffuse power in proportion to its area — so for each aperture sum(share * A_receiver) = 1. The zone behind a window is
    the one its back faces, else the one its front faces. A convenience, like sky.sun_direction — not part of the contract.
    Returns a dict of en_surface, en_side, en_aperture, en_beam, en_diffuse (aperture-major, fronts before backs)."""
    area = np.asarray(md["area"], dtype=np.float64)
    faces = [(np.asarray(md["front_kind"]) == mdl.SPACE, np.asarray(md["front_zone"])),
             (np.asarray(md["back_kind"]) == mdl.SPACE, np.asarray(md["back_zone"]))]
    Z = int(md["n_zones"])
    total = np.zeros(Z)
    for is_space, zone in faces:
        np.add.at(total, zone[is_space], area[is_space])
    members = []   # per zone: (surfaces, sides)
    for z in range(Z):
        surf = [np.flatnonzero(is_space & (zone == z)) for is_space, zone in faces]
        members.append((np.concatenate(surf), np.concatenate([np.full(len(s), side, np.uint8) for side, s in enumerate(surf)])))
    out = dict(en_surface=[], en_side=[], en_aperture=[], en_beam=[], en_diffuse=[])
    for a, w in enumerate(np.asarray(aperture_surfaces, dtype=np.int64)):
        if faces[1][0][w]:
            z = int(faces[1][1][w])
        elif faces[0][0][w]:
            z = int(faces[0][1][w])
        else:
            raise ValueError("aperture %d: surface %d faces no zone" % (a, w))
        surf, side = members[z]
        out["en_surface"].append(surf)
        out["en_side"].append(side)
        out["en_aperture"].append(np.full(len(surf), a, np.int32))
        out["en_beam"].append(np.full(len(surf), 1.0 / total[z]))
        out["en_diffuse"].append(np.full(len(surf), 1.0 / total[z]))
    dt = dict(en_surface=np.int64, en_side=np.uint8, en_aperture=np.int32, en_beam=np.float64, en_diffuse=np.float64)
    return {k: (np.concatenate(v) if v else np.zeros(0)).astype(dt[k]) for k, v in out.items()}
