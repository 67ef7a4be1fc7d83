"""Sky of a series on the host (include/heat_amd.h, heat_sky): the rule the device applies to every sky-driven side at every
step, in numpy, and a sun-position convenience for tools and examples. No device, no library.

incident() IS the contract's rule, line for line — every product and sum one rounded f64 operation in the header's order
(numpy never fuses a multiply-add) — and so the reference of the tests: a host that writes its values into the irradiance
slots between heat_batch_march_ex calls gets the bits of heat_batch_march_series_sky.
The reference has no counterpart: solar geometry lives in another SIMPLE crate, and its harness reads EnergyPlus' incident
irradiance from CSV (validate_wall_heat_transfer.rs:675-705)."""
import numpy as np

FIELDS = ("sun_x", "sun_y", "sun_z", "beam", "diffuse", "ground", "ir_sky", "ir_ground")
SUN_X, SUN_Y, SUN_Z, BEAM, DIFFUSE, GROUND, IR_SKY, IR_GROUND = range(8)


Z0 = 0.08715574274765817   # cos 85 deg: the literal is the contract (heat_sky_aniso)


def circumsolar_ratio(c, sun_z):
    """rb of heat_sky_aniso: c / max(Z0, sun_z) where the plane sees a sun above the horizon, else 0. One division."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        up = sun_z > 0.0
        zb = np.where(sun_z > Z0, sun_z, Z0)
        return np.where((c > 0.0) & up, c / zb, 0.0)


def incident(record, normal, side, shade=None, aniso=None):
    """The incident irradiance (before the gain) of one kind of input of one side.
    record  [..., 8]: heat_sky_record fields (FIELDS), broadcast against the normals' leading shape
    normal  (x, y, z) of the FRONT face's outward normal, arrays or scalars
    side    "solar_front", "solar_back", "ir_front" or "ir_back" (a back side sees the component-wise negation)
    shade   None, or (f, fd, fg) of a shaded solar side (heat_shades): the step's sunlit fraction from shading.sunlit and the
            shade's diffuse and ground factor, broadcast like the normals
    aniso   None, or (circ, horiz, band) of heat_sky_aniso: the coefficient pair of the record's site at the step and the
            band of the side, broadcast like the normals; a solar side then follows the anisotropic rule
    Returns an array of the broadcast shape."""
    if side not in ("solar_front", "solar_back", "ir_front", "ir_back"):
        raise ValueError("side is solar_front, solar_back, ir_front or ir_back, not %r" % (side,))
    r = np.asarray(record, dtype=np.float64)
    nx, ny, nz = (np.asarray(a, dtype=np.float64) for a in normal)
    if side.endswith("back"):
        nx, ny, nz = -nx, -ny, -nz
    with np.errstate(invalid="ignore", over="ignore"):
        fs = 0.5 + 0.5 * nz
        fg = 0.5 - 0.5 * nz
        if side.startswith("solar"):
            c = (nx * r[..., SUN_X] + ny * r[..., SUN_Y]) + nz * r[..., SUN_Z]
            bm = np.where(c > 0.0, r[..., BEAM] * c, 0.0)
            if aniso is not None:
                circ, horiz, band = (np.asarray(a, dtype=np.float64) for a in aniso)
                rb = circumsolar_ratio(c, r[..., SUN_Z])
                iso = 1.0 - circ
                cs = (r[..., DIFFUSE] * circ) * rb
                sun = bm + cs
                dv = (r[..., DIFFUSE] * fs) * iso
                hv = (r[..., DIFFUSE] * horiz) * band
                dv = dv + hv
                gv = r[..., GROUND] * fg
                if shade is not None:
                    f, fd, fgr = (np.asarray(a, dtype=np.float64) for a in shade)
                    sun = sun * f
                    dv = dv * fd
                    gv = gv * fgr
                return (sun + dv) + gv
            if shade is not None:
                f, fd, fgr = (np.asarray(a, dtype=np.float64) for a in shade)
                bm = bm * f
                dv = (r[..., DIFFUSE] * fs) * fd
                gv = (r[..., GROUND] * fg) * fgr
                return (bm + dv) + gv
            return (bm + r[..., DIFFUSE] * fs) + r[..., GROUND] * fg
        if shade is not None:
            raise ValueError("a shade acts on a solar input, not on %r" % (side,))
        if aniso is not None:
            raise ValueError("the anisotropic sky acts on a solar input, not on %r" % (side,))
        return r[..., IR_SKY] * fs + r[..., IR_GROUND] * fg


def sun_direction(day_of_year, solar_hour, latitude_rad):
    """Unit vector towards the sun (x east, y north, z up) from the declination and hour-angle formula:
    declination = 23.45 deg * sin(2 pi (284 + day) / 365) (Cooper), hour angle = 15 deg per hour from solar noon.
    A convenience for tools and examples — not part of the contract: the library takes whatever vector the caller gives.
    Arguments broadcast; returns [..., 3]. z < 0: the sun is below the horizon."""
    day = np.asarray(day_of_year, dtype=np.float64)
    hour = np.asarray(solar_hour, dtype=np.float64)
    lat = np.asarray(latitude_rad, dtype=np.float64)
    decl = np.radians(23.45) * np.sin(2.0 * np.pi * (284.0 + day) / 365.0)
    h = np.radians(15.0) * (hour - 12.0)
    z = np.sin(lat) * np.sin(decl) + np.cos(lat) * np.cos(decl) * np.cos(h)
    y = np.cos(lat) * np.sin(decl) - np.sin(lat) * np.cos(decl) * np.cos(h)   # towards north
    x = -np.cos(decl) * np.sin(h)                                             # morning (h < 0): in the east
    return np.stack(np.broadcast_arrays(x, y, z), axis=-1)


SOLAR_CONSTANT = 1367.0   # W/m2


def _circumsolar(record, day_of_year):
    r = np.asarray(record, dtype=np.float64)
    day = np.asarray(day_of_year, dtype=np.float64)
    extra = SOLAR_CONSTANT * (1.0 + 0.033 * np.cos(2.0 * np.pi * day / 365.0))
    return r, np.clip(r[..., BEAM] / extra, 0.0, 1.0)


def hay_davies(record, day_of_year):
    """(circ, horiz) of the Hay-Davies model: circ = the anisotropy index, beam normal irradiance over the extraterrestrial
    normal irradiance 1367 (1 + 0.033 cos(2 pi day / 365)), clipped to [0, 1]; horiz = 0. record [..., 8], the day broadcast
    against its leading shape. A convenience like sun_direction — not part of the contract."""
    r, circ = _circumsolar(record, day_of_year)
    return circ, np.zeros_like(circ)


def reindl(record, day_of_year):
    """(circ, horiz) of the Reindl model: Hay-Davies' circ, and horiz = (1 - circ) sqrt(beam_h / (beam_h + diffuse)) with
    beam_h = beam * max(sun_z, 0) the beam on the horizontal; 0 where the denominator is 0. Use with band_reindl."""
    r, circ = _circumsolar(record, day_of_year)
    beam_h = r[..., BEAM] * np.maximum(r[..., SUN_Z], 0.0)
    total = beam_h + r[..., DIFFUSE]
    with np.errstate(invalid="ignore", divide="ignore"):
        root = np.where(total > 0.0, np.sqrt(beam_h / np.where(total > 0.0, total, 1.0)), 0.0)
    return circ, (1.0 - circ) * root


def band_reindl(normal):
    """Reindl's horizon term of a plane: fs sin^3(tilt / 2) = fs ((1 - n.z) / 2)^1.5, fs = 0.5 + 0.5 n.z. 0 on a horizontal
    plane: there reindl equals hay_davies."""
    nz = np.asarray(normal[2], dtype=np.float64)
    return (0.5 + 0.5 * nz) * np.maximum((1.0 - nz) / 2.0, 0.0) ** 1.5


def band_perez(normal):
    """Perez' horizon term of a plane: sin(tilt) = sqrt(max(0, 1 - n.z^2)); 1 on a vertical wall. (Perez' F1, F2 come from a
    table of coefficients by clearness bin, which this module does not carry.)"""
    nz = np.asarray(normal[2], dtype=np.float64)
    return np.sqrt(np.maximum(0.0, 1.0 - nz * nz))
