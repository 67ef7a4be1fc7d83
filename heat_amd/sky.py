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


def incident(record, normal, side, shade=None):
    """The incident irradiance (before the gain) of one kind of input of one side.
    record  [..., 8]: heat_sky_record fields (FIELDS), broadcast against the normals' leading shape
    normal  (x, y, z) of the FRONT face's outward normal, arrays or scalars
    side    "solar_front", "solar_back", "ir_front" or "ir_back" (a back side sees the component-wise negation)
    shade   None, or (f, fd, fg) of a shaded solar side (heat_shades): the step's sunlit fraction from shading.sunlit and the
            shade's diffuse and ground factor, broadcast like the normals
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
            if shade is not None:
                f, fd, fgr = (np.asarray(a, dtype=np.float64) for a in shade)
                bm = bm * f
                dv = (r[..., DIFFUSE] * fs) * fd
                gv = (r[..., GROUND] * fg) * fgr
                return (bm + dv) + gv
            return (bm + r[..., DIFFUSE] * fs) + r[..., GROUND] * fg
        if shade is not None:
            raise ValueError("a shade acts on a solar input, not on %r" % (side,))
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
