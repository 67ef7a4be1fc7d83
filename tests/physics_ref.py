"""A high-precision restatement of the per-side physics, for tests only.

Written from the text of SIMPLE-BuildingSimulation/heat v1.0.2 (convection.rs:87-168, surface.rs:37-46, 228-308,
596-717, gas.rs:45-315, cavity.rs:59-69, discretization.rs:596-700) — not from the device code and not from the CPU
oracle, so that it can judge both.

Two rules:

* **Predicates are the reference's, in f64.** `delta_t`, `fabs`, `gamma % PI`, the `t_front > t_back` flip of the
  cavity angle, every threshold constant and every regime test are evaluated on f64 values exactly as the reference
  writes them: the branch taken is the branch the reference takes.
* **The smooth arithmetic inside a branch is extended precision** (numpy ``longdouble``: the 64-bit-mantissa x87
  format on these hosts, eps 1.08e-19). Every literal enters as its f64 value — `1./3.` is the f64 nearest to a
  third, `crate::PI` the f64 nearest to pi — because that is the number the reference computes with.

Every function takes a *field* ``F`` (default ``LD``): how numbers are made and which `pow`, `sqrt`, `sin`, `cos` act
on them. tests/test_physics_ref_host.py passes an mpmath field of 50 digits through the same text to measure what
``longdouble`` loses.
"""
import math

import numpy as np

assert np.finfo(np.longdouble).eps < 1e-18, "physics_ref needs an extended-precision longdouble (x87)"

SPACE, AMBIENT, OUTDOOR = 0, 1, 2
AIR, ARGON, KRYPTON, XENON = 0, 1, 2, 3

PI = math.pi                          # crate::PI as f64
SIGMA = 5.670374419e-8                # lib.rs:49
MIN_H = 0.1                           # convection.rs:22
ROUGHNESS_RF = 1.67                   # COEFFICIENTS[roughness_index = 1], convection.rs:157, surface.rs:618

# predicate constants, folded in f64 as rustc folds them (gas.rs:198-199, 138)
THIRTY_RAD = 30. * PI / 180.
EPSILON_RAD = 0.5 * PI / 180.
PI_RAD_180 = 180. * (PI / 180.)       # (180. as Float).to_radians()
B_0_60 = 2. * THIRTY_RAD - EPSILON_RAD
B_60 = 2. * THIRTY_RAD + EPSILON_RAD
B_60_90 = 3. * THIRTY_RAD - EPSILON_RAD
B_90 = 3. * THIRTY_RAD + EPSILON_RAD
B_180 = 6. * THIRTY_RAD
REGIME_BOUNDS = (B_0_60, B_60, B_60_90, B_90)
REGIMES = ("0_60", "60", "60_90", "90", "90_180")
RA_CELLS = ("le_1e4", "1e4_5e4", "gt_5e4")


class LD:
    """numpy longdouble."""
    eps = float(np.finfo(np.longdouble).eps)

    @staticmethod
    def num(x):
        return np.longdouble(x)

    @staticmethod
    def f64(x):
        return float(x)

    pow = staticmethod(lambda x, y: np.power(np.longdouble(x), np.longdouble(y)))
    sqrt = staticmethod(lambda x: np.sqrt(np.longdouble(x)))
    sin = staticmethod(lambda x: np.sin(np.longdouble(x)))
    cos = staticmethod(lambda x: np.cos(np.longdouble(x)))


# ---------------------------------------------------------------------------------------------------------------------
# convection.rs
def tarp_branch(air_t, surf_t, cos_tilt):
    """Which of the three coefficient forms convection.rs:91-103 takes: 'flat' (1.31), 'same' (9.482), 'opposite'
    (1.81). All in f64."""
    delta_t = air_t - surf_t
    if abs(delta_t) < 1e-3 or abs(cos_tilt) < 1e-3:
        return "flat"
    if (delta_t < 0. and cos_tilt < 0.) or (delta_t > 0. and cos_tilt > 0.):
        return "same"
    if (delta_t > 0. and cos_tilt < 0.) or (delta_t < 0. and cos_tilt > 0.):
        return "opposite"
    raise AssertionError("unreachable (NaN input)")


def tarp_natural(air_t, surf_t, cos_tilt, F=LD):
    """get_tarp_natural_convection_coefficient, convection.rs:87-110."""
    delta_t = air_t - surf_t                              # f64
    abs_delta_t = F.num(abs(delta_t))
    third = F.num(1. / 3.)
    branch = tarp_branch(air_t, surf_t, cos_tilt)
    if branch == "flat":
        h = F.num(1.31) * F.pow(abs_delta_t, third)
    elif branch == "same":
        h = F.num(9.482) * F.pow(abs_delta_t, third) / (F.num(7.238) - F.num(abs(cos_tilt)))
    else:
        h = F.num(1.81) * F.pow(abs_delta_t, third) / (F.num(1.382) + F.num(abs(cos_tilt)))
    return F.num(MIN_H) if h < F.num(MIN_H) else h


def tarp_forced(air_speed, area, perimeter, windward, F=LD):
    """The forced term of get_tarp_convection_coefficient, convection.rs:159-163."""
    wf = 1.0 if windward else 0.5
    return F.num(2.537) * F.num(wf) * F.num(ROUGHNESS_RF) * F.sqrt(F.num(perimeter) * F.num(air_speed) / F.num(area))


def tarp_total(air_t, surf_t, cos_tilt, air_speed, area, perimeter, windward, F=LD):
    """get_tarp_convection_coefficient, convection.rs:151-168."""
    return tarp_forced(air_speed, area, perimeter, windward, F) + tarp_natural(air_t, surf_t, cos_tilt, F)


# ---------------------------------------------------------------------------------------------------------------------
# surface.rs
def is_windward(wind_direction, cos_tilt, nx, ny):
    """surface.rs:37-46. The dot product is the reference's f64 one (`normal * wind_direction`, z term 0)."""
    if abs(cos_tilt) < 0.98:
        return nx * math.sin(wind_direction) + ny * math.cos(wind_direction) + 0.0 > 0.0
    return True


def rad_temperature(ir, F=LD):
    """(ir / SIGMA).powf(0.25) - 273.15, surface.rs:647,692."""
    return F.pow(F.num(ir) / F.num(SIGMA), F.num(0.25)) - F.num(273.15)


def side_hs(kind, is_front, air_t, ambient, t_first, t_last, cos_tilt, wind_speed, wind_modifier, area, perimeter,
            windward, F=LD):
    """front_hs / back_hs of calc_border_conditions, surface.rs:611-702. ``air_t`` is t_front or t_back (the zone's
    or the outdoor temperature), ``t_first``/``t_last`` the wall's first and last node temperatures.

    An AmbientTemperature *back* is evaluated on the FRONT node's temperature (surface.rs:677) — as the reference
    has it."""
    if kind == SPACE:
        return tarp_natural(air_t, t_first if is_front else t_last, cos_tilt, F)
    if kind == AMBIENT:
        return tarp_natural(ambient, t_first, cos_tilt, F)
    if kind == OUTDOOR:
        ct = -cos_tilt if is_front else cos_tilt                       # surface.rs:652
        return tarp_total(air_t, t_first if is_front else t_last, ct, wind_speed * wind_modifier, area, perimeter,
                          windward, F)
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------------
# gas.rs
_GAS = {  # thermal_conductivity, dynamic_viscosity, heat_capacity (polynomial coefficients, low order first), mass
    AIR: ((2.873e-3, 7.760e-5), (3.723e-6, 4.94e-8), (1002.7370, 1.2324e-2), 28.97),
    ARGON: ((2.285e-3, 5.149e-5), (3.379e-6, 6.451e-8), (521.9285,), 39.948),
    KRYPTON: ((9.443e-4, 2.826e-5), (2.213e-6, 7.777e-8), (248.0907,), 83.8),
    XENON: ((4.538e-4, 1.723e-5), (1.069e-6, 7.414e-8), (158.3397,), 131.30),
}


def _poly(coef, x, F):
    r = F.num(0.0)
    for c in reversed(coef):
        r = r * x + F.num(c)
    return r


def gas_thermal_conductivity(gas, temp, F=LD):
    return _poly(_GAS[gas][0], F.num(temp), F)


def gas_dynamic_viscosity(gas, temp, F=LD):
    return _poly(_GAS[gas][1], F.num(temp), F)


def gas_heat_capacity(gas, temp, F=LD):
    return _poly(_GAS[gas][2], F.num(temp), F)


def gas_mass(gas):
    return _GAS[gas][3]


def gas_density(gas, temp, F=LD):
    """gas.rs:175-179."""
    return F.num(101325.) * F.num(_GAS[gas][3]) / (F.num(8314.46261815324) * F.num(temp))


def raleigh(gas, t_front, t_back, thickness, F=LD):
    """gas.rs:82-102."""
    if abs(t_front - t_back) < 1e-10:
        return F.num(0.0000001)
    tf, tb, d = F.num(t_front), F.num(t_back), F.num(thickness)
    temp = ((tf + F.num(273.15)) + (tb + F.num(273.15))) / F.num(2.)
    beta = F.num(1.) / temp
    c_p = gas_heat_capacity(gas, temp, F)
    mu = gas_dynamic_viscosity(gas, temp, F)
    lam = gas_thermal_conductivity(gas, temp, F)
    rho = gas_density(gas, temp, F)
    return rho * rho * (d * d * d) * F.num(9.81) * beta * c_p * abs(tf - tb) / (mu * lam)


def regime_of(gamma):
    """The branch of `nusselt` (gas.rs:201-220) for an angle already past the flip; f64."""
    gamma = math.fmod(gamma, PI)
    if 0.0 <= gamma < B_0_60:
        return "0_60"
    if gamma < B_60:
        return "60"
    if gamma < B_60_90:
        return "60_90"
    if gamma < B_90:
        return "90"
    if gamma < B_180:
        return "90_180"
    raise AssertionError("unreachable: gamma is %r" % gamma)


def ra_cell(ra):
    """The branch of nu_90 (gas.rs:286-297) for a Rayleigh number; f64."""
    ra = float(ra)
    if ra <= 1e4:
        return "le_1e4"
    if ra < 5e4:
        return "1e4_5e4"
    if ra > 5e4:
        return "gt_5e4"
    raise AssertionError("unreachable: ra is exactly 5e4")


def _powi(x, n):
    r = x
    for _ in range(n - 1):
        r = r * x
    return r


def nu_0_60(ra, gamma, F=LD):
    """gas.rs:227-244."""
    def aux(x):
        return (x + abs(x)) / F.num(2.)
    g = F.num(gamma)
    cos_gamma = F.cos(g)
    a = aux(F.num(1.) - F.num(1708.) / (ra * cos_gamma))
    b = F.num(1.) - F.num(1708.) * F.pow(F.sin(F.num(1.8) * g), F.num(1.6)) / (ra * cos_gamma)
    c = F.pow(ra * cos_gamma / F.num(5830.), F.num(1. / 3.)) - F.num(1.)
    return F.num(1.) + F.num(1.44) * a * b + aux(c)


def nu_60(ra, a_gi, F=LD):
    """gas.rs:249-263."""
    g = F.num(0.5) / F.pow(F.num(1.) + F.pow(ra / F.num(3160.), F.num(20.6)), F.num(0.1))
    nu1 = F.pow(F.num(1.) + _powi(F.num(0.0936) * F.pow(ra, F.num(0.314)) / (F.num(1.) + g), 7), F.num(1. / 7.))
    nu2 = (F.num(0.104) + F.num(0.175) / a_gi) * F.pow(ra, F.num(0.283))
    return nu1 if nu1 > nu2 else nu2


def nu_90(ra, a_gi, F=LD):
    """gas.rs:285-307."""
    cell = ra_cell(F.f64(ra))
    if cell == "le_1e4":
        nu1 = F.num(1.) + F.num(1.7596678) * F.num(1e-10) * F.pow(ra, F.num(2.2984755))
    elif cell == "1e4_5e4":
        nu1 = F.num(0.028154) * F.pow(ra, F.num(0.4134))
    else:
        nu1 = F.num(0.0673838) * F.pow(ra, F.num(1. / 3.))
    nu2 = F.num(0.242) * F.pow(ra / a_gi, F.num(0.272))
    return nu1 if nu1 > nu2 else nu2


def nu_60_90(ra, gamma, a_gi, F=LD):
    """gas.rs:269-280."""
    nu60 = nu_60(ra, a_gi, F)
    nu90 = nu_90(ra, a_gi, F)
    pi = F.num(PI)
    x = (F.num(gamma) - pi / F.num(3.)) / (pi / F.num(2.) - pi / F.num(3.))
    return nu60 + (nu90 - nu60) * x


def nu_90_180(ra, a_gi, gamma, F=LD):
    """gas.rs:312-315."""
    return F.num(1.) + (nu_90(ra, a_gi, F) - F.num(1.)) * F.sin(F.num(gamma))


def nusselt(ra, gamma, a_gi, F=LD):
    """gas.rs:197-221. ``gamma`` is f64; ``ra`` and ``a_gi`` are field numbers (or f64)."""
    ra, a_gi = F.num(ra), F.num(a_gi)
    gamma = math.fmod(gamma, PI)
    regime = regime_of(gamma)
    if regime == "0_60":
        return nu_0_60(ra, gamma, F)
    if regime == "60":
        return nu_60(ra, a_gi, F)
    if regime == "60_90":
        return nu_60_90(ra, gamma, a_gi, F)
    if regime == "90":
        return nu_90(ra, a_gi, F)
    return nu_90_180(ra, a_gi, gamma, F)


def flipped_angle(gamma, t_front, t_back):
    """gas.rs:137-139, f64."""
    return PI_RAD_180 - gamma if t_front > t_back else gamma


def cavity_convection(gas, height, thickness, gamma, t_front, t_back, F=LD):
    """gas.rs:126-152."""
    gamma = flipped_angle(gamma, t_front, t_back)
    a_gi = F.num(height) / F.num(thickness)
    ra = raleigh(gas, t_front, t_back, thickness, F)
    nu = nusselt(ra, gamma, a_gi, F)
    temp = ((F.num(t_front) + F.num(273.15)) + (F.num(t_back) + F.num(273.15))) / F.num(2.)
    return nu * gas_thermal_conductivity(gas, temp, F) / F.num(thickness)


def cavity_labels(cav, t_front, t_back):
    """(regime, Rayleigh cell) that Cavity::u_value lands in, from the reference's own tests."""
    gamma = flipped_angle(float(cav["angle"]), t_front, t_back)
    ra = raleigh(int(cav["gas"]), t_front, t_back, float(cav["thickness"]))
    return regime_of(gamma), ra_cell(float(ra))


def cavity_u_value(cav, t_front, t_back, F=LD):
    """Cavity::u_value, cavity.rs:59-69. ``cav`` has thickness, height, angle, eout, ein, gas."""
    conv = cavity_convection(int(cav["gas"]), float(cav["height"]), float(cav["thickness"]), float(cav["angle"]),
                             t_front, t_back, F)
    tm = (F.num(t_back) + F.num(t_front)) / F.num(2.) + F.num(273.15)
    ein, eout = F.num(float(cav["ein"])), F.num(float(cav["eout"]))
    rad = F.num(4.) * (tm * tm * tm) * F.num(SIGMA) * ein * eout / (F.num(1.) - (F.num(1.) - ein) * (F.num(1.) - eout))
    return rad + conv


# ---------------------------------------------------------------------------------------------------------------------
# discretization.rs:596-700, surface.rs:168-187, 228-308: one frozen-K RK4 step of an all-massive wall (one chunk)
def rad_hs(emissivity, rad_t, surf_t, F=LD):
    """4 eps SIGMA (273.15 + (rad_t + surf_t)/2)^3, surface.rs:941-948."""
    t = F.num(273.15) + (F.num(rad_t) + F.num(surf_t)) / F.num(2.)
    return F.num(4.) * F.num(emissivity) * F.num(SIGMA) * (t * t * t)


def _tri_prod(lo, dg, up, x, F):
    n = len(x)
    y = []
    for i in range(n):
        v = dg[i] * x[i]
        if i > 0:
            v = v + lo[i] * x[i - 1]
        if i < n - 1:
            v = v + up[i] * x[i + 1]
        y.append(v)
    return y


def massive_wall_step(mass, u_of_segment, temps, dt, front, back, solar=None, F=LD):
    """One march_mass (surface.rs:720-787) of a wall that is a single massive chunk [0, n).

    ``u_of_segment[i]`` is a number (UValue::Solid) or a cavity record (UValue::Cavity) for the segment between node i
    and i+1; ``front``/``back`` are dicts with air_t, rad_t, hs and rad_hs (field numbers or f64). Returns the n
    temperatures after the step, as field numbers. K and q are frozen at ``temps`` (get_k_q), scaled by dt/C
    (rearrange_k), and pushed through the literal four stages of rk4."""
    n = len(mass)
    T = [F.num(t) for t in temps]
    zero = F.num(0.0)
    lo, dg, up, q = [zero] * n, [zero] * n, [zero] * n, [zero] * n
    for i in range(n - 1):
        seg = u_of_segment[i]
        if isinstance(seg, (np.void, dict)):
            u = cavity_u_value(seg, float(temps[i]), float(temps[i + 1]), F)
        else:
            u = F.num(seg)
        dg[i] = dg[i] - u
        dg[i + 1] = dg[i + 1] - u
        up[i] = up[i] + u
        lo[i + 1] = lo[i + 1] + u
    q[0] = q[0] + (F.num(front["air_t"]) * F.num(front["hs"]) + F.num(front["rad_hs"]) * (F.num(front["rad_t"]) - T[0]))
    dg[0] = dg[0] - F.num(front["hs"])
    q[n - 1] = q[n - 1] + (F.num(back["air_t"]) * F.num(back["hs"])
                           + F.num(back["rad_hs"]) * (F.num(back["rad_t"]) - T[n - 1]))
    dg[n - 1] = dg[n - 1] - F.num(back["hs"])
    if solar is not None:
        q = [q[i] + F.num(solar[i]) for i in range(n)]
    for i in range(n):                                    # rearrange_k
        v = F.num(dt) / F.num(mass[i])
        lo[i], dg[i], up[i], q[i] = lo[i] * v, dg[i] * v, up[i] * v, q[i] * v
    half = F.num(0.5)

    def f(x):
        return [a + b for a, b in zip(_tri_prod(lo, dg, up, x, F), q)]
    k1 = f(T)
    k2 = f([t + half * k for t, k in zip(T, k1)])
    k3 = f([t + half * k for t, k in zip(T, k2)])
    k4 = f([t + k for t, k in zip(T, k3)])
    return [t + a / F.num(6.) + b / F.num(3.) + c / F.num(3.) + d / F.num(6.)
            for t, a, b, c, d in zip(T, k1, k2, k3, k4)]
