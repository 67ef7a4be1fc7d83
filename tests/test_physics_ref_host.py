"""tests/physics_ref.py judged from both sides, on the CPU.

(a) Against mpmath at 50 digits. The same text (the reference's formulas, its f64 predicates) is evaluated once in
    numpy longdouble and once in a 50-digit mpmath field: the distance is what longdouble loses.
(b) The CPU oracle's exported leaf functions (oracle/heat_oracle.c, plain f64) against physics_ref. A distance above
    a few f64 roundings would be a transcription difference in one of the two.

Both run over the sweeps of tests/helpers.py that the GPU edge tests use (tarp_sweep, WIND_SWEEP x NORMALS x GEOMETRY,
cavity_sweep with the exact regime-boundary angles added).

Measured (worst relative distance over the sweeps; x86-64, glibc libm):

    physics_ref against mpmath       tarp_natural 9.5e-20   tarp_total 7.3e-20   raleigh 4.2e-19   nusselt 1.4e-19
                                     u_value 2.1e-19        one RK4 step of a cavity wall 6.2e-20
    oracle against physics_ref       tarp_natural  flat 1.10e-16   same 1.41e-16   opposite 1.48e-16
                                     tarp_total 2.60e-16    gas properties 2.06e-16    raleigh 1.03e-15
                                     nusselt   0_60 2.34e-16   60 7.67e-17   60_90 1.26e-16   90 1.17e-16   90_180 1.90e-16
      or_cavity_u_value, by regime   Rayleigh <= 1e4    1e4 .. 5e4    > 5e4
                     0 .. 60 deg        3.61e-16         3.45e-16    3.43e-16
                     60 deg             3.80e-16         3.32e-16    3.16e-16
                     60 .. 90 deg       3.93e-16         5.48e-16    3.80e-16
                     90 deg             4.54e-16         3.42e-16    3.43e-16
                     90 .. 180 deg      6.27e-16         5.28e-16    4.10e-16

No transcription difference between the oracle and the reference's text was found: every distance is a few f64
roundings, also at the angles that are the f64 value of a regime boundary (the oracle takes the reference's branch).
"""
import ctypes as C
import math

import numpy as np
import pytest

import helpers as h
import physics_ref as pr

# A bound on the oracle's distance from exact arithmetic on the reference's text, per function: the number of f64
# roundings on the longest path through it (a libm pow, cbrt, sin or cos counted as one rounding of 1 ulp, an
# arithmetic operation as half an ulp), in units of 2^-53 = 1.11e-16.
#   tarp_natural  pow, *, -, /                                  -> 5
#   tarp_total    + sqrt(* /) * * * and the sum                 -> 5 + 6
#   gas property  Horner step (*, +)                            -> 2; density 2
#   raleigh       mean T (3), 1/T, 3 polynomials (2 + 2 on T), rho^2 (2+2), d^3 (2), 6 products, /  -> 24
#   nusselt       two pow chains of nu_60 (about 12), interpolation or sine (4)  -> 16, on an exact Rayleigh number
#   u_value       raleigh feeds a power of at most 0.4134 (x 0.42 of its error: 10), nusselt 16, lambda / d (4),
#                 the radiant term and the sum (8, shared)      -> 32
ULP = 2.0 ** -53
BOUND = dict(tarp_natural=5 * ULP, tarp_total=11 * ULP, gas=3 * ULP, raleigh=24 * ULP, nusselt=16 * ULP,
             u_value=32 * ULP)


@pytest.fixture(scope="module")
def lib(oracle):
    return oracle.lib()


def _cav_struct(oracle, cv):
    return oracle.Cavity(float(cv["thickness"]), float(cv["height"]), float(cv["angle"]), float(cv["eout"]),
                         float(cv["ein"]), int(cv["gas"]), 0)


def _all_cavities():
    cavs, tf, tb = h.cavity_sweep()
    ecavs, etf, etb = h.cavity_sweep(h.cavity_exact_angles())
    return np.concatenate([cavs, ecavs]), np.concatenate([tf, etf]), np.concatenate([tb, etb])


def _nusselt_sweep():
    ras = [1e-7, 3.0, 1708.0, 3160.0, 9999.0, 1e4, float(np.nextafter(1e4, 2e4)), 2.3e4, float(np.nextafter(5e4, 0)),
           float(np.nextafter(5e4, 1e5)), 8e4, 1e6, 4e7]
    return [(ra, g, 1.0 / th) for ra in ras for g in h.cavity_angles() + list(pr.REGIME_BOUNDS) for th in (0.006, 0.0127, 0.1)]


# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_leaf_functions_against_the_high_precision_reference(oracle, lib):
    err = C.c_int(0)
    worst = {}

    def note(key, got, ref):
        d = h.rel_distance(got, ref)
        if d > worst.get(key, 0.0):
            worst[key] = d
        return d

    for air, surf, c in h.tarp_sweep():
        note("tarp_natural " + pr.tarp_branch(air, surf, c), lib.or_tarp_natural(air, surf, c, C.byref(err)),
             pr.tarp_natural(air, surf, c))
        for i, (wd, ws) in enumerate(h.WIND_SWEEP):
            area, per, wm = h.GEOMETRY[i % len(h.GEOMETRY)]
            for windward in (0, 1):
                note("tarp_total", lib.or_tarp_total(air, surf, c, ws * wm, area, per, windward, C.byref(err)),
                     pr.tarp_total(air, surf, c, ws * wm, area, per, bool(windward)))
    assert err.value == 0
    for wd, _ in h.WIND_SWEEP + [(math.pi / 2, 1.0), (math.pi, 1.0), (1.0, 1.0)]:
        for c in h.COS_EDGES:
            for nx, ny in h.NORMALS:
                assert bool(lib.or_is_windward(wd, c, nx, ny)) == pr.is_windward(wd, c, nx, ny), (wd, c, nx, ny)
    assert not pr.is_windward(0.0, 0.0, 1.0, 0.0) and not pr.is_windward(0.0, 0.0, -1.0, 0.0)   # a dot product of exactly 0
    assert pr.is_windward(0.0, 0.98, 0.0, -1.0) and not pr.is_windward(0.0, float(np.nextafter(0.98, 0)), 0.0, -1.0)

    for gas in range(4):
        for t in np.linspace(230.0, 340.0, 23):
            note("gas", lib.or_gas_thermal_conductivity(gas, t), pr.gas_thermal_conductivity(gas, t))
            note("gas", lib.or_gas_dynamic_viscosity(gas, t), pr.gas_dynamic_viscosity(gas, t))
            note("gas", lib.or_gas_heat_capacity(gas, t), pr.gas_heat_capacity(gas, t))
            note("gas", lib.or_gas_density(gas, t), pr.gas_density(gas, t))
        assert lib.or_gas_mass(gas) == pr.gas_mass(gas)

    cavs, tf, tb = _all_cavities()
    cells = set()
    for cv, a, b in zip(cavs, tf, tb):
        cell = pr.cavity_labels(cv, a, b)
        cells.add(cell)
        note("raleigh", lib.or_raleigh(int(cv["gas"]), a, b, float(cv["thickness"])),
             pr.raleigh(int(cv["gas"]), a, b, float(cv["thickness"])))
        cs = _cav_struct(oracle, cv)
        note("u_value %s %s" % cell, lib.or_cavity_u_value(C.byref(cs), a, b, C.byref(err)), pr.cavity_u_value(cv, a, b))
    assert err.value == 0
    assert cells == {(r, c) for r in pr.REGIMES for c in pr.RA_CELLS}, sorted(cells)

    for ra, g, a_gi in _nusselt_sweep():
        note("nusselt " + pr.regime_of(g), lib.or_nusselt(ra, g, a_gi, C.byref(err)), pr.nusselt(ra, g, a_gi))
    assert err.value == 0

    for key in sorted(worst):
        print("oracle vs physics_ref  %-28s %.2e" % (key, worst[key]))
    for key, d in worst.items():
        assert d <= BOUND[key.split()[0]], (key, d)


def test_rad_temperature_and_rad_hs():
    for t in (-30.0, 0.0, 21.5, 55.0):
        ir = pr.SIGMA * (t + 273.15) ** 4
        assert abs(float(pr.rad_temperature(ir)) - t) < 1e-12
        assert h.rel_distance(4 * 0.9 * pr.SIGMA * (273.15 + t) ** 3, pr.rad_hs(0.9, t, t)) < 8 * ULP


def test_rk4_step_of_the_reference_closed_form():
    """surface.rs:1558-1620 (test_rk4): one node of mass C between two airs through conductances of h each relaxes as
    exp(-2 h t / C); ten steps of the frozen-K RK4 follow it to the method's order."""
    c, hh, dt, t0, tair = 1700. * 800. * 0.02, 10.0, 30.0, 22.0, 5.0
    T = [t0, t0]
    side = dict(air_t=tair, rad_t=tair, hs=hh, rad_hs=0.0)
    for _ in range(10):
        T = [float(x) for x in pr.massive_wall_step([c / 2, c / 2], [1e9], T, dt, side, side)]
    exact = tair + (t0 - tair) * math.exp(-2 * hh * 10 * dt / c)
    assert abs(0.5 * (T[0] + T[1]) - exact) < 1e-6 and abs(T[0] - T[1]) < 1e-9


# ---------------------------------------------------------------------------------------------------------------------
def test_physics_ref_against_mpmath_at_50_digits():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50

    class MP:
        num = staticmethod(lambda x: x if isinstance(x, mp.mpf) else mp.mpf(float(x)))
        f64 = staticmethod(float)
        pow = staticmethod(mp.power)
        sqrt = staticmethod(mp.sqrt)
        sin = staticmethod(mp.sin)
        cos = staticmethod(mp.cos)

    def exact(x):
        x = np.longdouble(x)
        hi = float(x)
        return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))

    worst = {}

    def note(key, ld, ref):
        d = float(abs(exact(ld) - ref) / abs(ref))
        worst[key] = max(worst.get(key, 0.0), d)

    for air, surf, c in h.tarp_sweep():
        note("tarp_natural", pr.tarp_natural(air, surf, c), pr.tarp_natural(air, surf, c, MP))
        wd, ws = h.WIND_SWEEP[3]
        area, per, wm = h.GEOMETRY[1]
        note("tarp_total", pr.tarp_total(air, surf, c, ws * wm, area, per, False),
             pr.tarp_total(air, surf, c, ws * wm, area, per, False, MP))
    cavs, tf, tb = _all_cavities()
    for cv, a, b in zip(cavs, tf, tb):
        note("raleigh", pr.raleigh(int(cv["gas"]), a, b, float(cv["thickness"])),
             pr.raleigh(int(cv["gas"]), a, b, float(cv["thickness"]), MP))
        note("u_value", pr.cavity_u_value(cv, a, b), pr.cavity_u_value(cv, a, b, MP))
    for ra, g, a_gi in _nusselt_sweep():
        note("nusselt", pr.nusselt(ra, g, a_gi), pr.nusselt(ra, g, a_gi, MP))
    # one RK4 step of a four-node wall with a cavity, as the GPU test builds it
    cv = cavs[len(cavs) // 2]
    T = [20.0, 19.5, 4.5, 4.0]
    side_f = dict(air_t=21.0, rad_t=21.0, hs=8.0, rad_hs=0.0)
    side_b = dict(air_t=2.0, rad_t=2.0, hs=12.0, rad_hs=0.0)
    a = pr.massive_wall_step([750.0] * 4, [5.0, cv, 5.0], T, 30.0, side_f, side_b)
    b = pr.massive_wall_step([750.0] * 4, [5.0, cv, 5.0], T, 30.0, side_f, side_b, F=MP)
    for x, y in zip(a, b):
        note("rk4 step", x, y)
    for key in sorted(worst):
        print("physics_ref vs mpmath  %-14s %.2e" % (key, worst[key]))
    # longdouble keeps 64 bits (eps 1.08e-19); the longest path (u_value) is some 60 operations, and the power 20.6
    # of nu_60 multiplies the error of its argument by 20.6: 100 eps bounds every one of them, 1/20 of an f64 ulp.
    for key, d in worst.items():
        assert d <= 100 * pr.LD.eps, (key, d)
