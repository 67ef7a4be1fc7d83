"""The two forms of the fast path's RK4 (kernels.hip: apply_A / rk4_horner and apply_PQ / rk4_horner_pq), restated in numpy
and held against the four literal RK4 stages (surface.rs:268-305) in extended precision.

  flux form          (A x)_j = V_j (f_j - f_{j-1}),  f_j = U_j (x_{j+1} - x_j): what every kernel but the converted
                     cluster-resident instantiations runs;
  coefficient form   (A x)_j = P_j g_j - Q_j g_{j-1},  g_j = x_{j+1} - x_j,  P_j = V_j U_j,  Q_j = V_j U_{j-1}, the two
                     products rounded once per block, the Horner term as the addend of the first of two FMAs.
Both take the differences first, so neither cancels rows of A against each other; what the coefficient form gives up is
the common rounding of V_j (f_j - f_{j-1}). The bound below is set against the flux form, the form the project's 1e-9
tests have always passed with, NOT against what the new code gives: on the same input the coefficient form's worst error
over a wall may be at most 4 times the flux form's, plus a floor of 8 ulp of the wall's largest temperature (for inputs
where the flux form happens to be exact to the last bit). The largest temperature is taken over the wall's temperatures
before AND after the step, the latter from the extended-precision reference: a light face node under a strong source
moves by tens of kelvin in one step here, and no form can state a result of 89 K closer than half an ulp of 89 K, whatever
the wall started from.

Both restatements round every operation to f64 as the kernel's source has it; an FMA is one rounding of the sum formed
in extended precision (64 mantissa bits: within 2^-11 ulp of the exact FMA — far below what is compared). The flux form
is restated without contraction: the compiler contracts some of its products, which moves single roundings, not the
bound's factor of 4.

Inputs: random walls of 2 to 64 nodes; conductances log-uniform over six decades from layer to layer (ratios up to 1e6);
V = dt / C so that V_j (U_{j-1} + U_j) is log-uniform in [1e-6, 2] — from nodes that hardly move to the edge of RK4's
stability —, with a share of the nodes at V = 1e-6 outright; face conductances up to 1e3 W/m2K with the face nodes' V
drawn the same way against them; temperatures between -10 and 40.
"""
import numpy as np
import pytest

LD = np.longdouble
SIZES = [2, 3, 4, 5, 8, 15, 16, 17, 20, 31, 32, 33, 48, 63, 64]
WALLS = 400                    # per size
FACTOR, FLOOR_ULP = 4.0, 8.0   # the issue's bound


def walls(n, seed):
    rng = np.random.default_rng(seed)
    B = WALLS
    U = 10.0 ** rng.uniform(-3, 3, (B, n - 1))                     # between nodes j and j + 1
    big = rng.random((B, 2)) < 0.5
    h = np.where(big, 10.0 ** rng.uniform(1, 3, (B, 2)), rng.uniform(0.5, 25.0, (B, 2)))   # hF, hB
    left = np.concatenate([h[:, :1], U], axis=1)                   # conductance to the left of node j
    right = np.concatenate([U, h[:, 1:]], axis=1)
    V = 10.0 ** rng.uniform(-6, np.log10(2.0), (B, n)) / (left + right)
    V = np.where(rng.random((B, n)) < 0.1, 1e-6, V)
    V = np.minimum(V, 2.0 / (left + right))
    T = rng.uniform(-10, 40, (B, 1)) + rng.uniform(-5, 5, (B, n))
    q = h * rng.uniform(-10, 40, (B, 2)) + rng.uniform(0, 800, (B, 2))   # h * T_air + absorbed radiation
    return dict(U=U, V=V, T=T, hF=h[:, 0], hB=h[:, 1], qF=q[:, 0], qB=q[:, 1])


def literal_stages(w):
    """surface.rs:268-305 in extended precision: k1..k4 with K and q frozen, T + (k1 + 2 k2 + 2 k3 + k4) / 6."""
    U, V, T = LD(w["U"]), LD(w["V"]), LD(w["T"])
    hF, hB, qF, qB = (LD(w[k])[:, None] for k in ("hF", "hB", "qF", "qB"))

    def rhs(x):
        f = U * (x[:, 1:] - x[:, :-1])
        fl = np.concatenate([hF * x[:, :1] - qF, f], axis=1)       # flux from the left of node j
        fr = np.concatenate([f, qB - hB * x[:, -1:]], axis=1)      # flux to the right
        return V * (fr - fl)
    k1 = rhs(T)
    k2 = rhs(T + k1 / 2)
    k3 = rhs(T + k2 / 2)
    k4 = rhs(T + k3)
    return T + (k1 + 2 * k2 + 2 * k3 + k4) / 6


def flux_form(w):
    """rk4_horner over apply_A, every operation rounded to f64."""
    U, V, T = w["U"], w["V"], w["T"]
    hF, hB, qF, qB = (w[k][:, None] for k in ("hF", "hB", "qF", "qB"))
    zero = np.zeros_like(T[:, :1])

    def apply_A(x, affine):
        xr = np.concatenate([x[:, 1:], zero], axis=1)              # the node behind the last one is held at 0
        f = np.concatenate([U, hB], axis=1) * (xr - x)
        fprev0 = hF * (x[:, :1] - zero)
        if affine:
            f[:, -1:] = f[:, -1:] + qB
            fprev0 = fprev0 - qF
        return V * (f - np.concatenate([fprev0, f[:, :-1]], axis=1))
    v = apply_A(T, True) * (1.0 / 24.0)
    z = 4.0 * v + apply_A(v, False)
    z = 12.0 * v + apply_A(z, False)
    return (T + 24.0 * v) + apply_A(z, False)


def fma(a, b, c):
    return np.asarray(LD(a) * LD(b) + LD(c), dtype=np.float64)


def coefficient_form(w):
    """rk4_horner_pq over apply_PQ: P and Q rounded once, y_j = fma(-Q_j, g_{j-1}, fma(P_j, g_j, base_j))."""
    U, V, T = w["U"], w["V"], w["T"]
    hF, hB, qF, qB = (w[k][:, None] for k in ("hF", "hB", "qF", "qB"))
    zero = np.zeros_like(T[:, :1])
    P = V * np.concatenate([U, hB], axis=1)
    Q = V * np.concatenate([hF, U], axis=1)
    src = np.zeros_like(T)
    src[:, :1] = V[:, :1] * qF
    src[:, -1:] = src[:, -1:] + V[:, -1:] * qB                     # (node 0 is first and last node of a one-node tail only)

    def apply_PQ(x, base):
        g = np.concatenate([x[:, 1:], zero], axis=1) - x
        gprev = np.concatenate([x[:, :1] - zero, g[:, :-1]], axis=1)
        return fma(-Q, gprev, fma(P, g, base))
    v = apply_PQ(T, src) * (1.0 / 24.0)
    z = apply_PQ(v, 4.0 * v)
    z = apply_PQ(z, 12.0 * v)
    return apply_PQ(z, fma(24.0, v, T))


def test_extended_precision_is_wider_than_f64():
    assert np.finfo(LD).eps < 1e-18, "the reference of this file needs a long double wider than f64"


def test_both_forms_are_the_literal_stages_on_a_plain_wall():
    """The restatements themselves: on benign walls both forms sit within a few ulp of the literal stages."""
    for n in (2, 7, 32):
        rng = np.random.default_rng(n)
        B = 50
        w = dict(U=rng.uniform(1, 3, (B, n - 1)), V=rng.uniform(0.05, 0.15, (B, n)), T=rng.uniform(10, 30, (B, n)),
                 hF=rng.uniform(2, 8, B), hB=rng.uniform(2, 8, B), qF=rng.uniform(50, 300, B), qB=rng.uniform(50, 300, B))
        ref = literal_stages(w)
        for form in (flux_form, coefficient_form):
            err = float(np.max(np.abs(LD(form(w)) - ref)))
            assert err < 16 * np.spacing(30.0), (form.__name__, n, err)
        # and they are not the same computation: some bits differ
        assert not np.array_equal(flux_form(w), coefficient_form(w))


@pytest.mark.parametrize("n", SIZES)
def test_coefficient_form_is_no_worse_than_four_times_the_flux_form(n):
    w = walls(n, 9000 + n)
    ref = literal_stages(w)
    assert np.all(np.isfinite(np.asarray(ref, dtype=np.float64)))
    e_flux = np.max(np.abs(LD(flux_form(w)) - ref), axis=1).astype(np.float64)
    e_pq = np.max(np.abs(LD(coefficient_form(w)) - ref), axis=1).astype(np.float64)
    ulp = np.spacing(np.maximum(np.max(np.abs(w["T"]), axis=1), np.max(np.abs(ref), axis=1).astype(np.float64)))
    ratio = e_pq / (FACTOR * e_flux + FLOOR_ULP * ulp)
    i = int(np.argmax(ratio))
    print("n = %2d: worst error over %d walls — flux form %.3e K (%.1f ulp), coefficient form %.3e K (%.1f ulp); "
          "worst e_pq / (4 e_flux + 8 ulp) = %.3f (there: flux %.3e, coefficient %.3e); stiffest V (U_left + U_right) = %.2f" % (
              n, WALLS, e_flux.max(), (e_flux / ulp).max(), e_pq.max(), (e_pq / ulp).max(), ratio[i], e_flux[i], e_pq[i],
              float(np.max(w["V"][:, 1:-1] * (w["U"][:, :-1] + w["U"][:, 1:]))) if n > 2 else float("nan")))
    assert ratio[i] <= 1.0, (n, i, e_flux[i], e_pq[i], ulp[i])
