"""The no-mass loop in high precision, with its trace. For tests only.

Written from the text of SIMPLE-BuildingSimulation/heat v1.0.2 as tests/physics_ref.py is — `get_k_q`
(discretization.rs:596-700), `march_nomass` (surface.rs:790-898), the border conditions (surface.rs:596-717, 939-948),
the solar terms (surface.rs:916-931) — not from the device code and not from the CPU oracle, so that it can judge both.
Arithmetic is numpy ``longdouble`` (physics_ref.LD); the loop's decisions are taken on those numbers, and `margins`
says how far every decision was from its threshold, so that a case can be held clear of the ones f64 could take the
other way.

The loop (surface.rs:790-898), with `x` the pass's solve (K x = -q, mut_n_diag_gaussian), err = sum |x - T| over the
chunk's n nodes, old_err = 99999 and count = 0 at the start:

  exit  rule                                                       what the surface keeps
  A     err > old_err on the very first pass (err > 99999)         its temperatures unchanged
  B     err > old_err on a later pass (:842-848)                   the updates of the passes before, not this pass's
  C     err / n < 0.01 while count < 100 (:885-893)                the update of this pass included
  D     err / n < 0.5 once count >= 100                            as C
  E     err is NaN (:850)                                          the reference's error
"""
import numpy as np

import physics_ref as pr
from physics_ref import LD

MASS_THRESHOLD = 1e-5             # discretization.rs:149,155
OLD_ERR_0 = 99999.                # surface.rs:804
TIGHT, LOOSE, N_TIGHT = 0.01, 0.5, 100   # surface.rs:885
MAX_PASSES = 100000               # (a guard of this file's, never reached by a case: the loose rule ends every bounded orbit)


def chunks(mass):
    """(massive, no-mass) chunks [(ini, fin), ...] of a wall, discretization.rs:117-160."""
    out = ([], [])
    n = len(mass)
    i = 0
    while i < n:
        light = mass[i] < MASS_THRESHOLD
        j = i
        while j < n and (mass[j] < MASS_THRESHOLD) == light:
            j += 1
        out[1 if light else 0].append((i, j))
        i = j
    return out


def _u_value(wall, g, t_before, t_after, F):
    """UValue::u_value, discretization.rs:48-55: Solid(u) -> u, Cavity(c) -> c.u_value(t_before, t_after), Back -> 0."""
    sc = wall.get("seg_cavity")
    if sc is not None and sc[g] >= 0:
        return pr.cavity_u_value(wall["cavities"][sc[g]], t_before, t_after, F)
    return F.num(wall["uvalue"][g])


def get_k_q(wall, ini, fin, T, front, back, F=LD):
    """Discretization::get_k_q (discretization.rs:596-700) for the chunk (ini, fin): the three diagonals of K and q.
    ``wall``: uvalue, and seg_cavity / cavities where it has gas layers; ``T``: the whole wall's temperatures (field
    numbers); ``front`` / ``back``: air_t, rad_t, hs, rad_hs. Interior segments first (:634-655), then the front term
    (:658-677), then the back term (:680-697); a chunk that does not touch a face takes its massive neighbour's
    conductance and temperature."""
    nrows = len(T)
    n = fin - ini
    zero = F.num(0.0)
    lo, dg, up, q = [zero] * n, [zero] * n, [zero] * n, [zero] * n
    for li in range(n - 1):
        gi = ini + li
        t_next = T[gi + 1] if gi + 1 < nrows else F.num(back["air_t"])          # get_t_after :627-632
        u = _u_value(wall, gi, T[gi], t_next, F)
        dg[li] = dg[li] - u
        dg[li + 1] = dg[li + 1] - u
        up[li] = up[li] + u
        lo[li + 1] = lo[li + 1] + u
    if ini == 0:
        front_q = F.num(front["air_t"]) * F.num(front["hs"]) + F.num(front["rad_hs"]) * (F.num(front["rad_t"]) - T[0])
        hs_front = F.num(front["hs"])
    else:
        u = _u_value(wall, ini - 1, T[ini - 1], T[ini], F)
        hs_front = u
        front_q = u * T[ini - 1]
    q[0] = q[0] + front_q
    dg[0] = dg[0] - hs_front
    if fin == nrows:
        back_q = F.num(back["air_t"]) * F.num(back["hs"]) + F.num(back["rad_hs"]) * (F.num(back["rad_t"]) - T[fin - 1])
        hs_back = F.num(back["hs"])
    else:
        u = _u_value(wall, fin - 1, T[fin - 1], T[fin], F)
        hs_back = u
        back_q = u * T[fin]
    q[n - 1] = q[n - 1] + back_q
    dg[n - 1] = dg[n - 1] - hs_back
    return lo, dg, up, q


def _solve(lo, dg, up, rhs):
    """mut_n_diag_gaussian(rhs, 3), call site surface.rs:834: elimination without pivoting, back-substitution."""
    n = len(rhs)
    dg, rhs = list(dg), list(rhs)
    for i in range(1, n):
        f = lo[i] / dg[i - 1]
        dg[i] = dg[i] - f * up[i - 1]
        rhs[i] = rhs[i] - f * rhs[i - 1]
    x = [None] * n
    x[n - 1] = rhs[n - 1] / dg[n - 1]
    for i in range(n - 2, -1, -1):
        x[i] = (rhs[i] - up[i] * x[i + 1]) / dg[i]
    return x


class ChunkResult:
    """ini, fin; exit ('A'..'E'); count (the loop's counter when it left); trace (err of every pass, as floats of the
    field numbers in trace_ld); and, where asked for, earlier / later: the chunk's temperatures had the loop stopped one
    pass earlier (None where no pass came before) or gone one pass further."""

    def __repr__(self):
        return "<chunk (%d, %d) exit %s count %d passes %d>" % (self.ini, self.fin, self.exit, self.count, len(self.trace))


def _pass(wall, ini, fin, T, front, back, solar, F):
    lo, dg, up, q = get_k_q(wall, ini, fin, T, front, back, F)
    q = [(q[i] + F.num(solar[ini + i])) * F.num(-1.) for i in range(fin - ini)]      # surface.rs:828-832
    x = _solve(lo, dg, up, q)
    err = F.num(0.0)
    for i in range(fin - ini):
        err = err + abs(x[i] - T[ini + i])                                          # :836-841
    return x, err


def _updated(T, ini, fin, x, F):
    T = list(T)
    for i in range(fin - ini):
        T[ini + i] = (T[ini + i] + x[i]) * F.num(0.5)                               # :878-883
    return T


def march_chunk(wall, ini, fin, T, front, back, solar, neighbours=False, F=LD):
    """march_nomass (surface.rs:790-898) on the chunk (ini, fin). Returns (new T of the whole wall, ChunkResult)."""
    n = fin - ini
    old_err = F.num(OLD_ERR_0)
    count = 0
    r = ChunkResult()
    r.ini, r.fin, r.trace_ld = ini, fin, []
    T = list(T)
    T_prev = None                                      # the wall before the last update that was applied
    while True:
        x, err = _pass(wall, ini, fin, T, front, back, solar, F)
        r.trace_ld.append(err)
        if err > old_err:                              # :842-848
            r.exit = "A" if count == 0 else "B"
            earlier, later = T_prev, _updated(T, ini, fin, x, F)
            break
        if err != err:                                 # :850
            r.exit = "E"
            earlier, later = T_prev, None
            break
        T_prev, T = T, _updated(T, ini, fin, x, F)
        tol = F.num(TIGHT) if count < N_TIGHT else F.num(LOOSE)                     # :885
        if err / F.num(n) < tol:                       # :887-893
            r.exit = "C" if count < N_TIGHT else "D"
            earlier = T_prev
            later = None
            if neighbours:
                x2, _ = _pass(wall, ini, fin, T, front, back, solar, F)
                later = _updated(T, ini, fin, x2, F)
            break
        old_err = err
        count += 1
        assert count < MAX_PASSES, "the loop does not end"
    r.count = count
    r.n = n
    r.trace = [float(e) for e in r.trace_ld]
    if neighbours:
        r.earlier = None if earlier is None else earlier[ini:fin]
        r.later = None if later is None else later[ini:fin]
    return T, r


def margins(res):
    """The smallest relative distance of any decision of any pass of the chunk from its threshold: err against old_err
    (|err / old_err - 1|), and, where the pass got that far, err / n against 0.01 or 0.5. A NaN err decides nothing by
    a margin (both comparisons are false whatever the rounding): such a pass does not count."""
    worst = np.inf
    old = LD.num(OLD_ERR_0)
    count = 0
    for k, err in enumerate(res.trace_ld):
        if err != err:
            break
        worst = min(worst, float(abs(err / old - LD.num(1.))))
        if err > old:
            break
        tol = LD.num(TIGHT) if count < N_TIGHT else LD.num(LOOSE)
        worst = min(worst, float(abs(err / LD.num(res.n) / tol - LD.num(1.))))
        old = err
        count += 1
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# A surface of a model dict
def solar_per_node(md, state, s, F=LD):
    """surface.rs:916-931: the clamps (the second one tests solar_front — as the reference has it) and the per-node sums."""
    off = int(md["node_offset"][s])
    n = int(md["node_offset"][s + 1]) - off
    sf = float(state[md["solar_front_slot"][s]])
    sb = float(state[md["solar_back_slot"][s]])
    if sf != sf or sf < 0.0:
        sf = 0.0
    if sb != sb or sf < 0.0:
        sb = 0.0
    return [F.num(md["front_alpha"][off + i]) * F.num(sf) + F.num(md["back_alpha"][off + i]) * F.num(sb) for i in range(n)]


def border_conditions(md, state, s, wind_direction, wind_speed, t_out, F=LD):
    """calc_border_conditions (surface.rs:596-717) and the radiative coefficients frozen over the loop (:939-948), from
    physics_ref's side_hs / rad_temperature / rad_hs, or from the debug overrides (:708-714; a NaN override is none).
    Returns (front, back): air_t, rad_t, hs, rad_hs."""
    first = int(md["first_node_slot"][s])
    n = int(md["node_offset"][s + 1] - md["node_offset"][s])
    t_first, t_last = float(state[first]), float(state[first + n - 1])
    cos_tilt = float(md["cos_tilt"][s])
    windward = pr.is_windward(wind_direction, cos_tilt, float(md["normal_x"][s]), float(md["normal_y"][s]))
    zone_t = lambda z: float(state[md["zone_slot"][z]])
    sides = []
    t_front = None
    for is_front in (True, False):
        sd = "front" if is_front else "back"
        kind = int(md[sd + "_kind"][s])
        ambient = float(md[sd + "_ambient"][s])
        t_b = {pr.SPACE: lambda: zone_t(int(md[sd + "_zone"][s])), pr.AMBIENT: lambda: ambient,
               pr.OUTDOOR: lambda: float(t_out)}[kind]()                             # model.rs:79-96
        if is_front:
            t_front = t_b
        if kind == pr.SPACE:
            air_t, rad_t, surf_t = t_b, F.num(t_b), t_first if is_front else t_last
        elif kind == pr.AMBIENT:                       # (:672-686: a back of this kind takes t_front and the FRONT node)
            air_t, rad_t, surf_t = ambient, F.num(t_front), t_first
        else:
            air_t, surf_t = t_b, t_first if is_front else t_last
            rad_t = pr.rad_temperature(float(state[md["ir_%s_slot" % sd][s]]), F)
        fix = md.get(sd + "_hs_fix")
        if fix is not None and fix[s] == fix[s]:
            hs = F.num(fix[s])
        else:
            hs = pr.side_hs(kind, is_front, t_b, ambient, t_first, t_last, cos_tilt, wind_speed,
                            float(md["wind_modifier"][s]), float(md["area"][s]), float(md["perimeter"][s]), windward, F)
        emis = float(md[sd + "_emissivity"][s])
        sides.append(dict(air_t=F.num(air_t), rad_t=rad_t, hs=hs, rad_hs=pr.rad_hs(emis, rad_t, surf_t, F)))
    return sides[0], sides[1]


def wall_of(md, s):
    off, end = int(md["node_offset"][s]), int(md["node_offset"][s + 1])
    wall = dict(mass=np.asarray(md["mass"])[off:end], uvalue=np.asarray(md["uvalue"])[off:end])
    if md.get("seg_cavity") is not None and md.get("cavities") is not None and len(md["cavities"]):
        wall["seg_cavity"] = np.asarray(md["seg_cavity"])[off:end]
        wall["cavities"] = md["cavities"]
    return wall


class SurfaceResult:
    """T: the wall's temperatures after all its no-mass chunks (field numbers; massive nodes as they came);
    chunks: a ChunkResult per no-mass chunk, in the order the reference marches them; passes: their sum; nomass: the
    indices of the no-mass nodes."""


def march_surface(md, state, s, wind_direction, wind_speed, t_out, neighbours=False, F=LD):
    """The no-mass part of ThermalSurfaceData::march (surface.rs:902-965) for surface s of a model dict on `state`."""
    wall = wall_of(md, s)
    first = int(md["first_node_slot"][s])
    n = len(wall["mass"])
    T = [F.num(state[first + i]) for i in range(n)]
    front, back = border_conditions(md, state, s, wind_direction, wind_speed, t_out, F)
    solar = solar_per_node(md, state, s, F)
    r = SurfaceResult()
    r.chunks = []
    for ini, fin in chunks(wall["mass"])[1]:
        T, c = march_chunk(wall, ini, fin, T, front, back, solar, neighbours, F)
        r.chunks.append(c)
        if c.exit == "E":
            break
    r.T = T
    r.passes = sum(len(c.trace) for c in r.chunks)
    r.nomass = [i for c in r.chunks for i in range(c.ini, c.fin)]
    r.front, r.back = front, back
    return r


# ---------------------------------------------------------------------------------------------------------------------
# The closed form of a one-node chunk
class OneNode:
    """A one-node chunk with constant neighbours: K = -(h + u) with h, u the conductances to its two sides (a face's hs or
    a segment's U), q = c - r T with r the face's rad_hs (0 inside the wall). Then x(T) = (c - r T) / (h + u), the
    undamped map has slope g = -r / (h + u), the damped one lambda = (1 + g) / 2, the fixed point is
    T* = c / (h + u + r), T_k = T* + (T_0 - T*) lambda^k and err_k = |1 - g| |T_0 - T*| |lambda|^k."""

    def __init__(self, h, u, r, c, F=LD):
        self.F = F
        self.g = -F.num(r) / (F.num(h) + F.num(u))
        self.lam = (F.num(1.) + self.g) / F.num(2.)
        self.t_star = F.num(c) / (F.num(h) + F.num(u) + F.num(r))

    def err(self, t0, k):
        return abs(self.F.num(1.) - self.g) * abs(self.F.num(t0) - self.t_star) * abs(self.lam) ** k

    def temperature(self, t0, k):
        return self.t_star + (self.F.num(t0) - self.t_star) * self.lam ** k

    def outcome(self, t0):
        """(exit, count, T kept) as the rules of the loop give them on err_k, without running the loop."""
        e0 = self.err(t0, 0)
        if e0 != e0:
            return "E", 0, None
        if e0 > OLD_ERR_0:
            return "A", 0, self.F.num(t0)
        k = 0
        while True:
            e = self.err(t0, k)
            if k > 0 and e > self.err(t0, k - 1):
                return "B", k, self.temperature(t0, k)
            if e < (TIGHT if k < N_TIGHT else LOOSE):
                return ("C" if k < N_TIGHT else "D"), k, self.temperature(t0, k + 1)
            k += 1
            assert k < MAX_PASSES


def one_node_form(wall, ini, T, front, back, solar, F=LD):
    """The OneNode of the chunk (ini, ini + 1) of a wall without cavities beside the chunk."""
    n = len(T)
    h = u = r = c = F.num(0.0)
    if ini == 0:
        h, r = F.num(front["hs"]), F.num(front["rad_hs"])
        c = c + F.num(front["air_t"]) * h + r * F.num(front["rad_t"])
    else:
        h = F.num(wall["uvalue"][ini - 1])
        c = c + h * T[ini - 1]
    if ini + 1 == n:
        u, rb = F.num(back["hs"]), F.num(back["rad_hs"])
        c = c + F.num(back["air_t"]) * u + rb * F.num(back["rad_t"])
        r = r + rb
    else:
        u = F.num(wall["uvalue"][ini])
        c = c + u * T[ini + 1]
    return OneNode(h, u, r, c + F.num(solar[ini]), F)
