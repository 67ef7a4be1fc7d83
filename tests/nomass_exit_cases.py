"""Cases that drive the no-mass loop (march_nomass, surface.rs:790-898) through every one of its exits, shared by
tests/test_nomass_exits_host.py and tests/test_nomass_exits_gpu.py. Importable without a GPU. tests/nomass_ref.py names
the exits A to E.

Every wall comes from the oracle's restatement of the reference's discretization (oracle.discretize, a 180 s model step
with max_dx = 0.04 and min_dt = 60, marched at 45 s as tests/test_parity_gpu.py marches such walls), with emissivity 0.9
on both sides. A family is one kind of wall — one copy of the loop in kernels.hip — in 256 surfaces at most, between the
zones of two clusters, an AmbientTemperature front on every eighth. Within a family the surfaces differ by

* both hs overrides (surface.rs:708-714), 64 values log-spaced from the family's lowest to 3 W/m2K, so that
  neighbouring lanes of one tile leave the loop at different passes;
* overrides solved for a chosen contraction factor lambda of the chunk's damped map (nomass_ref.OneNode gives it in
  closed form for one node; for more nodes it is the dominant eigenvalue of (I + K^-1 R) / 2, R the radiative
  coefficients on the diagonal) together with a first error per node chosen so that the rules of the loop give C at a
  count of 20 to 99, D at exactly 100 and D beyond it;
* the initial distance from the fixed point (C at the first pass for the smallest);
* a solar irradiance of 3e6 W/m2 on the face of the chunk (exit A);
* an override on one side only (a NaN override is none).

The lowest override of a family is the one at which lambda = -LAMBDA_MOST (or 0.1 W/m2K where that is lower), and the
distance from the fixed point shrinks with |lambda|^3 beyond |lambda| = 1.5: three sub-timesteps then keep the
reference's temperatures within -100 ... 200 C (tests/test_nomass_exits_host.py asserts it).
"""
import functools
import math

import numpy as np

import nomass_ref as nr
from heat_amd import modeldict as mdl
from oracle import oracle as orc

DT = 45.0
EMIS = 0.9
ZONE_T = [20.0, 21.0, 23.0, 24.0]           # zones 0-1 are one cluster, 2-3 the other
AMBIENT_T = 19.0
LAMBDA_MOST = 3.0
WEATHER = mdl.weather_series(3, DT, wind_speed=0.0)      # no wind
N_SUB = (1, 3)

POLY = dict(thickness=0.02, k=0.0252, rho=17.5, cp=2400.)
WOOL = dict(thickness=0.05, k=0.04, rho=30., cp=1000.)
BRICK = dict(thickness=0.1, k=0.6, rho=1600., cp=840.)
GLASS = dict(thickness=0.003, k=1.0, rho=2500., cp=840.)
GAP = dict(thickness=0.0127, is_gas=True, gas=orc.AIR)


def conc(thickness):
    return dict(thickness=thickness, k=0.816, rho=1700., cp=800.)


# family -> [(layers, nodes the discretization must give)], and the class of class_counts() it must run in
# (0-2: the register kernel at 4 / 8 / 16 nodes per lane, 3: small_step, 4: k_surfaces_general)
FAMILIES = {
    "panel2": ([([POLY], 2)], "small"),
    "panel4": ([([POLY, WOOL, POLY], 4), ([POLY, WOOL], 3)], "small"),
    "glazing": ([([GLASS, GAP, GLASS], 4), ([GLASS, dict(GAP, gas=orc.ARGON, thickness=0.02), GLASS], 4)], "small"),
    "facing_front": ([([POLY, conc(0.07)], 8), ([POLY, conc(0.2)], 20), ([POLY, conc(0.35)], 33)], "fast"),
    "facing_back": ([([conc(0.07), POLY], 8), ([conc(0.2), POLY], 20), ([conc(0.35), POLY], 33)], "fast"),
    "facing_both": ([([POLY, conc(0.06), POLY], 8), ([POLY, conc(0.195), POLY], 20), ([POLY, conc(0.34), POLY], 33)], "fast"),
    "chunk2_front": ([([POLY, WOOL, conc(0.2)], 21), ([POLY, WOOL, conc(0.2), WOOL, POLY], 23),
                      ([BRICK, WOOL, POLY, BRICK], 23)], "fast"),
    "chunk2_back": ([([conc(0.2), WOOL, POLY], 21), ([POLY, WOOL, conc(0.2), WOOL, POLY], 23),
                     ([BRICK, WOOL, POLY, BRICK], 23)], "fast"),
    "long_run": ([([POLY, WOOL, POLY, WOOL], 5)], "general"),
}
STILL_AIR = ("panel2", "panel4", "glazing")       # the families of still_air: the same walls without overrides
COMPANIONS = 16                                    # massive walls beside the small surfaces of a family, in the same clusters
N_GRID = 64


@functools.lru_cache(maxsize=None)
def segments(family):
    out = []
    for layers, n in FAMILIES[family][0]:
        d = orc.discretize(layers, 180., 0.04, 60., 1., math.pi / 2)
        assert d["tstep_subdivision"] == 2 and d["n_nodes"] == n, (family, d["n_nodes"], n, d["tstep_subdivision"])
        out.append(d)
    return out


def assemble(walls, kinds_front):
    """One model dict of the walls (discretization dicts), surface i between zones 2c and 2c + 1 of cluster c = i % 2."""
    S = len(walls)
    md = mdl.empty(S, len(ZONE_T), DT)
    n = np.array([len(w["mass"]) for w in walls], dtype=np.int64)
    md["node_offset"] = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    for k in ("mass", "uvalue", "front_alpha", "back_alpha"):
        md[k] = np.concatenate([np.asarray(w[k], dtype=np.float64) for w in walls])
    if any(len(w["cavities"]) for w in walls):
        segc, cavs, base = [], [], 0
        for w in walls:
            sc = np.asarray(w["seg_cavity"], dtype=np.int32)
            segc.append(np.where(sc >= 0, sc + base, -1).astype(np.int32))
            cavs.append(np.asarray(w["cavities"], dtype=mdl.CAVITY_DTYPE))
            base += len(w["cavities"])
        md["seg_cavity"] = np.concatenate(segc)
        md["cavities"] = np.concatenate(cavs)
    i = np.arange(S)
    md["front_kind"] = np.asarray(kinds_front, dtype=np.int32)
    md["back_kind"] = np.full(S, mdl.SPACE, dtype=np.int32)
    md["front_zone"] = (2 * (i % 2)).astype(np.int32)
    md["back_zone"] = (2 * (i % 2) + 1).astype(np.int32)
    md["front_ambient"] = np.full(S, AMBIENT_T)
    md["back_ambient"] = np.zeros(S)
    md["front_emissivity"] = np.full(S, EMIS)
    md["back_emissivity"] = np.full(S, EMIS)
    md["area"] = np.full(S, 4.0)
    md["perimeter"] = np.full(S, 8.0)
    md["cos_tilt"] = np.zeros(S)
    md["normal_x"] = np.ones(S)
    md["normal_y"] = np.zeros(S)
    md["wind_modifier"] = np.full(S, mdl.wind_speed_modifier(3.0))
    md["front_hs_fix"] = np.full(S, np.nan)
    md["back_hs_fix"] = np.full(S, np.nan)
    md["zone_volume"] = np.full(len(ZONE_T), 300.0)
    st = mdl.layout_state(md)
    st[md["zone_slot"]] = ZONE_T
    mdl.set_ir_from_air(md, st, float(WEATHER[0, 0]))
    return md, st


# ---------------------------------------------------------------------------------------------------------------------
# The damped map of a chunk, linearised where it stands (f64: this places inputs, it judges nothing)
def face_chunks(md, s):
    n = int(md["node_offset"][s + 1] - md["node_offset"][s])
    off = int(md["node_offset"][s])
    return [(i, f) for i, f in nr.chunks(np.asarray(md["mass"])[off:off + n])[1] if i == 0 or f == n]


def linear_map(md, st, s, ini, fin):
    """(lambda, v, T*, g) of the chunk's damped map at the state: the eigenvalue of largest modulus of (I + K^-1 R) / 2,
    its eigenvector scaled to an L1 norm of n, the fixed point, and the eigenvalue g = 2 lambda - 1 of K^-1 R."""
    wall = nr.wall_of(md, s)
    first = int(md["first_node_slot"][s])
    nn = len(wall["mass"])
    T = [nr.LD.num(st[first + i]) for i in range(nn)]
    front, back = nr.border_conditions(md, st, s, float(WEATHER[0, 1]), float(WEATHER[0, 2]), float(WEATHER[0, 0]))
    solar = nr.solar_per_node(md, st, s)
    lo, dg, up, q = nr.get_k_q(wall, ini, fin, T, front, back)
    n = fin - ini
    K = np.zeros((n, n))
    for i in range(n):
        K[i, i] = float(dg[i])
        if i + 1 < n:
            K[i, i + 1] = float(up[i])
            K[i + 1, i] = float(lo[i + 1])
    R = np.zeros(n)
    if ini == 0:
        R[0] += float(front["rad_hs"])
    if fin == nn:
        R[n - 1] += float(back["rad_hs"])
    Tc = np.array([float(t) for t in T[ini:fin]])
    c = np.array([float(x) for x in q]) + R * Tc + np.array([float(x) for x in solar[ini:fin]])
    t_star = np.linalg.solve(K - np.diag(R), -c)
    ev, vec = np.linalg.eig(np.linalg.solve(K, np.diag(R)))
    k = int(np.argmax(np.abs((1.0 + ev.real) / 2.0)))
    g = float(ev.real[k])
    v = vec[:, k].real
    v = v / np.abs(v).sum() * n
    return (1.0 + g) / 2.0, v, t_star, g


def _set_hs(md, s, side, h):
    for sd in ("front", "back"):
        if side in (sd, "both"):
            md[sd + "_hs_fix"][s] = h


def solve_hs(md, st, s, ini, fin, side, lam):
    """The override (on `side`) at which the chunk's lambda is `lam`: lambda rises with hs."""
    lo, hi = 1e-3, 1e3
    for _ in range(60):
        mid = math.sqrt(lo * hi)
        _set_hs(md, s, side, mid)
        if linear_map(md, st, s, ini, fin)[0] < lam:
            lo = mid
        else:
            hi = mid
    return math.sqrt(lo * hi)


def place(md, st, s, spec, rng):
    """Writes surface s's overrides and initial temperatures for `spec`:
    hs: the override, or lam: the contraction factor to solve the override for; sides: which overrides are set;
    err0: the first pass's error per node; solar: irradiance on the chunk's face."""
    n = int(md["node_offset"][s + 1] - md["node_offset"][s])
    first = int(md["first_node_slot"][s])
    tf = AMBIENT_T if md["front_kind"][s] == mdl.AMBIENT else ZONE_T[md["front_zone"][s]]
    tb = ZONE_T[md["back_zone"][s]]
    st[first:first + n] = np.linspace(tf, tb, n) + rng.uniform(-0.4, 0.4, n)
    sides = spec.get("sides", "both")
    if "profile" in spec:                         # off the dominant mode: the line between two faces further apart than their airs
        _set_hs(md, s, "both", spec["hs"])
        st[first:first + n] = np.linspace(tf - spec["profile"], tb + spec["profile"], n)
        return
    if sides != "both":
        _set_hs(md, s, sides, spec["hs"])         # the one override, whether that side's node carries mass or not
    for ini, fin in face_chunks(md, s):
        side = "both" if (ini == 0 and fin == n) else ("front" if ini == 0 else "back")
        if sides != "both" and side != "both" and side != sides:
            continue                              # the chunk at the side left alone: free convection, where it stands
        mine = side if sides == "both" else sides
        if spec.get("solar"):
            st[md["solar_front_slot" if ini == 0 else "solar_back_slot"][s]] = spec["solar"]
        for _ in range(4):                        # (rad_hs is frozen at the face's temperature, which moves with T0)
            if "lam" in spec:
                _set_hs(md, s, mine, solve_hs(md, st, s, ini, fin, mine, spec["lam"]))
            else:
                _set_hs(md, s, mine, spec["hs"])
            if spec.get("solar"):
                break
            lam, v, t_star, g = linear_map(md, st, s, ini, fin)
            e0 = spec["err0"] / abs(1.0 - g)
            if abs(lam) > 1.5:
                e0 = max(e0 / abs(lam) ** 3, 0.03 / abs(1.0 - g))
            st[first + ini:first + fin] = t_star + e0 * v * spec.get("sign", 1.0)


def specs_of(family, lowest):
    grid = np.geomspace(lowest, 3.0, N_GRID)
    specs = [dict(hs=float(h), err0=1.5 * (1.0 + 0.37 * (i % 5)), sign=(-1.0) ** i) for i, h in enumerate(grid)]
    for lam, err0 in ((-0.99, 0.05), (-0.99, 0.1), (-0.995, 0.03), (-0.98, 0.06),      # D at exactly 100
                      (-0.99, 2.0), (-0.995, 1.2), (-0.98, 4.0), (-0.97, 15.0),       # D beyond 100
                      (-0.97, 0.1), (-0.9, 1.0), (-0.95, 0.5), (-0.8, 3.0), (-0.93, 0.2), (-0.96, 0.4)):   # C at 20..99
        for sign in (1.0, -1.0):
            specs.append(dict(lam=lam, err0=err0, sign=sign))
    for h in (0.3, 0.9, 1.6, 2.7, 1.2, 2.0):                                          # C at the first pass
        specs.append(dict(hs=h, err0=0.004))
    for h in (0.5, 1.3, 2.2, 2.9):                                                    # A
        specs.append(dict(hs=h, err0=1.0, solar=3e6))
    for k, h in enumerate((0.4, 0.8, 1.5, 2.5, 0.6, 1.1, 1.9, 2.8)):                  # one side overridden only
        specs.append(dict(hs=h, err0=1.0 + 0.5 * k, sides="front" if k % 2 == 0 else "back"))
    for h, p in ((0.9, 0.43), (1.0, 0.43), (1.1, 0.3), (1.0, 0.35)):                  # far from the dominant mode (B after several passes
        specs.append(dict(hs=h, profile=p))                                           # where a gas cavity bends the map)
    return specs


class Case:
    """md, st: the family's model and initial state (read-only); family; n_own: its own surfaces come first, the massive
    companions of a small family after them; ref[s]: nomass_ref.march_surface of the first sub-timestep (neighbours
    included) of every surface with a no-mass chunk; exit_of[s]: the exit its grouping goes by."""


def _exit_of(res):
    """The exit a surface is filed under: that of its first chunk other than a plain early C, else of its first chunk."""
    for c in res.chunks:
        if not (c.exit == "C" and c.count < 20):
            return c.exit + ("0" if c.exit == "C" and c.count == 0 else "")
    return "C"


@functools.lru_cache(maxsize=None)
def case(family):
    still = family.startswith("still_air")
    base = family.split(":")[1] if still else family
    segs = segments(base)
    rng = np.random.default_rng(sum(map(ord, family)))
    small = FAMILIES[base][1] != "fast"
    if still:
        n_own = 96
        specs = [None] * n_own
    else:
        probe_md, probe_st = assemble([segs[0]], [mdl.SPACE])
        ini, fin = face_chunks(probe_md, 0)[0]
        side = "both" if fin - ini == len(segs[0]["mass"]) else ("front" if ini == 0 else "back")
        lowest = max(0.1, solve_hs(probe_md, probe_st, 0, ini, fin, side, -LAMBDA_MOST))
        specs = specs_of(base, lowest)
        n_own = len(specs)
    walls = [segs[i % len(segs)] for i in range(n_own)]
    kinds = [mdl.AMBIENT if i % 8 == 5 else mdl.SPACE for i in range(n_own)]
    n_comp = COMPANIONS if small else 0
    if n_comp:
        comp = orc.discretize([conc(0.07)], 180., 0.04, 60., 1., math.pi / 2)
        walls += [comp] * n_comp
        kinds += [mdl.SPACE] * n_comp
    md, st = assemble(walls, kinds)
    assert md["n_surfaces"] <= 256
    for s in range(n_own, n_own + n_comp):
        first, n = int(md["first_node_slot"][s]), len(comp["mass"])
        st[first:first + n] = np.linspace(ZONE_T[md["front_zone"][s]], ZONE_T[md["back_zone"][s]], n) + rng.uniform(-0.4, 0.4, n)
    if still:
        md["front_hs_fix"] = None
        md["back_hs_fix"] = None
        for s in range(n_own):
            # faces 0.05 ... 0.5 K off their air, on both sides; the nodes between on the line between the faces
            first, n = int(md["first_node_slot"][s]), len(walls[s]["mass"])
            tf = AMBIENT_T if md["front_kind"][s] == mdl.AMBIENT else ZONE_T[md["front_zone"][s]]
            tb = ZONE_T[md["back_zone"][s]]
            d = np.geomspace(0.2 if base == "glazing" else 0.05, 0.5, n_own)[s] * np.array([(-1.0) ** s, (-1.0) ** (s // 2)])
            st[first:first + n] = np.linspace(tf + d[0], tb + d[1], n)
    else:
        for s, spec in enumerate(specs):
            place(md, st, s, spec, rng)
    c = Case()
    c.family, c.md, c.n_own, c.specs = family, md, n_own, specs
    st.setflags(write=False)
    c.st = st
    w = WEATHER[0]
    c.ref = [nr.march_surface(md, st, s, float(w[1]), float(w[2]), float(w[0]), neighbours=True) for s in range(n_own)]
    c.exit_of = [_exit_of(r) for r in c.ref]
    return c


CASES = sorted(FAMILIES) + ["still_air:" + f for f in STILL_AIR]


# ---------------------------------------------------------------------------------------------------------------------
# The two orders
def grouped(c):
    """{exit: surfaces}: one batch per exit (every batch with the family's companions, so that its clusters keep walls)."""
    comp = list(range(c.n_own, int(c.md["n_surfaces"])))
    out = {}
    for s, e in enumerate(c.exit_of):
        out.setdefault(e, []).append(s)
    return {e: np.array(idx + comp, dtype=np.int64) for e, idx in sorted(out.items())}


def interleaved(c):
    """All surfaces, the exits dealt out in turn: every tile of 64 lanes mixes all of them."""
    keyed = []
    for g, v in enumerate(grouped(c).values()):
        own = [s for s in v if s < c.n_own]
        keyed += [((r + 0.5) / len(own), g, s) for r, s in enumerate(own)]      # every group spread over the whole order
    order = [s for _, _, s in sorted(keyed)]
    return np.array(order + list(range(c.n_own, int(c.md["n_surfaces"]))), dtype=np.int64)


def batches(c):
    """[(name, surfaces)]: the interleaved order and the batches of the grouped one."""
    return [("interleaved", interleaved(c))] + [("exit " + e, idx) for e, idx in grouped(c).items()]


def with_nan_irradiance(c, s):
    """The case's model with surface s turned to an Outdoor front under a NaN long-wave irradiance (exit E): (md, st)."""
    md, st = dict(c.md), c.st.copy()
    md["front_kind"] = np.array(md["front_kind"])
    md["front_kind"][s] = mdl.OUTDOOR
    st[md["ir_front_slot"][s]] = np.nan
    return md, st


E_FAMILIES = ["panel2", "facing_front", "chunk2_front", "long_run"]


def damaged(family):
    """The family's model with one surface of cluster 0 — a plain convergent one from the middle of the family, with a
    no-mass chunk at its front face — turned to an Outdoor front: (md, healthy state, state with a NaN long-wave
    irradiance on that front, the surface). The healthy state is the undamaged run of the same model, hence of the same plan."""
    c = case(family)
    cand = [s for s in range(c.n_own) if s % 2 == 0 and c.exit_of[s] == "C" and c.md["front_kind"][s] == mdl.SPACE
            and c.ref[s].chunks[0].ini == 0]
    s = cand[len(cand) // 2]
    md, bad = with_nan_irradiance(c, s)
    healthy = bad.copy()
    healthy[md["ir_front_slot"][s]] = c.st[c.md["ir_front_slot"][s]]
    return md, healthy, bad, s
