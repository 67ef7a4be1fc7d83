"""Shared builders for tests: single-surface model dicts in the shape of the reference's unit tests."""
import math
import os
import subprocess

import numpy as np

from heat_amd import build as heat_build, modeldict as mdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host_main(tmp_path, stem):
    """tests/<stem>.cpp — a stand-alone program with its own main — compiled together with the library's host-only sources
    (heat_amd.build.HOST_SOURCES) under AddressSanitizer / UBSan, the sanitizers' runtimes linked in. Returns the executable."""
    exe = tmp_path / stem
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", stem + ".cpp")] + [os.path.join(heat_build.CSRC, s) for s in heat_build.HOST_SOURCES] +
                          ["-o", str(exe)])
    return exe


# ---------------------------------------------------------------------------------------------------------------------
# The workgroup lists of a plan (tests/plan_lists_shim.cpp): which instantiation of the resident march a batch reaches
N_FAST = 18                                 # plan.hpp, kNumFast
FAST_M = [4] * 6 + [8] * 6 + [16] * 6        # plan.cpp, kFastM
FAST_NM = [0, 0, 0, 1, 1, 1] * 3            # plan.cpp, kFastNM
_plan_lists_lib = []


def plan_lists_library():
    """tests/plan_lists_shim.cpp and the planner (heat_amd.build.HOST_SOURCES), compiled once per process by g++ into a
    temporary directory — no sanitizer, nothing preloaded — and loaded with ctypes."""
    if not _plan_lists_lib:
        import atexit
        import ctypes as C
        import tempfile
        from heat_amd import binding
        tmp = tempfile.TemporaryDirectory(prefix="plan_lists_")
        so = os.path.join(tmp.name, "libplan_lists.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", os.path.join(ROOT, "tests", "plan_lists_shim.cpp")] +
                              [os.path.join(heat_build.CSRC, s) for s in heat_build.HOST_SOURCES] + ["-o", so])
        L = C.CDLL(so)
        L.plan_lists.restype = C.c_int
        L.plan_lists.argtypes = [C.POINTER(binding.Desc), C.POINTER(binding.Options), C.POINTER(C.c_int64), C.c_int]
        atexit.register(tmp.cleanup)         # (the directory lives as long as the library is loaded)
        _plan_lists_lib.extend([L, tmp])
    return _plan_lists_lib[0]


def plan_lists(md, **opts):
    """The plan of a batch made from `md` with the options `opts` (binding.make_options), as heat::make_plan gives it:
      lists       {(class, list): workgroups} of the non-empty workgroup lists (Plan::fblocks)
      teams       team clusters over all classes;   stream_tiles   streamed fast tiles over all classes
      most_zones  the largest FusedBlock::n_zones;  reason         ideal_resident_reason (binding.IDEAL_RESIDENT_*)
      resident_cavity_tiles   small-surface tiles with a gas cavity that a resident workgroup marches
    Host-only; needs neither the product library nor a GPU."""
    import ctypes as C
    from heat_amd import binding
    L = plan_lists_library()
    desc, keep = binding.make_desc(md)
    opt = binding.make_options(**opts)
    out = (C.c_int64 * (N_FAST * 6 + 5))()
    rc = L.plan_lists(C.byref(desc), C.byref(opt), out, len(out))
    assert rc == 0, "make_plan returned %d" % rc
    out = list(out)
    n_small, n_plain, n_cav_streamed = out[N_FAST * 6 + 2:]
    return dict(lists={(c, g2): out[c * 4 + g2] for c in range(N_FAST) for g2 in range(4) if out[c * 4 + g2]},
                teams=sum(out[N_FAST * 4:N_FAST * 5]), stream_tiles=sum(out[N_FAST * 5:N_FAST * 6]), most_zones=out[N_FAST * 6],
                reason=out[N_FAST * 6 + 1], resident_cavity_tiles=n_small - n_plain - n_cav_streamed)


def instantiation_of(c, g2):
    """The IDEAL instantiation a workgroup list marches with (batch.hip, enqueue_fused; kernels.hip, launch_surfaces_fused):
    (M, "mixed" or "nm0" / "nm1", wavefronts per workgroup)."""
    return FAST_M[c], "mixed" if g2 >> 1 else "nm%d" % FAST_NM[c], 8 if g2 & 1 else 4


BRICKWORK = dict(k=0.816, rho=1700., cp=800., front_thermal_abs=0., back_thermal_abs=0.)   # surface.rs:1061-1075
POLYURETHANE = dict(k=0.0252, rho=17.5, cp=2400., front_thermal_abs=0., back_thermal_abs=0.)  # surface.rs:1048-1059
CONCRETE = dict(k=0.816, rho=1700., cp=800.)  # tests/massive_*/in.idf, tests/tilted/back.spl


def surfaces_model(segs, dt, front_kind, back_kind, n_zones=0, zone_volume=(), front_zone=0, back_zone=0,
                   front_ambient=0.0, back_ambient=0.0, front_emis=0.0, back_emis=0.0, area=4.0, perimeter=8.0,
                   cos_tilt=1.0, normal=(0., 0., 1.), wind_modifier=None, height=10.0, hs_fix=None, copies=1):
    """A model dict with `copies` identical surfaces built from one discretization dict `segs`
    (keys mass, uvalue, seg_cavity, cavities, front_alpha, back_alpha)."""
    n = len(segs["mass"])
    S = copies
    md = mdl.empty(S, n_zones, dt)
    md["node_offset"] = np.arange(S + 1, dtype=np.int64) * n
    for k in ("mass", "uvalue", "front_alpha", "back_alpha"):
        md[k] = np.tile(np.asarray(segs[k], dtype=np.float64), S)
    cav = segs.get("cavities")
    if cav is not None and len(cav):
        nc = len(cav)
        sc = np.asarray(segs["seg_cavity"], dtype=np.int32)
        allsc = []
        allcav = []
        for s in range(S):
            allsc.append(np.where(sc >= 0, sc + s * nc, -1))
            allcav.append(cav)
        md["seg_cavity"] = np.concatenate(allsc).astype(np.int32)
        md["cavities"] = np.concatenate(allcav)
    md["front_kind"] = np.full(S, front_kind, dtype=np.int32)
    md["back_kind"] = np.full(S, back_kind, dtype=np.int32)
    md["front_zone"] = np.full(S, front_zone, dtype=np.int32)
    md["back_zone"] = np.full(S, back_zone, dtype=np.int32)
    md["front_ambient"] = np.full(S, front_ambient)
    md["back_ambient"] = np.full(S, back_ambient)
    md["front_emissivity"] = np.full(S, front_emis)
    md["back_emissivity"] = np.full(S, back_emis)
    md["area"] = np.full(S, area)
    md["perimeter"] = np.full(S, perimeter)
    md["cos_tilt"] = np.full(S, cos_tilt)
    md["normal_x"] = np.full(S, normal[0])
    md["normal_y"] = np.full(S, normal[1])
    wm = mdl.wind_speed_modifier(height) if wind_modifier is None else wind_modifier
    md["wind_modifier"] = np.full(S, wm)
    if hs_fix is not None:
        md["front_hs_fix"] = np.full(S, hs_fix[0])
        md["back_hs_fix"] = np.full(S, hs_fix[1])
    md["zone_volume"] = np.asarray(zone_volume, dtype=np.float64)
    state = mdl.layout_state(md)
    return md, state


def random_zone_graph_model(seed):
    """The random small models of test_planner_stress_random_zone_graphs: walls, facings, windows, partitions, walls
    between random pairs of zones (longer chains), zones nobody faces, walls facing the same zone on both sides,
    walls facing no zone. Returns (model dict, initial state)."""
    rng = np.random.default_rng(1000 + seed)
    S = int(rng.integers(60, 900))
    Z = int(rng.integers(3, 40))
    gen = mdl.rooms_with_windows if seed % 2 else mdl.clustered_massive
    md, st = gen(S, Z=Z, dt=45.0, seed=seed)
    pick = rng.random(S)
    both = (md["front_kind"] == mdl.SPACE) & (md["back_kind"] == mdl.SPACE)
    rew = both & (pick < 0.3)
    md["front_zone"] = np.where(rew, rng.integers(0, Z, S), md["front_zone"]).astype(np.int32)
    same = both & (pick > 0.9)
    md["front_zone"] = np.where(same, md["back_zone"], md["front_zone"]).astype(np.int32)
    nodes = np.diff(md["node_offset"])
    lone = (pick > 0.5) & (pick < 0.56) & (nodes > 4)
    md["front_kind"] = np.where(lone, mdl.AMBIENT, md["front_kind"]).astype(np.int32)
    md["back_kind"] = np.where(lone, mdl.OUTDOOR, md["back_kind"]).astype(np.int32)
    md["front_ambient"] = np.where(lone, 12.5, md["front_ambient"])
    md["_rng"] = rng
    return md, st


def walls_example_model(n_walls=12):
    """The building of examples/march_walls.cpp as a model dict, discretized by the oracle's restatement of the
    setup (so that it needs no device library): 12 walls — concrete / insulation-concrete-insulation / insulation —
    around two zones, every fifth wall between the zones."""
    from oracle import oracle as orc
    ins = dict(thickness=0.02, k=0.0252, rho=17.5, cp=2400.)
    conc = dict(thickness=0.2, k=0.816, rho=1700., cp=800.)
    mass, uval, offs = [], [], [0]
    main_dt = 3600.0 / 20
    segs = []
    for i in range(n_walls):
        layers = [conc] if i % 3 == 0 else ([ins, conc, ins] if i % 3 == 1 else [ins])
        segs.append(orc.discretize(layers, main_dt, 0.04, 60.0))
    dt = main_dt / max(sg["tstep_subdivision"] for sg in segs) / 2.0
    for sg in segs:
        mass.extend(sg["mass"]); uval.extend(sg["uvalue"]); offs.append(offs[-1] + len(sg["mass"]))
    S = n_walls
    md = mdl.empty(S, 2, dt)
    md["node_offset"] = np.asarray(offs, dtype=np.int64)
    md["mass"] = np.asarray(mass); md["uvalue"] = np.asarray(uval)
    N = offs[-1]
    fa = np.zeros(N); ba = np.zeros(N)
    fa[md["node_offset"][:-1]] = 0.7
    ba[md["node_offset"][1:] - 1] = 0.7
    md["front_alpha"], md["back_alpha"] = fa, ba
    i = np.arange(S)
    md["front_kind"] = np.where(i % 5 == 4, mdl.SPACE, mdl.OUTDOOR).astype(np.int32)
    md["back_kind"] = np.full(S, mdl.SPACE, dtype=np.int32)
    md["front_zone"] = np.ones(S, dtype=np.int32)
    md["back_zone"] = (i % 2).astype(np.int32)
    md["front_ambient"] = np.zeros(S); md["back_ambient"] = np.zeros(S)
    md["front_emissivity"] = np.where(i % 3 == 0, 0.9, 0.2); md["back_emissivity"] = md["front_emissivity"].copy()
    md["area"] = 10.0 + i
    md["perimeter"] = 2.0 * (md["area"] / 3.0 + 3.0)
    md["cos_tilt"] = np.zeros(S)
    md["normal_x"] = np.sin(0.4 * i); md["normal_y"] = np.cos(0.4 * i)
    md["wind_modifier"] = np.array([mdl.wind_speed_modifier(1.5 + 3.0 * (q % 4)) for q in range(S)])
    md["zone_volume"] = np.array([600.0, 250.0])
    state = mdl.layout_state(md)
    return md, state


# ---------------------------------------------------------------------------------------------------------------------
# Sweeps over the edges of the side physics (tests/physics_ref.py; the host and the GPU tests share them)
def _signed(vals):
    out = []
    for v in vals:
        out.append(v)
        if v != 0:
            out.append(-v)
    return out


_DT_EXACT = [0.0, 1e-9, 4e-4, float(np.nextafter(1e-3, 0.0)), 1e-3, float(np.nextafter(1e-3, 1.0)), 2.2e-3]
DT_EDGES = _signed(_DT_EXACT + [0.5, 7.0, 40.0])            # air - surface: the 1.31 branch and the MIN_H clamp straddled
COS_EDGES = _signed([0.0, float(np.nextafter(1e-3, 0.0)), 1e-3, 0.5, 0.707, float(np.nextafter(0.98, 0.0)), 0.98, 1.0])
GRID = 2.0 ** -26


def on_grid(x):
    """x rounded to the 2^-26 grid: sums and differences of such temperatures are exact in f64."""
    return np.round(np.asarray(x, dtype=np.float64) / GRID) * GRID


def is_exact_dt(dt):
    """The temperature differences that are given exactly (a face at 0.0 or an air at 0.0)."""
    return abs(dt) <= 2.2e-3


def tarp_sweep():
    """(air, surface, cos_tilt) triples: DT_EDGES x COS_EDGES; the small differences against a face at 0.0 and against
    an air at 0.0 (both exact), the others on the grid around three face temperatures."""
    rows = []
    for d in DT_EDGES:
        for c in COS_EDGES:
            if is_exact_dt(d):
                rows.append((d, 0.0, c))
                rows.append((0.0, -d, c))
            else:
                for face in (-12.25, 3.0 + 5 * GRID, 31.5 - GRID):
                    rows.append((face + d, face, c))
    return np.array(rows)


WIND_SWEEP = [(0.0, 0.0), (0.0, 3.5), (-0.0, 0.75), (2.0, 9.0), (4.4, 0.31), (5.9, 2.0)]   # (direction rad, speed m/s)
NORMALS = [(1.0, 0.0), (-1.0, 0.0), (-0.0, 1.0), (0.0, -1.0), (0.6, 0.8), (-0.6, -0.8), (0.8, -0.6)]
GEOMETRY = [(4.0, 8.0, 1.0), (37.5, 25.0, 0.45), (0.81, 3.6, 0.62), (120.0, 62.0, 0.0), (11.0, 13.5, 0.3)]  # area, perimeter, wind modifier

CAVITY_THICKNESS = [0.006, 0.0127, 0.02, 0.03, 0.05, 0.1]
CAVITY_DT = _signed([0.0, 5e-11, 1e-6, 0.3, 3.0, 15.0, 40.0])
CAVITY_EMIS = [(0.84, 0.84), (0.1, 1.0), (0.3, 0.1), (1.0, 1.0), (0.84, 0.3), (1.0, 0.3), (0.1, 0.1)]   # (ein, eout)


def cavity_angles():
    rad = math.radians
    a = [0.0, 1e-6, rad(30.0)]
    for deg in (59.5, 60.5, 89.5, 90.5):
        a += [rad(deg) - 1e-9, rad(deg) + 1e-9]
    a += [rad(60.0), rad(73.0), rad(90.0), rad(134.0), rad(179.9)]
    return a


def cavity_exact_angles():
    """The f64 value of every regime boundary expression of `nusselt` (gas.rs:198-215), and the angles whose flip
    (180 deg - angle, gas.rs:137-139) lands on one: the branch taken there is part of the claim."""
    import physics_ref as pr
    out = []
    for b in pr.REGIME_BOUNDS:
        out += [b, pr.PI_RAD_180 - b]
    return out


def cavity_sweep(angles=None):
    """Records (cavity, t_front, t_back): thickness x temperature difference x gas x angle, height 1, the emissivity
    pairs taken in turn. The mean temperature wanders between 5 and 30 C on the grid."""
    angles = cavity_angles() if angles is None else angles
    cavs, tf, tb = [], [], []
    i = 0
    for th in CAVITY_THICKNESS:
        for d in CAVITY_DT:
            for gas in range(4):
                for ang in angles:
                    ein, eout = CAVITY_EMIS[i % len(CAVITY_EMIS)]
                    base = float(on_grid(5.0 + 25.0 * ((i * 0.6180339887) % 1.0)))
                    cavs.append((th, 1.0, ang, eout, ein, gas, 0))
                    tf.append(base)
                    tb.append(base - d if abs(d) < 1e-3 else float(on_grid(base - d)))
                    i += 1
    return np.array(cavs, dtype=mdl.CAVITY_DTYPE), np.array(tf), np.array(tb)


def rel_distance(got, ref):
    """|got - ref| / |ref| of an f64 against an extended-precision reference, as a float."""
    ref = np.longdouble(ref)
    return float(abs(np.longdouble(got) - ref) / abs(ref))


# ---------------------------------------------------------------------------------------------------------------------
def ambient_backs(md, state, rng, fraction):
    """Turns the BACK side of a share of the surfaces to Boundary::AmbientTemperature, in place, across all three kinds
    of front side; returns the indices of the converted surfaces. The conversion is tools/fuzz.py's `ambient_backs`
    (the fuzzer draws it too; the suite's own tests import the fuzzer, and it has to load beside any tests/helpers.py
    those tests come with, so it cannot take a name from here that older ones lack): see there for what it guarantees —
    emissivities of 0.3 at least, faces more than 0.5 K apart, ambient temperatures from U(5, 30) more than 0.5 K off
    the front face, the front side's air and the zone."""
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import fuzz
    return fuzz.ambient_backs(md, state, rng, fraction)


# ---------------------------------------------------------------------------------------------------------------------
# Buildings for the team tests (tests/test_team_rounds_gpu.py)
def faced_buildings(md, state, every=3, seed=0):
    """No-mass facings on every `every`-th wall of a modeldict.partitioned_buildings model (all-massive walls of one
    material each, four nodes at least), in place, in the pattern of modeldict.ragged_mixed: node 0 and node n-1 carry no
    mass, their neighbours half an element's mass, the first and the last segment are a thin insulation layer of
    U in U[0.5, 3]; both emissivities of those walls are scaled by 0.2 / 0.9, which keeps the reference's no-mass update
    in its convergent regime (see ragged_mixed). Returns (md, state); the state's layout does not change."""
    rng = np.random.default_rng(seed)
    S = int(md["n_surfaces"])
    off = np.asarray(md["node_offset"], dtype=np.int64)
    assert np.all(np.diff(off) >= 4)
    faced = np.arange(S) % every == 0
    first, last = off[:-1][faced], off[1:][faced] - 1
    mass = np.array(md["mass"], dtype=np.float64)
    u = np.array(md["uvalue"], dtype=np.float64)
    half = mass[first].copy()          # an end node of an all-massive wall holds half an element's mass
    mass[first] = 0.0
    mass[last] = 0.0
    mass[first + 1] = half
    mass[last - 1] = half
    u_ins = rng.uniform(0.5, 3.0, S)[faced]
    u[first] = u_ins
    u[last - 1] = u_ins
    md["mass"], md["uvalue"] = mass, u
    for key in ("front_emissivity", "back_emissivity"):
        md[key] = np.where(faced, np.asarray(md[key]) * (0.2 / 0.9), md[key])
    return md, state


def uneven_parts(n, rooms_list, seed):
    """One building of 12 walls a room (n nodes each) per entry of rooms_list: [(md, state), ...]."""
    return [mdl.partitioned_buildings(rooms * 12, n, rooms=rooms, dt=45.0, seed=seed + 17 * k)
            for k, rooms in enumerate(rooms_list)]


def uneven_buildings(n, rooms_list, seed):
    """The buildings of uneven_parts joined by modeldict.concat into ONE site: clusters of different sizes in one batch —
    teams of different member counts, and plain resident workgroups beside them. Returns (md, state); the state is the
    buildings' states back to back."""
    parts = uneven_parts(n, rooms_list, seed)
    md, _ = mdl.concat([m for m, _ in parts])
    return md, np.concatenate([s for _, s in parts])
