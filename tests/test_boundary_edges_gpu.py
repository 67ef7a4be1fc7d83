"""The per-side boundary physics of the kernels at its edges, against tests/physics_ref.py (extended precision, written
from the reference's text; tests/test_physics_ref_host.py holds it to mpmath and the CPU oracle to it).

Convection coefficients (hs_front / hs_back, flow_front / flow_back)
    The slots hold the coefficients of the POST-step node temperatures (model.rs:150-169). Walls of 1e25 J/m2K per node
    do not move (dt U dT / m is far below an ulp), so the march returns the node temperatures it was given — asserted
    first, bit for bit — and the slots are a known function of the inputs: physics_ref on exactly those f64 numbers.
    A face at exactly 0.0 (the exact-threshold cases: `air - 0.0` is the air, exactly) is the one temperature no finite
    mass holds bit for bit (0.0 + 1e-25 is 1e-25): for faces below 1e-8 in magnitude the assertion is that `air - face`,
    the only way the face enters, is unchanged in f64, and the expected values are taken on the returned numbers.
    Swept (tests/helpers.py): air - surface over 0, 1e-9, 4e-4, the two neighbours of 1e-3 and 1e-3 itself, 2.2e-3, 0.5,
    7, 40, both signs (the 1.31 branch and the MIN_H clamp of each of the three forms straddled); cos_tilt over 0, the
    neighbours of 1e-3 and of 0.98, 0.5, 0.707, 1, both signs; wind speed 0 and positive; wind direction 0 against
    normals (+-1, 0) (a dot product of exactly 0: leeward), -0.0, directions clearly windward and leeward (the 0.98 cases
    face away from the wind: a wrong "always windward" bit doubles the forced term); several areas, perimeters and wind
    modifiers; sides Ambient (natural only; a back Ambient side reads the FRONT node, surface.rs:677) and Outdoor.
    Tolerance, for coefficients and flows alike: eight times the oracle's worst relative distance from physics_ref over
    the same sweep (its leaf functions, and the flows formed from them as the oracle forms them; measured in the test,
    on the host), at least 4 ulp, never above 1e-13.

Cavity U-value
    Four-node massive walls, node node | cavity | node node (cluster-resident: three nodes on either side, two lanes,
    two sub-timesteps in one launch, the reference marched two steps with the cavity evaluated again), dt 30 s, 1500 J/m2K per node, 5 W/m2K in the solid, both
    faces Outdoor with fixed coefficients, no long-wave, no sun: the cavity conductance, frozen at the pre-step
    temperatures, moves its two nodes by dt/m U dT, and one RK4 step of physics_ref is the expectation. Thickness, gas,
    emissivities, temperature difference (both signs: the 180 deg - angle flip) and angle (every regime boundary at
    +- 1e-9 rad) swept as the issue lists them; all five regimes in all three Rayleigh cells, asserted. The angles that
    ARE the f64 value of a boundary expression are compared with the oracle (the branch taken is the claim there).
    Tolerance on temperatures: eight times the oracle's distance from physics_ref on the same walls, at least 8 ulp
    of the temperature; the implied relative error of U (|dT| / (dt/m U |T2 - T1|), where |T2 - T1| >= 0.3 K) at most 1e-12.

Measured on an MI355X (worst relative distance of hs and flows from physics_ref; the oracle's own distance on the same
numbers 3.3e-16 to 3.4e-16 for the coefficients, 3.7e-16 to 4.6e-16 with the flows):
    the planner's choice at 0 / 4 / 8 / 16 nodes per lane   4.44e-16      without the palette            4.44e-16
    catch-all kernel (force_general)                        4.61e-16      small kernel (two no-mass)     4.27e-16
    zone-facing sides, cluster-resident march               4.63e-16      the same walls, streamed       4.63e-16
Cavity walls (worst |dT| of a node after the step; the oracle's own 1.91e-14 K, tolerance 1.53e-13 K; implied U error):
    planned (register kernel, cavity tiles)   1.32e-14 K   8.8e-14
    catch-all kernel (force_general)          1.91e-14 K   1.0e-13      (without the palette a cavity wall is the catch-all's too)
Every test prints its figures (classes, cluster-resident walls, worst distances, tolerance) before it asserts.
"""
import ctypes as C
import math

import numpy as np
import pytest

import helpers as h
import physics_ref as pr
from heat_amd import HeatBatch
from heat_amd import modeldict as mdl

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
MASS = 1e25
T_OUT = [0.0, 0.0, 0.0, 3.25, -7.5, 12.0 + 2.0 ** -20]        # outdoor air of the calls; their wind is h.WIND_SWEEP
A, O, SP = mdl.AMBIENT, mdl.OUTDOOR, mdl.SPACE


# ---------------------------------------------------------------------------------------------------------------------
# B. convection coefficients
def edge_model(combos, node_counts, n_zones=0, massive=True):
    """One surface per (kind combination, air - surface of the front side, cos_tilt, node count); the back side's
    difference, the normal and the geometry taken in turn with periods coprime to the sweep's."""
    dts = h.DT_EDGES if massive else [d for d in h.DT_EDGES if abs(d) >= 0.5]
    rows = [(fk, bk, i, j, n) for n in node_counts for (fk, bk) in combos for i in range(len(dts))
            for j in range(len(h.COS_EDGES))]
    S = len(rows)
    n_nodes = np.array([r[4] for r in rows], dtype=np.int64)
    md = mdl.empty(S, n_zones, 30.0)
    off = np.concatenate(([0], np.cumsum(n_nodes))).astype(np.int64)
    md["node_offset"] = off
    N = int(off[-1])
    surf = np.repeat(np.arange(S), n_nodes)
    local = np.arange(N) - off[surf]
    last_node = local == n_nodes[surf] - 1
    md["mass"] = np.full(N, MASS if massive else 0.0)
    md["uvalue"] = np.where(last_node, 0.0, 1e-6 if massive else 2.0)
    md["front_alpha"], md["back_alpha"] = np.zeros(N), np.zeros(N)
    k = np.arange(S)
    md["front_kind"] = np.array([r[0] for r in rows], dtype=np.int32)
    md["back_kind"] = np.array([r[1] for r in rows], dtype=np.int32)
    md["front_zone"] = (k % max(n_zones, 1)).astype(np.int32)
    md["back_zone"] = ((k % max(n_zones, 1)) ^ 1).astype(np.int32) if n_zones else np.zeros(S, np.int32)
    md["front_emissivity"], md["back_emissivity"] = np.zeros(S), np.zeros(S)
    md["cos_tilt"] = np.array([h.COS_EDGES[r[3]] for r in rows])
    nrm = np.array([h.NORMALS[q % len(h.NORMALS)] for q in k])
    md["normal_x"], md["normal_y"] = nrm[:, 0].copy(), nrm[:, 1].copy()
    geo = np.array([h.GEOMETRY[(q // 4) % len(h.GEOMETRY)] for q in k])
    md["area"], md["perimeter"], md["wind_modifier"] = geo[:, 0].copy(), geo[:, 1].copy(), geo[:, 2].copy()
    md["zone_volume"] = np.full(n_zones, 250.0)
    md["front_ambient"], md["back_ambient"] = np.zeros(S), np.zeros(S)
    st = mdl.layout_state(md)
    st[md["zone_slot"]] = 0.0
    st[md["ir_front_slot"]] = mdl.SIGMA * 283.15 ** 4
    st[md["ir_back_slot"]] = mdl.SIGMA * 283.15 ** 4
    first = md["first_node_slot"]
    last = first + n_nodes - 1
    exact = 0
    for s, (fk, bk, i, j, n) in enumerate(rows):
        d_f = dts[i]
        d_b = dts[(7 * i + 3 * j + s // 7) % len(dts)]
        face = float(h.on_grid(-11.0 + 37.0 * ((s * 0.6180339887) % 1.0)))
        # front face: the air of an Outdoor or Space side is 0.0 in the first calls (face = -difference, exact); an
        # Ambient side brings its own air (face 0.0 for the small differences, exact)
        if fk == A:
            t0 = 0.0 if (not massive or h.is_exact_dt(d_f) or (bk == A and h.is_exact_dt(d_b))) else face
            md["front_ambient"][s] = t0 + d_f
            exact += t0 == 0.0
        else:
            t0 = -d_f
        if bk == A:      # evaluated on the FRONT node
            tn = float(h.on_grid(t0 + 1.75 - 3.5 * ((s * 0.377) % 1.0)))
            md["back_ambient"][s] = t0 + d_b
        else:
            tn = -d_b
        if massive:
            st[first[s]:last[s] + 1] = h.on_grid(np.linspace(t0, tn, n))
            st[first[s]], st[last[s]] = t0, tn
    assert exact > 100 or not massive
    return md, st


_EXPECTED = {}


def expected_sides(oracle, md, st_in, st_out, call):
    """hs and flows of both sides from physics_ref, on the air of the call's incoming state and the node temperatures of
    its outgoing one; and the worst relative distance from them of the oracle's leaf functions, and of the flows formed
    from those as the oracle forms them, on the same numbers.
    (Computed once for the kernel families that are given, and return, the same temperatures.)"""
    slots = np.concatenate([mdl.node_slots(md), md["zone_slot"]])
    key = (call, md["n_surfaces"], md["front_kind"].tobytes(), st_in[slots].tobytes(), st_out[slots].tobytes())
    if key not in _EXPECTED:
        _EXPECTED[key] = _expected_sides(oracle, md, st_in, st_out, call)
    return _EXPECTED[key]


def _expected_sides(oracle, md, st_in, st_out, call):
    lib = oracle.lib()
    err = C.c_int(0)
    wd, ws = h.WIND_SWEEP[call]
    t_out = T_OUT[call]
    S = md["n_surfaces"]
    first = md["first_node_slot"]
    last = first + np.diff(md["node_offset"]) - 1
    out = np.zeros((4, S), dtype=np.longdouble)
    worst = 0.0
    for s in range(S):
        t0, tn, ct = float(st_out[first[s]]), float(st_out[last[s]]), float(md["cos_tilt"][s])
        area, per, wm = float(md["area"][s]), float(md["perimeter"][s]), float(md["wind_modifier"][s])
        ww = pr.is_windward(wd, ct, float(md["normal_x"][s]), float(md["normal_y"][s]))
        assert ww == bool(lib.or_is_windward(wd, ct, float(md["normal_x"][s]), float(md["normal_y"][s])))
        for side, (kind, zone, amb) in enumerate(((md["front_kind"][s], md["front_zone"][s], md["front_ambient"][s]),
                                                  (md["back_kind"][s], md["back_zone"][s], md["back_ambient"][s]))):
            air = float(amb) if kind == A else (t_out if kind == O else float(st_in[md["zone_slot"][zone]]))
            hs = pr.side_hs(int(kind), side == 0, air, float(amb), t0, tn, ct, ws, wm, area, per, ww)
            face = t0 if side == 0 else tn
            out[side, s] = hs
            out[2 + side, s] = (np.longdouble(face) - np.longdouble(air)) * hs
            surf = t0 if (side == 0 or kind == A) else tn
            if kind == O:
                o = lib.or_tarp_total(air, surf, -ct if side == 0 else ct, ws * wm, area, per, int(ww), C.byref(err))
            else:
                o = lib.or_tarp_natural(air, surf, ct, C.byref(err))
            worst = max(worst, h.rel_distance(o, hs))
            if face != air:      # the flow as the oracle forms it (model.rs:161-169): one f64 difference, one product
                worst = max(worst, h.rel_distance((face - air) * o, out[2 + side, s]))
    assert err.value == 0
    return out, worst


def check_nodes_held(md, st_in, st_out, t_out):
    """The massive walls return the temperatures they were given."""
    ns = mdl.node_slots(md)
    a, b = st_in[ns], st_out[ns]
    tiny = np.abs(a) < 1e-8
    assert np.array_equal(a[~tiny], b[~tiny]), "%d node temperatures moved" % int((a[~tiny] != b[~tiny]).sum())
    assert np.all(np.abs(b[tiny] - a[tiny]) < 1e-18)
    # a face at (nearly) 0.0 enters through `air - face` only: that difference is what it was, to the bit around the
    # thresholds (4e-4, 1e-3 and its neighbours, 2.2e-3) and within 1e-18 for 0 and 1e-9, which sit far inside the 1.31
    # branch and under the MIN_H clamp
    first = md["first_node_slot"]
    last = first + np.diff(md["node_offset"]) - 1

    def same(air, slot, on):
        d0, d1 = air - st_in[slot[on]], air - st_out[slot[on]]
        assert np.all((d0 == d1) | ((np.abs(d0) < 1e-4) & (np.abs(d1 - d0) < 1e-18)))
    for kind, amb in ((md["front_kind"], md["front_ambient"]), (md["back_kind"], md["back_ambient"])):
        on = (kind == A) & (np.abs(st_in[first]) < 1e-8)
        same(amb[on], first, on)
    for kind, slot in ((md["front_kind"], first), (md["back_kind"], last)):
        on = (kind == O) & (np.abs(st_in[slot]) < 1e-8)
        same(t_out, slot, on)


def run_edges(oracle, md, st, massive, **opts):
    """A handful of calls of one sub-timestep each, another wind in every one. Returns the worst relative distance of
    the four slots from physics_ref and the tolerance they were held to."""
    worst_gpu, worst_or = 0.0, 0.0
    cur = st.copy()
    records = []
    with HeatBatch(md, **opts) as b:
        counts, n_fused = b.class_counts(), b.n_fused_surfaces
        if opts.get("fuse_always"):
            assert n_fused == md["n_surfaces"], (n_fused, counts)
        if opts.get("no_fusion"):
            assert n_fused == 0, n_fused
            if massive and not opts.get("force_general") and not opts.get("no_palette"):
                assert counts[3] == 0 and sum(counts[:3]) > 0, counts       # the streamed register kernel
        if opts.get("force_general"):
            assert counts[4] == md["n_surfaces"]
        if not massive:
            assert counts[3] == md["n_surfaces"], counts
        for call in range(len(T_OUT)):
            before = cur.copy()
            wd, ws = h.WIND_SWEEP[call]
            b.upload_state(cur)
            b.march(cur, np.array([[T_OUT[call], wd, ws]]))
            if opts.get("fuse_always"):
                assert b.n_fused_launches > call
            if massive:
                check_nodes_held(md, before, cur, T_OUT[call])
            records.append((before, cur.copy()))
    for call, (before, after) in enumerate(records):
        exp, d_or = expected_sides(oracle, md, before, after, call)
        worst_or = max(worst_or, d_or)
        for i, key in enumerate(("hs_front_slot", "hs_back_slot", "flow_front_slot", "flow_back_slot")):
            got = after[md[key]]
            e = exp[i]
            nz = e != 0
            assert np.all(got[~nz] == 0.0), key
            d = np.abs(got[nz].astype(np.longdouble) - e[nz]) / np.abs(e[nz])
            records[call] += ((key, float(d.max()), int(np.flatnonzero(nz)[d.argmax()])),)
            worst_gpu = max(worst_gpu, float(d.max()))
    tol = max(8.0 * worst_or, 4.0 * ULP)
    print("edges %s: classes %s, %d cluster-resident: GPU worst %.3e, oracle worst %.3e, tolerance %.3e" % (
        opts, counts, n_fused, worst_gpu, worst_or, tol))
    assert tol <= 1e-13
    for call, rec in enumerate(records):
        for key, d, s in rec[2:]:
            assert d <= tol, "call %d %s: %.3e > %.3e at surface %d (kinds %d/%d, cos_tilt %r)" % (
                call, key, d, tol, s, md["front_kind"][s], md["back_kind"][s], md["cos_tilt"][s])
    return worst_gpu, tol


def test_the_sweep_holds_what_it_claims():
    """Leeward sides just below |cos_tilt| = 0.98 in wind, a dot product of exactly 0, all four side kinds at a face of 0.0."""
    md, st = edge_model([(A, A), (A, O), (O, A), (O, O)], (2,))
    lee = 0
    for wd, ws in h.WIND_SWEEP:
        for s in range(md["n_surfaces"]):
            ct = md["cos_tilt"][s]
            if abs(ct) == float(np.nextafter(0.98, 0)) and ws > 0 and md["wind_modifier"][s] > 0:
                lee += not pr.is_windward(wd, ct, md["normal_x"][s], md["normal_y"][s])
    assert lee > 50
    assert md["normal_x"][0] * math.sin(0.0) + md["normal_y"][0] * math.cos(0.0) == 0.0


@pytest.mark.parametrize("opts", [dict(nodes_per_lane=0), dict(nodes_per_lane=4), dict(nodes_per_lane=8),
                                  dict(nodes_per_lane=16), dict(nodes_per_lane=0, no_fusion=True),
                                  dict(nodes_per_lane=4, no_fusion=True), dict(nodes_per_lane=8, no_fusion=True),
                                  dict(nodes_per_lane=16, no_fusion=True), dict(no_palette=True), dict(force_general=True)],
                         ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_convection_coefficients_of_ambient_and_outdoor_sides(oracle, opts):
    """Walls of 2, 7 and 33 nodes: one lane per wall, and several. The planner's own choice at every blocking factor
    (a small batch of walls that face no zone may be marched cluster-resident as a whole: the line printed says how
    many were), and the same with fusion forbidden: the streamed register kernel, asserted."""
    md, st = edge_model([(A, A), (A, O), (O, A), (O, O)], (2, 7, 33))
    run_edges(oracle, md, st, True, **opts)


def test_convection_coefficients_of_zone_facing_sides_in_the_resident_march(oracle):
    """Sides that face zones (at 0.0 in the first call: the small differences exact), cluster-resident."""
    md, st = edge_model([(SP, SP), (O, SP), (A, SP), (SP, A), (SP, O)], (2, 7, 33), n_zones=16)
    run_edges(oracle, md, st, True, fuse_always=True)
    run_edges(oracle, md, st, True, no_fusion=True)


def test_convection_coefficients_in_the_small_kernel(oracle):
    """All-no-mass walls of two nodes: their temperatures are solved, so physics_ref is applied to the face temperatures
    the GPU returned (the predicates are decided on f64 values the test sees); no exact-threshold inputs."""
    md, st = edge_model([(A, A), (A, O), (O, A), (O, O)], (2,), massive=False)
    run_edges(oracle, md, st, False)


# ---------------------------------------------------------------------------------------------------------------------
# C. cavity U-value
DT_C, MASS_C, U_SOLID, HS_FIX = 30.0, 1500.0, 5.0, (8.0, 12.0)
T_OUT_C = 10.0


def cavity_model(angles=None, n_side=2):
    """Walls of n_side massive nodes on either side of a cavity (the sweep's temperatures on the two cavity nodes)."""
    cavs, tf, tb = h.cavity_sweep(angles)
    S, n = len(cavs), 2 * n_side
    md = mdl.empty(S, 0, DT_C)
    md["node_offset"] = np.arange(S + 1, dtype=np.int64) * n
    md["mass"] = np.full(n * S, MASS_C)
    u = np.full(n, U_SOLID)
    u[n_side - 1] = u[n - 1] = 0.0
    md["uvalue"] = np.tile(u, S)
    segc = np.full(n * S, -1, dtype=np.int32)
    segc[n_side - 1::n] = np.arange(S)
    md["seg_cavity"], md["cavities"] = segc, cavs
    md["front_alpha"], md["back_alpha"] = np.zeros(n * S), np.zeros(n * S)
    for key in ("front_kind", "back_kind"):
        md[key] = np.full(S, O, dtype=np.int32)
    for key in ("front_zone", "back_zone"):
        md[key] = np.zeros(S, dtype=np.int32)
    for key in ("front_ambient", "back_ambient", "front_emissivity", "back_emissivity", "normal_x"):
        md[key] = np.zeros(S)
    md["normal_y"] = np.ones(S)
    md["area"], md["perimeter"], md["wind_modifier"] = np.full(S, 4.0), np.full(S, 8.0), np.full(S, 0.5)
    md["cos_tilt"] = np.cos(cavs["angle"])
    md["front_hs_fix"], md["back_hs_fix"] = np.full(S, HS_FIX[0]), np.full(S, HS_FIX[1])
    md["zone_volume"] = np.zeros(0)
    st = mdl.layout_state(md)
    st[md["ir_front_slot"]] = mdl.SIGMA * 283.15 ** 4
    st[md["ir_back_slot"]] = mdl.SIGMA * 283.15 ** 4
    f = md["first_node_slot"]
    for j in range(n_side):
        st[f + n_side - 1 - j] = tf if j == 0 else h.on_grid(tf + 0.5 * j)
        st[f + n_side + j] = tb if j == 0 else h.on_grid(tb - 0.25 * j)
    return md, st


def reference_steps(md, st, n_steps):
    """n_steps RK4 steps of physics_ref per wall; between two steps the temperatures are rounded to f64, as the state
    holds them, and the cavity is evaluated again on them. Returns [S, n] longdouble."""
    S = md["n_surfaces"]
    f = md["first_node_slot"]
    n = int(md["node_offset"][1])
    front = dict(air_t=T_OUT_C, rad_t=T_OUT_C, hs=HS_FIX[0], rad_hs=0.0)
    back = dict(air_t=T_OUT_C, rad_t=T_OUT_C, hs=HS_FIX[1], rad_hs=0.0)
    out = np.zeros((S, n), dtype=np.longdouble)
    for s in range(S):
        T = [float(x) for x in st[f[s]:f[s] + n]]
        seg = [U_SOLID] * (n - 1)
        seg[n // 2 - 1] = md["cavities"][s]
        for k in range(n_steps):
            Tn = pr.massive_wall_step([MASS_C] * n, seg, T, DT_C, front, back)
            if k < n_steps - 1:
                T = [float(x) for x in Tn]
        out[s] = Tn
    return out


_CAVITY_CASES = {}


def cavity_case(oracle, n_side, n_steps):
    """The walls, physics_ref's expectation after n_steps, and the tolerance from the oracle's march of the same walls."""
    key = (n_side, n_steps)
    if key not in _CAVITY_CASES:
        md, st = cavity_model(n_side=n_side)
        f = md["first_node_slot"] + n_side - 1
        labels = [pr.cavity_labels(md["cavities"][s], st[f[s]], st[f[s] + 1]) for s in range(md["n_surfaces"])]
        assert set(labels) == {(r, c) for r in pr.REGIMES for c in pr.RA_CELLS}, sorted(set(labels))
        ns = mdl.node_slots(md).reshape(-1, 2 * n_side)
        exp = reference_steps(md, st, n_steps)
        ref = st.copy()
        rc, _ = oracle.OracleModel(md).march(ref, np.tile([T_OUT_C, 0.0, 2.0], (n_steps, 1)))
        assert rc == 0
        d_or = np.abs(ref[ns].astype(np.longdouble) - exp).astype(np.float64)
        tol = np.maximum(8.0 * d_or.max(), 8.0 * ULP * np.abs(exp.astype(np.float64)))
        _CAVITY_CASES[key] = dict(md=md, st=st, labels=labels, exp=exp, tol=tol, d_or=float(d_or.max()))
    return _CAVITY_CASES[key]


def implied_u_error(md, st, exp, got, n_side):
    """|dT| of the two cavity nodes over dt/m U |T2 - T1|, for the walls with at least 0.3 K across the cavity."""
    f = md["first_node_slot"] + n_side - 1
    t1, t2 = st[f], st[f + 1]
    on = np.abs(t2 - t1) >= 0.3
    u = np.array([float(pr.cavity_u_value(md["cavities"][s], t1[s], t2[s])) for s in np.flatnonzero(on)])
    dT = np.abs(got[on][:, n_side - 1:n_side + 1].astype(np.longdouble) - exp[on][:, n_side - 1:n_side + 1]).astype(np.float64).max(axis=1)
    return dT / (DT_C / MASS_C * u * np.abs(t2 - t1)[on])


@pytest.mark.parametrize("opts", [dict(), dict(no_palette=True), dict(force_general=True), dict(fuse_always=True)],
                         ids=lambda o: "-".join(o) or "planned")
def test_cavity_u_value_moves_its_nodes_as_the_reference_says(oracle, opts):
    """Four-node walls, one step. The cluster-resident march takes a wall that faces no zone from two lanes on
    (plan.cpp, lone surfaces), so its walls have three nodes on either side of the cavity (four nodes per lane: two
    lanes), and it marches two sub-timesteps in one launch — the cavity is evaluated again between them, in the
    reference's two steps as well."""
    fused = bool(opts.get("fuse_always"))
    n_side, n_steps = (3, 2) if fused else (2, 1)
    case = cavity_case(oracle, n_side, n_steps)
    md, st, exp, tol = case["md"], case["st"], case["exp"], case["tol"]
    got = st.copy()
    with HeatBatch(md, **opts) as b:
        counts = b.class_counts()
        if fused:
            assert b.n_fused_surfaces == md["n_surfaces"], (b.n_fused_surfaces, counts)
        elif opts.get("force_general") or opts.get("no_palette"):
            assert counts[4] == md["n_surfaces"], counts          # (without the palette a cavity wall is the catch-all's)
        else:
            assert counts[3] == 0 and counts[4] == 0, counts      # cavity tiles on the fast path
        b.upload_state(got)
        b.march(got, np.tile([T_OUT_C, 0.0, 2.0], (n_steps, 1)))
        if fused:
            assert b.n_fused_launches > 0
    g = got[mdl.node_slots(md)].reshape(-1, 2 * n_side)
    d = np.abs(g.astype(np.longdouble) - exp).astype(np.float64)
    implied = implied_u_error(md, st, exp, g, n_side) / n_steps
    print("cavity %s: GPU worst |dT| %.3e K, oracle %.3e K, implied U error %.3e" % (opts, d.max(), case["d_or"], implied.max()))
    s = int((d / tol).max(axis=1).argmax())
    assert np.all(d <= tol), "wall %d %s %s: |dT| %s K, allowed %s" % (s, md["cavities"][s], case["labels"][s], d[s], tol[s])
    assert implied.max() <= 1e-12


def test_cavity_at_the_exact_regime_boundaries_takes_the_oracles_branch(oracle):
    """The angles that are the f64 value of a boundary expression of `nusselt` (and those whose flip lands on one)."""
    for opts, n_side, n_steps in ((dict(), 2, 1), (dict(no_palette=True), 2, 1), (dict(force_general=True), 2, 1),
                                  (dict(fuse_always=True), 3, 2)):
        md, st = cavity_model(h.cavity_exact_angles(), n_side=n_side)
        w = np.tile([T_OUT_C, 0.0, 2.0], (n_steps, 1))
        ref = st.copy()
        rc, _ = oracle.OracleModel(md).march(ref, w)
        assert rc == 0
        ns = mdl.node_slots(md)
        got = st.copy()
        with HeatBatch(md, **opts) as b:
            if opts.get("fuse_always"):      # (walls of two lanes: see the test above)
                assert b.n_fused_surfaces == md["n_surfaces"], (b.n_fused_surfaces, b.class_counts())
            b.upload_state(got)
            b.march(got, w)
        # a wrong branch moves U by a part in 1e3 and more, the nodes by 1e-4 K; the same branch agrees to roundings:
        # 64 ulp of the temperatures the step works with (Celsius values cross zero, the terms of the step are of the
        # size of the 10 C outdoor air and more: 1.4e-13 K at least)
        scale = np.maximum(np.abs(ref[ns]), T_OUT_C)
        assert np.all(np.abs(got[ns] - ref[ns]) <= 64 * ULP * scale), (opts, np.abs(got[ns] - ref[ns]).max())


def test_double_glazing_in_the_small_kernel(oracle):
    """Four no-mass nodes: the cavity is evaluated again in every pass of the no-mass loop. Against the oracle at the
    suite's 1e-9, pass counts equal (the high-precision method does not apply to the iterated solve)."""
    from test_parity_gpu import assert_state_close, run_both
    cavs, _, _ = h.cavity_sweep()
    keep = (cavs["thickness"] == 0.0127)
    cavs = cavs[keep][::13]                       # every angle, every gas; one thickness, the emissivities in turn
    cavs = np.concatenate([cavs, h.cavity_sweep(h.cavity_exact_angles())[0][::13]])
    pairs = {(float(a), int(g)) for a, g in zip(cavs["angle"], cavs["gas"])}
    assert pairs == {(a, g) for a in h.cavity_angles() + h.cavity_exact_angles() for g in range(4)}
    S = len(cavs)
    md = mdl.empty(S, 2, 45.0)
    md["node_offset"] = np.arange(S + 1, dtype=np.int64) * 4
    md["mass"] = np.zeros(4 * S)
    md["uvalue"] = np.tile([1.0 / 0.003, 0.0, 1.0 / 0.003, 0.0], S)
    segc = np.full(4 * S, -1, dtype=np.int32)
    segc[1::4] = np.arange(S)
    md["seg_cavity"], md["cavities"] = segc, cavs
    md["front_alpha"] = np.tile([0.05, 0.05, 0.03, 0.03], S)
    md["back_alpha"] = np.tile([0.03, 0.03, 0.05, 0.05], S)
    md["front_kind"] = np.full(S, O, dtype=np.int32)
    md["back_kind"] = np.full(S, SP, dtype=np.int32)
    md["front_zone"] = np.zeros(S, dtype=np.int32)
    md["back_zone"] = (np.arange(S) % 2).astype(np.int32)
    md["front_ambient"], md["back_ambient"] = np.zeros(S), np.zeros(S)
    md["front_emissivity"], md["back_emissivity"] = np.full(S, 0.2), np.full(S, 0.2)
    md["area"], md["perimeter"], md["wind_modifier"] = np.full(S, 2.0), np.full(S, 6.0), np.full(S, 0.6)
    md["cos_tilt"] = np.cos(cavs["angle"])
    md["normal_x"], md["normal_y"] = np.sin(cavs["angle"]), np.zeros(S)
    md["zone_volume"] = np.array([80.0, 120.0])
    st = mdl.layout_state(md)
    rng = np.random.default_rng(5)
    st[md["zone_slot"]] = [24.0, 17.0]
    st[md["solar_front_slot"]] = rng.uniform(0., 600., S)
    mdl.set_ir_from_air(md, st, -3.0)
    w = mdl.weather_series(4, 45.0, wind_speed=2.0, wind_deg=80.0)
    w[:, 0] -= 13.0                               # cold outside: 20 K and more across the glazing, both cavity flips occur
    ref, got, iters, gpu_iters, counts = run_both(oracle, md, st, w, np.array([300., 0.]), np.array([10., 0.]))
    assert counts[3] == S and iters == gpu_iters and iters > 0
    assert_state_close(md, ref, got)
