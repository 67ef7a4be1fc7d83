"""The cases of the air networks' tests (include/heat_amd.h, heat_air_networks), shared by tests/test_air_networks_host.py — which
runs them through the CPU oracle alone and asserts the conditions below — and tests/test_air_networks_gpu.py. They build on the
controllers' cases: zone loads, air paths, handlers, two species, the openings, the controllers and the room radiation; the
networks, a few controllers that open their windows and the air paths that read every derived channel are appended.

Every zone is a node of one network. On ragged_mixed (20 zones) the networks have 1, 2, 8 and 9 nodes; on
rooms_with_windows_large (500 zones) 1, 2, 7, 8, 9, 10, 12, 13, 16, 17, 20, 32, 33 and 64 nodes and the rest threes and fives,
shuffled, so that every width class has a full wavefront of networks and a ragged last one where it can have one: the class of 8
lanes many full wavefronts and a tail, the class of 16 lanes five networks (9, 10, 12, 13, 16: four and one), the class of 32
three (17, 20, 32: two and one), the class of 64 two (33, 64; its workgroups hold one network and are never ragged —
wave_shapes, asserted by the host test). A network is a tree of doorways — half of them
air_networks.tall_opening pairs, so two links join the same two zones — plus a few more doorways that close loops, and links to
outside at two or more heights behind wind pressures of four facades. Open fractions come from a schedule that leaves [0, 1], from
a controller that senses the zone (a window that follows the room temperature) or are absent; one node in six has an extract fan.

The expected result is DEFINED by `loop_with_rules`: per step heat_amd.controllers.apply, heat_amd.openings.apply and
heat_amd.air_networks.apply on the zone and node temperatures the march call before returned and the step's channel row, then
the existing terms' rules on the row with its derived columns, the room radiation's rule; the inputs written; one march call.

The host's channel table holds NaN in every derived column: the contract ignores a derived column's host values."""
import numpy as np

from heat_amd import air_networks as an, air_paths, controllers as ctl, openings as opn
import controllers_cases as cc
import openings_cases as oc
import room_radiation_cases as rrc

SEED = 97
N_STEPS = 24
MARGIN = oc.MARGIN
MAX_ITER = 24          # twice the worst count of the rule's prototype
TOL = 1e-7
C_MAX = 1.5            # the largest flow coefficient of a case: the oracle bound's Lipschitz constant rests on it
ORACLE_CASES = [("ragged_mixed", 2), ("ragged_mixed", 5)]
SIZES = {20: [1, 2, 8, 9], 500: [1, 2, 7, 8, 9, 10, 12, 13, 16, 17, 20, 32, 33, 64]}


def network_sizes(Z, rng):
    """The node counts of a case's networks: SIZES, then the rest as threes and fives, shuffled."""
    sizes = list(SIZES[Z])
    rest = Z - sum(sizes)
    threes = next(b for b in range(5) if (rest - 3 * b) % 5 == 0 and rest >= 3 * b)
    threes += 5 * int(rng.integers(0, (rest - 3 * threes) // 15 + 1))
    sizes += [3] * threes + [5] * ((rest - 3 * threes) // 5)
    return [int(v) for v in rng.permutation(sizes)]


def random_networks(c, rng, floor, tol):
    """Appends the networks' channels and derived columns to c["channel"], the window controllers to c["controllers"], the paths
    that read every derived column to c["air"], and returns (networks, info). floor: every p_lin is at least 0.1 Pa (the
    oracle cases); else p_lin is drawn from 0.01 Pa up."""
    md, n_steps = c["md"], c["n_steps"]
    Z = int(md["n_zones"])
    op, oinfo = c["openings"], c["openings_info"]
    t_out_chan = np.asarray(op["temp_chan"])[oinfo["outside"]]        # the outside temperature of every zone
    sizes = network_sizes(Z, rng)
    zones = rng.permutation(Z)
    off = np.concatenate([[0], np.cumsum(sizes)])
    # kind 0: a link to outside, 1: a doorway link, + 2: the link never closes — the doorways of a network's tree and its first
    # link to outside carry no open fraction, so no room and no network is ever sealed around its extract fan
    za, zb, cc_, gh, kind = [], [], [], [], []
    for w, n in enumerate(sizes):
        zs = zones[off[w]:off[w + 1]]
        storey = 3.0 * (np.arange(n) // 4)                            # four rooms a storey: a stairwell's stack over the taller ones
        doors = [(i, int(rng.integers(0, i))) for i in range(1, n)] + [tuple(rng.choice(n, 2, replace=False)) for _ in range(n // 6)]
        for j, (a, b) in enumerate(doors):
            if rng.random() < 0.5:
                a, b = b, a
            if j % 2 == 0:
                t = an.tall_opening(rng.uniform(0.7, 1.0), rng.uniform(1.9, 2.2), rng.uniform(0.5, 0.7), sill=max(storey[a], storey[b]))
                for h in range(2):
                    za.append(zs[a]), zb.append(zs[b]), cc_.append(float(t["c"][h])), gh.append(float(t["gh"][h])), kind.append(1 if j >= n - 1 else 3)
            else:                                                     # a closed door: its undercut and cracks
                za.append(zs[a]), zb.append(zs[b]), cc_.append(float(an.orifice(rng.uniform(0.005, 0.03), 0.6))), kind.append(1 if j >= n - 1 else 3)
                gh.append(an.G * (max(storey[a], storey[b]) + rng.uniform(0.0, 2.0)))
        outside = [i for i in range(n) if rng.random() < 0.85] or [0]
        if len(outside) < 2:
            outside.append(outside[0] if n == 1 else (outside[0] + 1) % n)
        for j, i in enumerate(outside):
            za.append(zs[i]), zb.append(-1), cc_.append(float(an.orifice(rng.uniform(0.004, 0.04), 0.6))), kind.append(0 if j else 2)
            gh.append(an.G * (storey[i] + rng.uniform(0.3, 2.6)))
    L = len(za)
    perm = rng.permutation(L)
    za, zb, cc_, gh, kind = (np.asarray(v)[perm] for v in (za, zb, cc_, gh, kind))
    out_l = np.flatnonzero(zb < 0)
    # ---- the channels: open fractions, wind pressures of four facades, the fans; then the derived columns ----
    c0 = c["channel"].shape[1]
    frac = rng.uniform(-0.3, 1.4, (n_steps, 2))
    wp = rng.uniform(-6.0, 6.0, (n_steps, 4))
    fan = -rng.uniform(0.005, 0.03, (n_steps, 1))                     # kg/s: an extract fan takes air out
    c_frac, c_wp, c_fan = c0, c0 + 2, c0 + 6
    # the window controllers: half of the outside links that close open with the room temperature (cooling action)
    closes = kind < 2
    auto = out_l[closes[out_l] & (rng.random(len(out_l)) < 0.5)]
    n_ct = len(auto)
    cool_sp = np.asarray(c["controllers"]["set_chan"])[np.asarray(c["controllers"]["action"]) < 0]
    windows = dict(sense_index=za[auto], set_chan=rng.choice(cool_sp, n_ct), action=-np.ones(n_ct, np.int32), kp=1.0 / rng.uniform(2.0, 8.0, n_ct),
                   bias=rng.uniform(0.0, 0.5, n_ct), out_hi=np.ones(n_ct))
    n_out_cols = 2 * int((zb >= 0).sum()) + len(out_l)
    c_ct, c_out = c0 + 7, c0 + 7 + n_ct
    windows["out_chan"] = (c_ct + rng.permutation(n_ct)).astype(np.int32)
    c["channel"] = np.concatenate([c["channel"], frac, wp, fan, np.full((n_steps, n_ct + n_out_cols), np.nan)], axis=1)
    n_before_ct = ctl.n_controllers(c["controllers"])
    c["controllers"] = ctl.concat(c["controllers"], windows)
    frac_chan = np.where(closes & (rng.random(L) < 0.8), c_frac + rng.integers(0, 2, L), -1)
    frac_chan[auto] = windows["out_chan"]
    cols = c_out + rng.permutation(n_out_cols)
    out_ab, out_ba = np.full(L, -1), np.full(L, -1)
    inner = np.flatnonzero(zb >= 0)
    out_ab[inner], out_ba[inner], out_ba[out_l] = cols[:len(inner)], cols[len(inner):2 * len(inner)], cols[2 * len(inner):]
    N = Z
    fans = rng.random(N) < 1.0 / 6.0
    nw = dict(net_offset=off.astype(np.int32), tol=np.full(len(sizes), tol), max_iter=np.full(len(sizes), MAX_ITER, np.int32),
              g_min=np.full(len(sizes), 1e-9), node_zone=zones.astype(np.int32), src_chan=np.where(fans, c_fan, -1).astype(np.int32),
              src_gain=rng.uniform(0.5, 1.5, N), zone_a=za.astype(np.int32), zone_b=zb.astype(np.int32),
              temp_chan=np.where(zb < 0, t_out_chan[za], -1).astype(np.int32), wp_chan=np.where(zb < 0, c_wp + rng.integers(0, 4, L), -1).astype(np.int32),
              wp_gain=rng.uniform(0.5, 1.0, L), frac_chan=frac_chan.astype(np.int32), out_ab=out_ab.astype(np.int32), out_ba=out_ba.astype(np.int32),
              c=cc_, gh=gh, p_lin=rng.uniform(0.1, 0.12, L) if floor else rng.uniform(0.01, 0.12, L))
    assert nw["c"].max() <= C_MAX
    paths = an.paths(nw)
    n_before = air_paths.n_paths(c["air"])
    c["air"] = air_paths.concat(c["air"], {k: v for k, v in paths.items() if k != "link"})
    info = dict(sizes=np.asarray(sizes), kind=kind, auto=auto, windows=np.arange(n_before_ct, n_before_ct + n_ct), fans=np.flatnonzero(fans),
                paths=np.arange(n_before, n_before + len(paths["link"])), path_link=paths["link"], derived=np.arange(c_out, c_out + n_out_cols),
                c_wp=c_wp, plan=an.structure(nw))
    return nw, info


def case(model, n_steps, n_sub, form, seed, floor=True, tol=TOL):
    c = cc.case(model, n_steps, n_sub, form, seed, floor=floor)
    rng = np.random.default_rng(seed + 4000)
    c["networks"], c["networks_info"] = random_networks(c, rng, floor, tol)
    return c


def rule_args(nw):
    """The networks' dict without what the binding alone takes."""
    return {k: v for k, v in nw.items() if k not in ("state", "stats", "resume")}


def networks_with(nw, acc):
    """The networks' dict with what a loop's carry or a series' result holds, as resume."""
    return dict(nw, resume={k: acc[k] for k in an.STATE + an.ACC if k in acc})


def loop_with_rules(march, c, state, steps=slice(None), carry=None, step_base=0):
    """The definition: per step controllers.apply, openings.apply and air_networks.apply, in this order, on the zone and node
    temperatures the state holds — each on the row the one before left —, then the existing terms' rules
    (air_species_cases.loop_with_rules) on the row with its derived columns and the room radiation's rule; the inputs written;
    one march call. march(state, weather of the step, a0, b0). Returns what that loop returns plus control_u, control_out,
    opening_v, irradiance, link_q, node_p, net_iters, what controllers_cases.margin needs, per step and network `fired` and per
    step and link `root` and `frac` (the unclamped open fraction), rows, and the carries of the three terms."""
    md, ct, op, rad = c["md"], cc.rule_args(c["controllers"]), c["openings"], c["radiation"]
    nw, plan = rule_args(c["networks"]), c["networks_info"]["plan"]
    ks = list(range(c["n_steps"])[steps])
    m, n = len(ks), ctl.n_controllers(ct)
    cn = an.counts(nw)
    acc_ct = {k: v.copy() for k, v in carry["controllers"].items()} if carry and "controllers" in carry else ctl.fresh(ct)
    acc_op = {k: v.copy() for k, v in carry["openings"].items()} if carry and "openings" in carry else opn.fresh(op)
    acc_nw = {k: v.copy() for k, v in carry["networks"].items()} if carry and "networks" in carry else an.fresh(nw)
    sum_irr = np.array(carry["sum_irradiance"]) if carry and "sum_irradiance" in carry else np.zeros(len(rad["rc_surface"]))
    both = dict(c, channel=c["channel"].copy())        # what the consumers read: the derived columns filled in step by step
    rec = dict(control_u=np.zeros((m, n)), control_out=np.zeros((m, n)), sensed=np.zeros((m, n)), limited=np.zeros((m, n)),
               integral_before=np.zeros((m, n)), tripped_before=np.zeros((m, n), np.uint8), irradiance=np.zeros((m, len(rad["rc_surface"]))),
               opening_v=np.zeros((m, opn.n_openings(op))), link_q=np.zeros((m, cn["link"])), node_p=np.zeros((m, cn["node"])),
               net_iters=np.zeros((m, cn["net"]), np.int32), fired=np.zeros((m, cn["net"]), bool), converged=np.zeros((m, cn["net"]), bool),
               root=np.zeros((m, cn["link"]), bool), mass_in=np.zeros((m, cn["node"])))
    g = {k: ctl._given(ct, k, n) for k in ctl.INT_KEYS}
    at = [0]

    def head():
        j, k = at[0], ks[at[0]]
        T = state[md["zone_slot"]]
        rec["sensed"][j] = ctl._read(g["sense_kind"], g["sense_index"], g["sense_node"], T, state, c["channel"][k], md)
        rec["limited"][j] = ctl._read(g["lim_kind"], g["lim_index"], g["lim_node"], T, state, c["channel"][k], md)
        rec["integral_before"][j], rec["tripped_before"][j] = acc_ct["integral"], acc_ct["tripped"]
        row, rec["control_u"][j], rec["control_out"][j] = ctl.apply(T, state, c["channel"][k], ct, acc_ct, md)
        ctl.accumulate(rec["control_u"][j], rec["control_out"][j], acc_ct)
        row, rec["opening_v"][j] = opn.apply(T, row, op)
        opn.accumulate(rec["opening_v"][j], acc_op, step_base + k)
        before = row
        row, r = an.apply(T, row, nw, acc_nw, plan)
        an.accumulate(r, acc_nw)
        for key in ("link_q", "node_p", "net_iters", "fired", "converged", "root"):
            rec[key][j] = r[key]
        rec["mass_in"][j] = an.mass_in(T, before, nw, r, plan)
        both["channel"][k] = row

    def step(s, wk, za, zb):
        j, k = at[0], ks[at[0]]
        rec["irradiance"][j] = rrc.rule(md, s, both["channel"][k], rad, c["drives"])
        sum_irr[:] = sum_irr + rec["irradiance"][j]
        s[rrc.receiver_slots(md, rad)] = rec["irradiance"][j]
        march(s, wk, za, zb)
        at[0] += 1
        if at[0] < m:
            head()                                     # (the next step's terms see the temperatures this march call returned)

    if ks:
        head()
    out = oc.asc.loop_with_rules(step, both, state, steps, carry, step_base)
    out.update(rec)
    out["rows"] = both["channel"][steps]
    fc = np.asarray(nw["frac_chan"])
    out["frac"] = np.where(fc >= 0, out["rows"][:, np.maximum(fc, 0)], 1.0)
    out["carry"]["controllers"], out["carry"]["openings"], out["carry"]["networks"], out["carry"]["sum_irradiance"] = acc_ct, acc_op, acc_nw, sum_irr
    return out


def margin(c, out):
    """The least distance, in K, that every decision of the controllers, the openings' consumers and the controlled paths keeps
    from its threshold (controllers_cases.margin, which includes openings_cases.margin)."""
    return cc.margin(c, out)


def wave_counts(c, out):
    """The largest number of different iteration counts among the networks of one wavefront at one step."""
    t = c["networks_info"]["sizes"]
    cls = np.select([t <= 8, t <= 16, t <= 32], [0, 1, 2], 3)
    best = 0
    for k in range(4):
        nets = np.flatnonzero(cls == k)
        per = 64 // (8 << k)
        for w0 in range(0, len(nets), per):
            its = out["net_iters"][:, nets[w0:w0 + per]]
            best = max(best, max(len(set(r.tolist())) for r in its))
    return best


def wave_shapes(sizes):
    """Per width class (8, 16, 32, 64 lanes): (networks, full workgroups, networks in the ragged last one)."""
    t = np.asarray(sizes)
    cls = np.select([t <= 8, t <= 16, t <= 32], [0, 1, 2], 3)
    return {8 << k: (int((cls == k).sum()), int((cls == k).sum()) // (8 >> k), int((cls == k).sum()) % (8 >> k)) for k in range(4)}


def coverage(c, out):
    """What a run of loop_with_rules exercised (the conditions of the issue, measured on the loop itself)."""
    q, frac = out["link_q"], out["frac"]
    fc = np.asarray(c["networks"]["frac_chan"])
    return dict(converged=float(out["converged"].mean()), worst_iters=float(out["net_iters"].max()), wave_counts=float(wave_counts(c, out)),
                reversing=float(((q > 0).any(axis=0) & (q < 0).any(axis=0)).mean()), linear=float((~out["root"]).mean()), root=float(out["root"].mean()),
                fired=float(out["fired"].any(axis=0).mean()), clamped=float(((frac < 0.0) | (frac > 1.0))[:, fc >= 0].mean()),
                imbalance=float(np.abs(out["mass_in"][out["converged"][:, c["networks_info"]["plan"]["node_net"]]]).max()))


def assert_coverage(cov, what="", tol=TOL):
    """The conditions of every case (conditions, not measurements). The signed mass into a zone is recomputed from the flows
    written with the operations of the last assembly, so at a converged step it is at most tol with no slack. With tol = 0.0
    a solve stops only at a residual of 0.0 exactly and otherwise runs its max_iter iterations: "every solve converges" and
    "three different counts in a wavefront" are conditions of the cases with a tolerance and are not asked there."""
    print("%s: %s" % (what, ", ".join("%s %.3g" % kv for kv in cov.items())))
    if tol > 0.0:
        assert cov["converged"] == 1.0 and cov["worst_iters"] <= MAX_ITER, (what, cov)
        assert cov["wave_counts"] >= 3, (what, cov)
    assert cov["imbalance"] <= tol, (what, cov)
    assert cov["reversing"] >= 0.10, (what, cov)
    assert cov["linear"] >= 0.05 and cov["root"] >= 0.50, (what, cov)
    assert cov["fired"] >= 0.5, (what, cov)
    assert cov["clamped"] >= 0.05, (what, cov)
