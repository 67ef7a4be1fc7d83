"""The cases of the controllers' tests (include/heat_amd.h, heat_controllers), shared by tests/test_controllers_host.py — which runs
them through the CPU oracle alone and asserts that the loops respond, that limits trip and release and that no decision sits on
its threshold — and tests/test_controllers_gpu.py. They build on the openings' cases: zone loads, air paths, handlers, two
species and the openings; the controllers, a small room-radiation term and their consumers are appended.

Two controllers per zone. The first, by zone number modulo 4: a modulating radiator (a gain of the zone loads), a window whose
open fraction follows the room temperature (the frac_chan of the zone's opening to outside), a supply fan (the volume of an
uncontrolled air path) and a radiant panel (a channel entry of a room-radiation receiver). The second is a slab: a massive wall
of the zone whose back alpha row controllers.embed has put on one node, heated in even zones and — with a negative out_hi —
cooled in odd ones, behind a high-limit cut-out that senses a node of the wall, half of them PI loops, sensing the zone's air,
the heated node itself or an outside-temperature channel, and every other one behind an enable channel that drops mid-series.

The expected result is DEFINED by `loop_with_rules`: per step heat_amd.controllers.apply on the zone and node temperatures the
march call before returned and the step's channel row, then openings_cases.loop_with_rules' rules on the row with its derived
columns, the room radiation's rule, the driven inputs written; one march call.

The host's channel table holds NaN in every derived column: the contract ignores a derived column's host values."""
import numpy as np

from heat_amd import air_paths, controllers as ctl, modeldict as mdl, openings as opn
import openings_cases as oc
import room_radiation_cases as rrc

SEED = 83
N_STEPS = 24
MARGIN = oc.MARGIN    # K: the distance every decision of an oracle case keeps from its threshold
ORACLE_CASES = [("ragged_mixed", 2), ("ragged_mixed", 5)]


def slab_surfaces(md):
    """One wall per zone for the slab: the first all-massive wall of at least 8 nodes whose back faces the zone."""
    Z = int(md["n_zones"])
    off = np.asarray(md["node_offset"], dtype=np.int64)
    count = np.diff(off)
    light = np.add.reduceat((np.asarray(md["mass"]) < 1e-5).astype(np.int64), off[:-1])
    ok = (light == 0) & (count >= 8) & (np.asarray(md["back_kind"]) == mdl.SPACE)
    out = np.full(Z, -1, np.int64)
    for s in np.flatnonzero(ok)[::-1]:
        out[int(md["back_zone"][s])] = s
    assert (out >= 0).all()
    return out


def random_controllers(c, rng):
    """Appends the controllers' channels and derived columns to c["channel"], embeds the slabs in c["md"], names the derived
    columns in c["loads"], c["openings"], c["air"], c["radiation"] and c["drives"], and returns (controllers, info)."""
    md, st, n_steps = c["md"], c["st"], c["n_steps"]
    Z = int(md["n_zones"])
    h = float(max(c["n_sub"], 1)) * float(md["dt"])
    T0 = st[md["zone_slot"]]
    t_mid = float(np.median(T0))
    op, oinfo = c["openings"], c["openings_info"]
    c0 = c["channel"].shape[1]
    # (the cases' gains heat the zones by 5 to 25 K over the steps: the setpoints are drawn across that range)
    heat_sp = t_mid + rng.uniform(2.0, 24.0, (n_steps, 2))
    cool_sp = t_mid + rng.uniform(-2.0, 16.0, (n_steps, 2))
    enable = np.ones((n_steps, 1))
    enable[n_steps // 2:n_steps // 2 + 4] = 0.0                       # drops mid-series, and comes back
    n = 2 * Z
    c["channel"] = np.concatenate([c["channel"], heat_sp, cool_sp, enable, np.full((n_steps, n), np.nan)], axis=1)
    c_heat, c_cool, c_en, c_out = c0, c0 + 2, c0 + 4, c0 + 5
    z = np.arange(Z)
    kind = z % 4
    t_out_chan = np.asarray(op["temp_chan"])[oinfo["outside"]]        # the outside temperature of every zone's opening
    # ---- the first controller of every zone ----
    heating = (kind == 0) | (kind == 3)
    band = rng.uniform(2.0, 8.0, Z)
    is_pi = (z // 4) % 2 == 1
    pi = ctl.pi(band, rng.uniform(4.0, 12.0, Z))
    pr = ctl.proportional(band)
    full = np.select([kind == 0, kind == 1, kind == 2], [rng.uniform(200.0, 1500.0, Z), np.ones(Z), rng.uniform(0.02, 0.08, Z)],
                     rng.uniform(5.0, 40.0, Z))
    first = dict(sense_index=z, set_chan=np.where(heating, c_heat, c_cool) + rng.integers(0, 2, Z), action=np.where(heating, 1, -1),
                 en_chan=np.where(kind == 3, c_en, -1), kp=pr["kp"], ki=np.where(is_pi, pi["ki"], 0.0), bias=np.where(is_pi, 0.0, pr["bias"]),
                 out_hi=full)
    # ---- the slabs ----
    slab = slab_surfaces(md)
    count = np.diff(np.asarray(md["node_offset"], dtype=np.int64))[slab]
    node = np.where(z % 5 == 0, count - 1, count // 2)                 # one in five at the back face: that wall stays in its class
    c["md"], drive = ctl.embed(md, slab, node, side="back")
    md = c["md"]
    area = np.asarray(md["area"])[slab]
    mass = np.asarray(md["mass"])[np.asarray(md["node_offset"])[slab] + node]
    flux = np.clip(mass * 8.0 / (4.0 * h), 10.0, 300.0)                # W/m2: about 8 K in four steps at full output
    cooling = z % 2 == 1
    sense_kind = np.select([z % 7 == 3, z % 3 == 0], [2, 1], 0)
    lim_at_node = z % 4 < 2                                            # the limit senses the heated node, or the wall's back face
    first_slot = np.asarray(md["first_node_slot"])[slab]
    # a heated node trips when it is warmer than every node of its wall was at the start; a back face a little above its start
    T_hi = np.where(lim_at_node, [st[f:f + m].max() for f, m in zip(first_slot, count)], st[first_slot + count - 1])
    lim_hi = np.where(cooling, 60.0, T_hi + rng.uniform(0.5, 2.5, Z))  # (a cooled slab never reaches its high limit)
    band2 = rng.uniform(3.0, 9.0, Z)
    pi2 = ctl.pi(band2, rng.uniform(4.0, 10.0, Z))
    is_pi2 = z % 4 < 2
    second = dict(sense_kind=sense_kind, sense_index=np.select([sense_kind == 2, sense_kind == 1], [t_out_chan, slab], z),
                  sense_node=np.where(sense_kind == 1, node, -1), set_chan=np.where(cooling, c_cool, c_heat) + rng.integers(0, 2, Z),
                  action=np.where(cooling, -1, 1), en_chan=np.where(z % 4 == 0, c_en, -1), kp=1.0 / band2,
                  ki=np.where(is_pi2, pi2["ki"], 0.0), bias=np.where(is_pi2, 0.0, 0.5), out_hi=np.where(cooling, -1.0, 1.0) * flux * area)
    second = ctl.with_limit(second, 1, slab, lim_hi, lim_hi - rng.uniform(0.2, 0.6, Z), np.where(lim_at_node, node, -1))
    ct = ctl.concat(first, second)
    perm = rng.permutation(n)
    ct = {k: v[perm] for k, v in ct.items()}
    where = np.argsort(perm)
    ct["out_chan"] = (c_out + rng.permutation(n)).astype(np.int32)
    out_of = ct["out_chan"][where]
    # ---- the consumers ----
    rad_z = np.flatnonzero(kind == 0)
    gains = dict(c["loads"]["gains"])
    gains = dict(zone=np.concatenate([gains["zone"], rad_z]).astype(np.int32), chan=np.concatenate([gains["chan"], out_of[rad_z]]).astype(np.int32),
                 factor=np.concatenate([gains["factor"], np.ones(len(rad_z))]))
    c["loads"] = dict(c["loads"], gains=gains)
    win_z = np.flatnonzero(kind == 1)
    frac = np.array(op["frac_chan"])
    frac[oinfo["outside"][win_z]] = out_of[win_z]
    c["openings"] = dict(op, frac_chan=frac.astype(np.int32))
    fan_z = np.flatnonzero(kind == 2)
    n_before = air_paths.n_paths(c["air"])
    c["air"] = air_paths.concat(c["air"], dict(target=fan_z, source=np.full(len(fan_z), -1), temp_chan=t_out_chan[fan_z], volume_chan=out_of[fan_z]))
    # a panel: the back of a wall of the zone (not the slab) receives its own emission, dimmed, plus the controller's W/m2
    pan_z = np.flatnonzero(kind == 3)
    back_space = np.asarray(md["back_kind"]) == mdl.SPACE
    wall = np.array([[s for s in np.flatnonzero(back_space & (np.asarray(md["back_zone"]) == zz)) if s != slab[zz]][0] for zz in pan_z], np.int64)
    R = len(wall)
    c["radiation"] = dict(rc_surface=wall, rc_side=np.ones(R, np.uint8), en_receiver=np.repeat(np.arange(R), 2),
                          en_surface=np.stack([wall, np.full(R, -1)], axis=1).reshape(-1), en_side=np.tile([1, 0], R).astype(np.uint8),
                          en_factor=np.stack([rng.uniform(0.85, 0.95, R), np.ones(R)], axis=1).reshape(-1),
                          en_chan=np.stack([np.full(R, -1), out_of[pan_z]], axis=1).reshape(-1).astype(np.int32))
    drives = {k: (v[0].copy(), v[1].copy()) for k, v in c["drives"].items() if v is not None}
    drives["ir_back"][0][wall] = -1                                    # an input has one source
    drives[drive["chan_key"]][0][slab] = out_of[Z:]
    drives[drive["chan_key"]][1][slab] = drive["gain"]
    c["drives"] = drives
    info = dict(first=where[:Z], second=where[Z:], kind=kind, slab=slab, node=node, cooling=cooling, n=n, derived=np.arange(c_out, c_out + n),
                fans=np.arange(n_before, n_before + len(fan_z)), general=drive["general"], c_en=c_en)
    return ct, info


def case(model, n_steps, n_sub, form, seed, floor=True):
    c = oc.case(model, n_steps, n_sub, form, seed, floor=floor)
    c["md_plain"] = c["md"]
    rng = np.random.default_rng(seed + 3000)
    c["controllers"], c["controllers_info"] = random_controllers(c, rng)
    return c


def rule_args(ct):
    """The controllers' dict without what the binding alone takes."""
    return {k: v for k, v in ct.items() if k not in ("state", "stats", "resume")}


def controllers_with(ct, acc):
    """The controllers' dict with what a loop's carry or a series' result holds, as resume."""
    return dict(ct, resume={k: acc[k] for k in ctl.STATE + ctl.ACC if k in acc})


def loop_with_rules(march, c, state, steps=slice(None), carry=None, step_base=0):
    """The definition: per step controllers.apply on the zone and node temperatures the state holds, then the openings' and the
    existing terms' rules (openings_cases.loop_with_rules) on the row with its derived columns, the room radiation's rule; the
    inputs written; one march call. march(state, weather of the step, a0, b0). Returns what that loop returns plus control_u,
    control_out, irradiance, sensed / limited / integral_before / tripped_before (what margin() needs), warmest (the warmest
    node of every slab after every step) and carry["controllers"], carry["sum_irradiance"]."""
    md, ct, rad = c["md"], rule_args(c["controllers"]), c["radiation"]
    info = c["controllers_info"]
    ks = list(range(c["n_steps"])[steps])
    n, m = ctl.n_controllers(ct), len(ks)
    acc = {k: v.copy() for k, v in carry["controllers"].items()} if carry and "controllers" in carry else ctl.fresh(ct)
    sum_irr = np.array(carry["sum_irradiance"]) if carry and "sum_irradiance" in carry else np.zeros(len(rad["rc_surface"]))
    seen = dict(c, channel=c["channel"].copy())       # the rows with the controllers' columns: what the openings' loop starts from
    rec = dict(control_u=np.zeros((m, n)), control_out=np.zeros((m, n)), sensed=np.zeros((m, n)), limited=np.zeros((m, n)),
               integral_before=np.zeros((m, n)), tripped_before=np.zeros((m, n), np.uint8), irradiance=np.zeros((m, len(rad["rc_surface"]))),
               warmest=np.zeros((m, len(info["slab"])), np.int64))
    g = {k: ctl._given(ct, k, n) for k in ctl.INT_KEYS}
    slots = [np.asarray(md["first_node_slot"])[s] + np.arange(np.diff(md["node_offset"])[s]) for s in info["slab"]]
    at = [0]

    def head():
        j, k = at[0], ks[at[0]]
        T = state[md["zone_slot"]]
        rec["sensed"][j] = ctl._read(g["sense_kind"], g["sense_index"], g["sense_node"], T, state, c["channel"][k], md)
        rec["limited"][j] = ctl._read(g["lim_kind"], g["lim_index"], g["lim_node"], T, state, c["channel"][k], md)
        rec["integral_before"][j], rec["tripped_before"][j] = acc["integral"], acc["tripped"]
        seen["channel"][k], rec["control_u"][j], rec["control_out"][j] = ctl.apply(T, state, c["channel"][k], ct, acc, md)
        ctl.accumulate(rec["control_u"][j], rec["control_out"][j], acc)

    def step(s, wk, za, zb):
        j, k = at[0], ks[at[0]]
        # (the openings' loop has written the driven inputs; the receivers' long-wave inputs are the room radiation's)
        rec["irradiance"][j] = rrc.rule(md, s, rows_of["channel"][k], rad, c["drives"])
        sum_irr[:] = sum_irr + rec["irradiance"][j]
        s[rrc.receiver_slots(md, rad)] = rec["irradiance"][j]
        march(s, wk, za, zb)
        rec["warmest"][j] = [int(np.argmax(s[sl])) for sl in slots]
        at[0] += 1
        if at[0] < m:
            head()                                     # (the next step's controllers see the temperatures this march call returned)

    rows_of = {}
    if ks:
        head()
    # the openings read row k of seen["channel"] when their head runs: after ours for that step
    out = _openings_loop(step, seen, state, steps, carry, step_base, rows_of)
    out.update(rec)
    out["carry"]["controllers"], out["carry"]["sum_irradiance"] = acc, sum_irr
    return out


def _openings_loop(step, seen, state, steps, carry, step_base, rows_of):
    """openings_cases.loop_with_rules on the table `seen` holds, whose rows our head fills in place ahead of the openings';
    rows_of["channel"]: the table the consumers read (the openings' copy with both kinds of derived columns)."""
    md, op = seen["md"], seen["openings"]
    ks = list(range(seen["n_steps"])[steps])
    acc = {k: v.copy() for k, v in carry["openings"].items()} if carry and "openings" in carry else opn.fresh(op)
    both = dict(seen, channel=seen["channel"].copy())
    rows_of["channel"] = both["channel"]
    opening_v = np.zeros((len(ks), opn.n_openings(op)))
    at = [0]

    def head():
        k = ks[at[0]]
        both["channel"][k], opening_v[at[0]] = opn.apply(state[md["zone_slot"]], seen["channel"][k], op)
        opn.accumulate(opening_v[at[0]], acc, step_base + k)

    def inner_step(s, wk, za, zb):
        step(s, wk, za, zb)                            # (ours: radiation, the march call, then the next step's controllers)
        at[0] += 1
        if at[0] < len(ks):
            head()

    if ks:
        head()
    out = oc.asc.loop_with_rules(inner_step, both, state, steps, carry, step_base)
    out["opening_v"], out["rows"] = opening_v, both["channel"][steps]
    out["carry"]["openings"] = acc
    return out


def margin(c, out):
    """The least distance, in K, that every decision of a run of loop_with_rules keeps from its threshold: the limits' Tl from
    lim_hi and, where tripped, from lim_lo; the integrators' and the signals' unclamped values from 0 and 1, as temperature
    errors (divided by ki and kp: u == 0 and u == 1 are reached by saturation only); and the openings' and paths' thresholds
    (openings_cases.margin)."""
    ct = rule_args(c["controllers"])
    n = ctl.n_controllers(ct)
    g = {k: ctl._given(ct, k, n) for k in ctl.KEYS}
    Ts, Tl, I0, trip0, u = out["sensed"], out["limited"], out["integral_before"], out["tripped_before"], out["control_u"]
    rows = out["rows"]
    worst = [oc.margin(c, out)]
    lim = g["lim_kind"] >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        d_hi = np.abs(Tl - g["lim_hi"])[:, lim]
        above = Tl > g["lim_hi"]
        d_lo = np.where((trip0 == 1) & ~above, np.abs(Tl - g["lim_lo"]), np.inf)[:, lim]
        trip1 = np.where(lim & above, 1, np.where(lim & (trip0 == 1) & (Tl < g["lim_lo"]), 0, trip0))
        enabled = (g["en_chan"] < 0) | (rows[:, np.maximum(g["en_chan"], 0)] > 0.0)
        run = enabled & (trip1 == 0)
        e0 = rows[:, g["set_chan"]] - Ts
        e = np.where(g["action"] > 0, e0, -e0)
        x = I0 + g["ki"] * e
        d_i = np.where(run & (g["ki"] > 0), np.minimum(np.abs(x), np.abs(x - 1.0)) / g["ki"], np.inf)
        v = g["kp"] * e + np.clip(x, 0.0, 1.0) + g["bias"]
        d_u = np.where(run & (g["kp"] > 0), np.minimum(np.abs(v), np.abs(v - 1.0)) / g["kp"], np.inf)
    for d in (d_hi, d_lo, d_i, d_u):
        if d.size:
            worst.append(float(np.nanmin(d)))
    return min(worst)


def coverage(c, out):
    """What a run of loop_with_rules exercised: the share of controller-steps with u strictly inside (0, 1), at 0 while running
    and at 1; the limits that trip and that release; the share of the enabled-channel controllers' steps that are disabled; the
    share of the heated slabs with an inside node whose heated node is the wall's warmest at some step at which they heat."""
    info, ct = c["controllers_info"], c["controllers"]
    u = out["control_u"]
    trips = out["carry"]["controllers"]["trips"]
    trip0 = out["tripped_before"]
    after = np.concatenate([trip0[1:], out["carry"]["controllers"]["tripped"][None, :]])
    en = np.asarray(ct["en_chan"])
    off = (en >= 0)[None, :] & ~(out["rows"][:, np.maximum(en, 0)] > 0.0)
    second = info["second"]
    count = np.diff(np.asarray(c["md"]["node_offset"]))[info["slab"]]
    inside = ~info["cooling"] & (info["node"] != count - 1)
    hot = ((out["warmest"] == info["node"][None, :]) & (u[:, second] > 0.0)).any(axis=0)
    cold = info["cooling"] & (out["control_out"][:, second] < 0.0).any(axis=0)
    return dict(inside=float(((u > 0.0) & (u < 1.0)).mean()), low=float(((u == 0.0) & ~off).mean()), high=float((u == 1.0).mean()),
                tripping=float((trips > 0).sum()), releasing=float(((trip0 == 1) & (after == 0)).any(axis=0).sum()),
                disabled=float(off[:, en >= 0].mean()), warmest=float(hot[inside].mean()), cooling=float(cold[info["cooling"]].mean()))


def assert_coverage(cov, what=""):
    """The conditions of every case (conditions, not measurements)."""
    print("%s: %s" % (what, ", ".join("%s %.2f" % kv for kv in cov.items())))
    assert cov["inside"] >= 0.10 and cov["low"] >= 0.05 and cov["high"] >= 0.05, (what, cov)
    assert cov["tripping"] >= 1 and cov["releasing"] >= 1, (what, cov)
    assert 0.05 <= cov["disabled"] <= 0.5, (what, cov)
    assert cov["warmest"] >= 0.5 and cov["cooling"] >= 0.5, (what, cov)
