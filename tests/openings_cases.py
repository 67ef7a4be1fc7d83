"""The cases of the openings' tests (include/heat_amd.h, heat_openings), shared by tests/test_openings_host.py — which runs them
through the CPU oracle alone and asserts that the flows respond, that controlled paths open and close and that no controller
decision sits on its threshold — and tests/test_openings_gpu.py. They build on the air species' cases: zone loads, air paths,
handlers and two species; the openings and their consumers are appended.

The expected result is DEFINED by `loop_with_rules`: per step heat_amd.openings.apply on the zone temperatures the march call
before returned and the step's channel row, then the rules of air_species_cases.loop_with_rules on the row with its derived
columns; the driven inputs written; one march call. No device is needed to build a case or to run the loop through the oracle.

The host's channel table holds NaN in every derived column: the contract ignores a derived column's host values, and a device
that read one would show it in every zone the opening feeds."""
import numpy as np

from heat_amd import air_paths, openings as opn
import air_species_cases as asc

SEED = 71
N_STEPS = 24
MARGIN = 1e-6      # K: the distance every controller decision of an oracle case keeps from its threshold
ORACLE_CASES = [("ragged_mixed", 2), ("ragged_mixed", 5), ("rooms_with_windows", 2)]


def random_openings(c, rng, floor):
    """Appends the openings' channels and the derived columns to c["channel"], the consumers to c["air"] and c["loads"], and
    returns (openings, info). One opening to outside per zone — wind and stack (openings.wind_and_stack) or single-sided
    (openings.single_sided), three in four behind an open-fraction channel that leaves [0, 1] at times — and one doorway
    (openings.doorway) per pair of neighbouring zones (2j, 2j + 1), every other one behind the open-fraction channel. Each
    outside opening feeds a CONTROLLED supply path of its zone (a night-ventilation window: sense +1, the same outside
    temperature) and, in every other zone, a flow of the zone loads (infiltration at a third of the opening's flow); each doorway
    feeds the two paths of air_paths.doorway. The species ride on all of them through those terms' tables. floor: every c0 is
    at least 0.01 (the oracle cases); else a third of the openings have c0 = 0, where V ~ sqrt|dT| is not Lipschitz."""
    md, st, n_steps = c["md"], c["st"], c["n_steps"]
    Z = int(md["n_zones"])
    T0 = st[md["zone_slot"]]
    t_mid = float(np.median(T0))
    c0 = c["channel"].shape[1]
    wind = rng.uniform(0.2, 6.0, (n_steps, 2))
    frac = rng.uniform(-0.3, 1.4, (n_steps, 2))
    # (the cases' gains heat the zones by 5 to 25 K over the steps: outside temperatures and setpoints are drawn across that range, so
    # that a window's zone is above its setpoint at some steps and not at others, and the outside air helps at some and not at others)
    t_out = t_mid + rng.uniform(-8.0, 22.0, (n_steps, 2))
    setpoint = t_mid + rng.uniform(0.0, 22.0, (n_steps, 2))
    n_door = Z // 2
    n = Z + n_door
    derived = np.full((n_steps, n), np.nan)
    c["channel"] = np.concatenate([c["channel"], wind, frac, t_out, setpoint, derived], axis=1)
    c_wind, c_frac, c_temp, c_set, c_out = c0, c0 + 2, c0 + 4, c0 + 6, c0 + 8
    # ---- the openings to outside, then the doorways; the list is shuffled below ----
    site = rng.integers(0, 2, Z)
    a = rng.uniform(0.02, 0.08, Z)
    ws = opn.wind_and_stack(a, rng.uniform(0.55, 0.65, Z), rng.uniform(0.25, 0.6, Z), rng.uniform(0.3, 1.2, Z))
    ss = opn.single_sided(a, rng.uniform(0.8, 1.6, Z))
    single = rng.random(Z) < 0.5
    outside = dict(zone_a=np.arange(Z), zone_b=np.full(Z, -1), temp_chan=c_temp + site, wind_chan=c_wind + rng.integers(0, 2, Z),
                   frac_chan=np.where(rng.random(Z) < 0.75, c_frac + rng.integers(0, 2, Z), -1),
                   area=np.where(single, ss["area"], ws["area"]), cw=np.where(single, ss["cw"], ws["cw"]),
                   cs=np.where(single, 0.0, ws["cs"]), ca=np.where(single, ss["ca"], 0.0), c0=np.where(single, ss["c0"], 0.0))
    dw = opn.doorway(rng.uniform(0.7, 1.0, n_door), rng.uniform(1.9, 2.2, n_door), rng.uniform(0.4, 0.8, n_door))
    swap = rng.random(n_door) < 0.5
    lo, hi = 2 * np.arange(n_door), 2 * np.arange(n_door) + 1
    doors = dict(zone_a=np.where(swap, hi, lo), zone_b=np.where(swap, lo, hi),
                 frac_chan=np.where(np.arange(n_door) % 2 == 0, c_frac + rng.integers(0, 2, n_door), -1), area=0.1 * dw["area"], cs=dw["cs"])
    op = opn.concat(outside, doors)
    if floor:
        op["c0"] = np.maximum(op["c0"], rng.uniform(0.01, 0.03, n))
    else:
        op["c0"] = np.where(np.arange(n) % 3 == 0, 0.0, np.maximum(op["c0"], rng.uniform(0.0, 0.03, n)))
    perm = rng.permutation(n)
    op = {k: v[perm] for k, v in op.items()}
    where = np.argsort(perm)                                          # where[i]: the number opening i of the list above has now
    op["out_chan"] = (c_out + rng.permutation(n)).astype(np.int32)
    out_of = op["out_chan"][where]
    # ---- the consumers ----
    vents = dict(target=np.arange(Z), source=np.full(Z, -1), temp_chan=c_temp + site, volume_chan=out_of[:Z],
                 open_chan=c_set + rng.integers(0, 2, Z), sense=np.ones(Z, np.int8), band=rng.uniform(0.0, 1.5, Z),
                 min_delta=rng.uniform(0.0, 1.0, Z))
    pairs = air_paths.doorway(lo, hi, out_of[Z:])
    n_before = air_paths.n_paths(c["air"])
    c["air"] = air_paths.concat(c["air"], vents, pairs)
    leaky = np.arange(0, Z, 2)
    flows = dict(c["loads"]["flows"])
    flows = dict(zone=np.concatenate([flows["zone"], leaky]).astype(np.int32),
                 volume_chan=np.concatenate([flows["volume_chan"], out_of[leaky]]).astype(np.int32),
                 temp_chan=np.concatenate([flows["temp_chan"], c_temp + site[leaky]]).astype(np.int32),
                 volume_gain=np.concatenate([flows["volume_gain"], np.full(len(leaky), 1.0 / 3.0)]))
    c["loads"] = dict(c["loads"], flows=flows)
    info = dict(vents=np.arange(n_before, n_before + Z), pairs=np.arange(n_before + Z, n_before + Z + 2 * n_door), n=n,
                derived=np.arange(c_out, c_out + n), outside=where[:Z], doors=where[Z:])
    return op, info


def case(model, n_steps, n_sub, form, seed, floor=True):
    c = asc.case(model, n_steps, n_sub, form, seed)
    rng = np.random.default_rng(seed + 2000)
    c["openings"], c["openings_info"] = random_openings(c, rng, floor)
    return c


def loop_with_rules(march, c, state, steps=slice(None), carry=None, step_base=0):
    """The definition: per step openings.apply on the zone temperatures the state holds, then the zone loads', the air paths',
    the air handlers' and the air species' rules (air_species_cases.loop_with_rules) on the row with its derived columns; the
    inputs written; one march call. march(state, weather of the step, a0, b0). Returns what that loop returns plus opening_v,
    rows (the channel rows the consumers read) and carry["openings"]."""
    md, op = c["md"], c["openings"]
    ks = list(range(c["n_steps"])[steps])
    acc = {k: v.copy() for k, v in carry["openings"].items()} if carry and "openings" in carry else opn.fresh(op)
    seen = dict(c, channel=c["channel"].copy())   # what the consumers read: the derived columns filled in step by step
    opening_v = np.zeros((len(ks), opn.n_openings(op)))
    at = [0]

    def head():
        k = ks[at[0]]
        seen["channel"][k], opening_v[at[0]] = opn.apply(state[md["zone_slot"]], c["channel"][k], op)
        opn.accumulate(opening_v[at[0]], acc, step_base + k)

    def step(s, wk, za, zb):
        march(s, wk, za, zb)
        at[0] += 1
        if at[0] < len(ks):
            head()                                # (the next step's openings see the temperatures this march call returned)

    if ks:
        head()
    out = asc.loop_with_rules(step, seen, state, steps, carry, step_base)
    out["opening_v"], out["rows"] = opening_v, seen["channel"][steps]
    out["carry"]["openings"] = acc
    return out


def margin(c, out):
    """The least distance, in K, that a controlled path's e - d, e + d, g - min_delta and g keep from zero over a run of
    loop_with_rules (heat_amd/air_paths.py, apply: the four quantities its comparisons test). A NaN setpoint compares false
    whatever the temperatures are: it has no distance."""
    air = c["air"]
    ctl = np.asarray(air["open_chan"]) >= 0
    target, source = np.asarray(air["target"])[ctl], np.asarray(air["source"])[ctl]
    s, d = np.asarray(air["sense"], dtype=np.float64)[ctl], np.asarray(air["band"])[ctl] / 2.0
    md_ = np.asarray(air["min_delta"])[ctl]
    T, rows = out["zone_T"], out["rows"]
    tt = T[:, target]
    ts = np.where(source >= 0, T[:, np.maximum(source, 0)], rows[:, np.maximum(np.asarray(air["temp_chan"])[ctl], 0)])
    e = s * (tt - rows[:, np.asarray(air["open_chan"])[ctl]])
    g = s * (tt - ts)
    with np.errstate(invalid="ignore"):
        return float(np.nanmin(np.abs(np.stack([e - d, e + d, g - md_, g]))))


def coverage(c, out):
    """What a run of loop_with_rules exercised: the share of the openings whose V varies over the steps by more than a factor
    of two; of the controlled paths that read a derived channel the share of step-paths that are open, the share that opens at
    some step and the share that closes at some step; the share of opening-steps whose open fraction is clamped."""
    v, info = out["opening_v"], c["openings_info"]
    states = out["states"][:, info["vents"]].astype(np.int8)
    before = np.concatenate([np.zeros((1, states.shape[1]), np.int8), states[:-1]])
    fc = np.asarray(c["openings"]["frac_chan"])
    f = out["rows"][:, np.maximum(fc, 0)]
    return dict(responding=float((v.max(axis=0) > 2.0 * v.min(axis=0)).mean()), open=float(states.mean()),
                opening=float(((states - before) > 0).any(axis=0).mean()), closing=float(((states - before) < 0).any(axis=0).mean()),
                clamped=float(((fc >= 0)[None, :] & ((f < 0.0) | (f > 1.0))).mean()))


def assert_coverage(cov, what=""):
    """The conditions of every case (conditions, not measurements)."""
    print("%s: %s" % (what, ", ".join("%s %.2f" % kv for kv in cov.items())))
    assert cov["responding"] >= 0.5, (what, cov)
    assert 0.10 <= cov["open"] <= 0.90 and cov["opening"] >= 0.20 and cov["closing"] >= 0.20, (what, cov)
    assert cov["clamped"] >= 0.05, (what, cov)


def rule_args(op):
    """The openings' dict without what the binding alone takes."""
    return {k: v for k, v in op.items() if k not in ("stats", "resume", "step_base")}


def openings_with(op, acc, step_base):
    """The openings' dict with what a loop's carry or a series' result holds, as resume."""
    return dict(op, resume={k: acc[k] for k in opn.ACC if k in acc}, step_base=step_base)
