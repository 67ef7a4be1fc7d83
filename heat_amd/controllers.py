"""Controllers of a series on the host (include/heat_amd.h, heat_controllers): the rule the device applies to every controller as
the first kernel of every step, in numpy, and conveniences that give the constants of common loops, join lists and embed a
controller's output in a wall. No device, no library.

apply() IS the contract's rule, line for line — every sum and product one rounded f64 operation in the header's order (numpy
never fuses a multiply-add) — and so the reference of the tests: a host that applies it to the step's channel row before the
openings' and the other terms' rules, between heat_batch_march_ex calls, gets the bits of heat_batch_march_series_controllers.
The reference has no counterpart: its harness feeds heating powers as given numbers."""
import numpy as np

INT_KEYS = ("sense_kind", "sense_index", "sense_node", "set_chan", "action", "en_chan", "lim_kind", "lim_index", "lim_node", "out_chan")
REAL_KEYS = ("kp", "ki", "bias", "out_lo", "out_hi", "lim_hi", "lim_lo")
KEYS = INT_KEYS + REAL_KEYS
STATE = ("integral", "tripped")
ACC = ("sum_u", "sum_out", "steps_on", "steps_sat", "trips")
_NEUTRAL = dict(sense_kind=0, sense_node=-1, action=1, en_chan=-1, lim_kind=-1, lim_index=-1, lim_node=-1, ki=0.0, bias=0.0, out_lo=0.0,
                lim_hi=0.0, lim_lo=0.0)
_DTYPE = dict(integral=np.float64, tripped=np.uint8, sum_u=np.float64, sum_out=np.float64, steps_on=np.int64, steps_sat=np.int64,
              trips=np.int64)


def n_controllers(ct):
    return 0 if not ct or ct.get("sense_index") is None else len(np.atleast_1d(ct["sense_index"]))


def _given(ct, key, n):
    dtype = np.int64 if key in INT_KEYS else np.float64
    return np.full(n, _NEUTRAL[key], dtype) if ct.get(key) is None else np.asarray(ct[key], dtype=dtype).reshape(-1)


def fresh(ct):
    """The state and the accumulators as resume == 0 leaves them on the device: all zero."""
    n = n_controllers(ct)
    return {k: np.zeros(n, _DTYPE[k]) for k in STATE + ACC}


def _read(kind, index, node, T, N, row, md):
    """What every controller senses (or limits on): [n]; where kind < 0 the value is 0 and unused.
    N: the caller's state vector; md: the model dict that places the nodes in it."""
    n = len(kind)
    out = np.zeros(n)
    z = kind == 0
    out[z] = T[index[z]]
    w = kind == 1
    if w.any():
        count = np.diff(np.asarray(md["node_offset"], dtype=np.int64))[index[w]]
        node_w = np.where(node[w] < 0, count - 1, node[w])
        out[w] = np.asarray(N, dtype=np.float64)[np.asarray(md["first_node_slot"], dtype=np.int64)[index[w]] + node_w]
    c = kind == 2
    out[c] = row[index[c]]
    return out


def apply(T, N, row, ct, state, md=None):
    """One step of the rule. Returns (row_with_derived_columns, u, out): a copy of `row` with out[i] stored at out_chan[i],
    and u, out [n_controllers], the step's rows of control_u and control_out. The integrals, the trip bytes and, where it
    holds one, the trips count of `state` (fresh(), or what a series returned) are updated in place.
    T     the zone AIR temperatures at the start of the step
    N     the state vector at the start of the step (read where a controller senses a node; may be None otherwise)
    row   the step's channel row (not written)
    ct    a dict of arrays: sense_index, set_chan, out_chan, kp, out_hi [n]; the others optional (make_controllers)
    md    the model dict (node_offset, first_node_slot): needed where a controller senses a node"""
    T = np.asarray(T, dtype=np.float64)
    new = np.array(row, dtype=np.float64)
    row = np.asarray(row, dtype=np.float64)
    n = n_controllers(ct)
    if n == 0:
        return new, np.zeros(0), np.zeros(0)
    g = {k: _given(ct, k, n) for k in KEYS}
    I, trip = state["integral"], state["tripped"]
    with np.errstate(invalid="ignore", over="ignore"):
        Ts = _read(g["sense_kind"], g["sense_index"], g["sense_node"], T, N, row, md)
        sp = row[g["set_chan"]]
        e0 = sp - Ts
        e = np.where(g["action"] > 0, e0, -e0)
        enabled = (g["en_chan"] < 0) | (row[np.maximum(g["en_chan"], 0)] > 0.0)
        lim = g["lim_kind"] >= 0
        Tl = _read(np.where(lim, g["lim_kind"], -1), g["lim_index"], g["lim_node"], T, N, row, md)
        above = lim & (Tl > g["lim_hi"])
        release = lim & ~above & (trip == 1) & (Tl < g["lim_lo"])
        if "trips" in state:
            state["trips"][above & (trip == 0)] += 1
        trip[above] = 1
        trip[release] = 0
        run = enabled & (trip == 0)
        p = g["kp"] * e
        ie = g["ki"] * e
        I1 = I + ie
        I1 = np.where(I1 < 0.0, 0.0, I1)
        I1 = np.where(I1 > 1.0, 1.0, I1)
        ub = p + I1
        u = ub + g["bias"]
        u = np.where(u < 0.0, 0.0, u)
        u = np.where(u > 1.0, 1.0, u)
        u = np.where(run, u, 0.0)
        I[:] = np.where(~enabled, 0.0, np.where(run, I1, I))
        span = g["out_hi"] - g["out_lo"]
        o = u * span
        out = g["out_lo"] + o
    new[g["out_chan"]] = out
    return new, u, out


def accumulate(u, out, acc):
    """The accumulators of one step, in place, from the u and out apply() returned (trips is apply()'s own)."""
    with np.errstate(invalid="ignore"):
        if "sum_u" in acc:
            acc["sum_u"][:] = acc["sum_u"] + u
        if "sum_out" in acc:
            acc["sum_out"][:] = acc["sum_out"] + out
        if "steps_on" in acc:
            acc["steps_on"][u > 0.0] += 1
        if "steps_sat" in acc:
            acc["steps_sat"][u >= 1.0] += 1


def concat(*parts):
    """Joins the lists of controller dicts (as apply() takes them) into one, filling what a part leaves out with the neutral
    value (sense_kind 0, action +1, a channel or limit -1, a constant 0)."""
    out = {}
    for key in KEYS:
        if key not in _NEUTRAL and all(p.get(key) is None for p in parts):
            continue  # (a list nobody has given yet: out_chan, where the caller numbers the derived channels afterwards)
        dtype = np.int32 if key in INT_KEYS else np.float64
        cols = [np.full(n_controllers(p), _NEUTRAL.get(key, 0), dtype) if p.get(key) is None else np.asarray(p[key], dtype=dtype).reshape(-1)
                for p in parts if n_controllers(p)]
        out[key] = np.concatenate(cols) if cols else np.zeros(0, dtype)
    return out


def proportional(band, full_at=None):
    """The constants of a proportional loop — a thermostatic radiator valve: u rises from 0 to 1 over `band` K of error,
    centred on the setpoint (u = 0.5 there) or, with full_at="band", from 0 at the setpoint to 1 at `band` K below it.
    Returns dict(kp, bias)."""
    band = np.asarray(band, dtype=np.float64)
    return dict(kp=1.0 / band, bias=np.zeros_like(band) if full_at == "band" else np.full_like(band, 0.5))


def pi(band, reset_steps):
    """The constants of a PI loop in the standard form u = kp (e + sum(e) / Ti): kp = 1 / band, and the integrator gains
    ki = kp / reset_steps per step — the caller's reset time Ti in steps of the series. The integrator is clamped to [0, 1],
    which is the loop's anti-windup. Returns dict(kp, ki)."""
    band, reset_steps = np.broadcast_arrays(np.asarray(band, dtype=np.float64), np.asarray(reset_steps, dtype=np.float64))
    kp = 1.0 / band
    return dict(kp=kp, ki=kp / reset_steps)


def with_limit(ct, kind, index, hi, lo, node=None):
    """A copy of the controller dict `ct` with a high-limit cut-out on every controller: the temperature named by kind / index /
    node as the sensed one is (kind 1: a node of surface `index`, node -1 its last — a floor's surface), u = 0 from above `hi`
    until below `lo`."""
    n = n_controllers(ct)
    one = np.ones(n)
    return dict(ct, lim_kind=(np.asarray(kind) * one).astype(np.int32), lim_index=(np.asarray(index) * one).astype(np.int32),
                lim_node=(np.asarray(-1 if node is None else node) * one).astype(np.int32), lim_hi=np.asarray(hi) * one, lim_lo=np.asarray(lo) * one)


def embed(md, surface, node, side="back"):
    """Puts controllers' outputs, in W, into nodes of walls — the pipes of a heated or cooled slab. Returns (md2, drive): md2
    a copy of the model dict whose `side` alpha row of every listed surface is 1 at its `node` and 0 elsewhere, and drive =
    dict(surface, chan_key, gain): for each listed surface s the series' driven solar input of that side must name the
    controller's channel — ``series[chan_key][0][s] = out_chan`` with ``series[chan_key][1][s] = gain`` (1 / area: the
    input is a flux per m2 of wall, which the wall multiplies by its area and its alpha row). The back side's value is
    not clamped at zero, so a negative output (out_hi < out_lo = 0) cools the node; the FRONT side's is clamped: embed a
    cooled slab through side="back". A NaN value of either side becomes 0 in the wall: a NaN output is no failure there.
    The side's own absorbed short-wave is given up: an input has one source.
    surface, node: [m] the surfaces and their nodes (-1: the last); a surface may be listed once.
    The planner's fast classes absorb at the two face nodes only. A wall whose alpha is not 0 off its face nodes is none of
    them: the planner routes it to the general class (the fifth count of heat_batch_class_counts and of heat_plan_check's
    summary), which applies the whole alpha row — correct, and slower per wall. drive["general"] counts the listed walls
    embedded off the side's face node: the fifth count of binding.plan_check(md2) exceeds that of plan_check(md) by those of
    them that were in another class before, and the tests hold the planner to it (tests/test_controllers_host.py)."""
    if side not in ("front", "back"):
        raise ValueError("embed: side %r is neither 'front' nor 'back'" % (side,))
    surface = np.atleast_1d(np.asarray(surface, dtype=np.int64))
    off = np.asarray(md["node_offset"], dtype=np.int64)
    count = np.diff(off)[surface]
    node = np.broadcast_to(np.asarray(node, dtype=np.int64), surface.shape)
    node = np.where(node < 0, count - 1, node)
    if len(np.unique(surface)) != len(surface):
        raise ValueError("embed: a surface is listed twice")
    if ((node < 0) | (node >= count)).any():
        raise ValueError("embed: a node outside its surface")
    key = "%s_alpha" % side
    alpha = np.array(md[key], dtype=np.float64)
    for s, i in zip(surface, node):
        alpha[off[s]:off[s + 1]] = 0.0
        alpha[off[s] + i] = 1.0
    md2 = dict(md)
    md2[key] = alpha
    face = np.zeros_like(count) if side == "front" else count - 1
    return md2, dict(surface=surface, chan_key="solar_%s" % side, gain=1.0 / np.asarray(md["area"], dtype=np.float64)[surface],
                     general=int((node != face).sum()))
