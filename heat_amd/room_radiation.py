"""Room radiation of a series on the host (include/heat_amd.h, heat_room_radiation): the rule the device applies to every
emitter side and every receiver at every step, in numpy, and a convenience that builds the lists of the common case. No
device, no library.

emitted() and irradiance() ARE the contract's rule, line for line — every product and sum one rounded f64 operation in the
header's order (numpy never fuses a multiply-add) — and so the reference of the tests: a host that downloads the state before
every heat_batch_march_ex call, applies them to the face nodes and writes the values into the long-wave slots gets the bits of
heat_batch_march_series_radiation.
The reference has no counterpart: its harness feeds EnergyPlus' long-wave columns plus the own-face term."""
import numpy as np

from . import modeldict as mdl

SIGMA = 5.670374419e-8


def emitted(T_face):
    """E = SIGMA (T + 273.15)^4 of face node temperatures in degrees C, any shape:
    tk = T + 273.15;  t2 = tk * tk;  t4 = t2 * t2;  E = SIGMA * t4"""
    with np.errstate(invalid="ignore", over="ignore"):
        tk = np.asarray(T_face, dtype=np.float64) + 273.15
        t2 = tk * tk
        t4 = t2 * t2
        return SIGMA * t4


def rad_temperature(v):
    """(v / SIGMA)^0.25 - 273.15: what the device makes of a raw long-wave value (surface.rs:647,692)."""
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.sqrt(np.asarray(v, dtype=np.float64) / SIGMA)) - 273.15


def irradiance(E, row, n_receivers, en_receiver, en_surface, en_side, en_factor, en_chan=None, gain=None):
    """The raw long-wave value of every receiver: [..., n_receivers].
    E       [..., 2, n_surfaces] from emitted(): side 0 the first node of every surface, side 1 its last (only the emitters
            the entries name are read)
    row     [..., n_channels] the step's row of the channel table, or None where no entry is a channel
    the entries as heat_room_radiation has them, in the caller's order:
            v = 0.0;  per entry of the receiver:  x = en_factor[i] * (E or row[en_chan[i]]);  v = v + x
    gain    None, or [n_receivers]: the series' ir_front_gain / ir_back_gain of each receiver's side (v = v * gain)"""
    E = np.asarray(E, dtype=np.float64)
    R = int(n_receivers)
    rec = np.asarray(en_receiver, dtype=np.int64).reshape(-1)
    surf = np.asarray(en_surface, dtype=np.int64).reshape(-1)
    side = np.asarray(en_side, dtype=np.int64).reshape(-1)
    factor = np.asarray(en_factor, dtype=np.float64).reshape(-1)
    is_chan = surf < 0
    lead = E.shape[:-2]
    if is_chan.any():
        row = np.asarray(row, dtype=np.float64)
        chan = np.asarray(en_chan, dtype=np.int64).reshape(-1)
        lead = np.broadcast_shapes(lead, row.shape[:-1])
    v = np.zeros(lead + (R,))
    # entry j of every receiver at once: the chain of one receiver stays sequential in the caller's order
    order = np.argsort(rec, kind="stable")
    k = rec[order]
    start = np.flatnonzero(np.r_[True, k[1:] != k[:-1]]) if len(k) else np.zeros(0, np.int64)
    rank = np.arange(len(k)) - np.repeat(start, np.diff(np.r_[start, len(k)]))
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(rank.max()) + 1 if len(k) else 0):
            i = order[rank == j]
            e, c = i[~is_chan[i]], i[is_chan[i]]
            if len(e):
                x = factor[e] * E[..., side[e], surf[e]]
                v[..., rec[e]] = v[..., rec[e]] + x
            if len(c):
                x = factor[c] * row[..., chan[c]]
                v[..., rec[c]] = v[..., rec[c]] + x
        if gain is not None:
            v = v * np.asarray(gain, dtype=np.float64)
    return v


def face_slots(md, surface, side):
    """The state slot of the face node of every (surface, side): the surface's first node for side 0, its last for side 1."""
    surface, side = np.asarray(surface, dtype=np.int64), np.asarray(side, dtype=np.int64)
    first = np.asarray(md["first_node_slot"], dtype=np.int64)[surface]
    return first + side * (np.diff(np.asarray(md["node_offset"], dtype=np.int64))[surface] - 1)


def exchange_by_area(md, weight=None):
    """The lists of the common case: every side that faces zone z is a receiver and sees every side that faces z, itself
    included, with factor w_j A_j / sum_z(w A) — the area-weighted mean of the room's emissions (the mean radiant temperature
    method). The factors of a receiver sum to 1; without weights A_i F_ij = A_j F_ji, with them
    w_i A_i F_ij = w_j A_j F_ji. weight: None, [n_surfaces] (both sides of a surface alike) or [2, n_surfaces], e.g. the
    emissivities. A convenience, like solar_gains.distribute_by_area — not part of the contract.
    Returns a dict of rc_surface, rc_side, en_receiver, en_surface, en_side, en_factor (receivers zone-major, fronts before
    backs; a receiver's entries in the order of the receivers): the arguments of make_room_radiation."""
    S = int(md["n_surfaces"])
    area = np.asarray(md["area"], dtype=np.float64)
    w = np.ones((2, S)) if weight is None else np.broadcast_to(np.asarray(weight, dtype=np.float64), (2, S))
    faces = [(np.asarray(md["front_kind"]) == mdl.SPACE, np.asarray(md["front_zone"], dtype=np.int64)),
             (np.asarray(md["back_kind"]) == mdl.SPACE, np.asarray(md["back_zone"], dtype=np.int64))]
    surf = np.concatenate([np.flatnonzero(is_space) for is_space, _ in faces])
    side = np.concatenate([np.full(int(is_space.sum()), s, np.uint8) for s, (is_space, _) in enumerate(faces)])
    zone = np.concatenate([z[is_space] for is_space, z in faces])
    order = np.argsort(zone, kind="stable")
    surf, side, zone = surf[order], side[order], zone[order]
    R = len(surf)
    wa = w[side.astype(np.int64), surf] * area[surf]
    Z = int(md["n_zones"])
    total = np.zeros(Z)
    np.add.at(total, zone, wa)
    count = np.bincount(zone, minlength=Z)
    first = np.r_[0, np.cumsum(count)][:-1]           # first receiver of every zone
    n_of = count[zone]                                # entries of every receiver: the members of its zone
    en_receiver = np.repeat(np.arange(R, dtype=np.int64), n_of)
    at = np.arange(len(en_receiver)) - np.repeat(np.r_[0, np.cumsum(n_of)][:-1], n_of)
    member = np.repeat(first[zone], n_of) + at
    return dict(rc_surface=surf.astype(np.int64), rc_side=side.astype(np.uint8), en_receiver=en_receiver,
                en_surface=surf[member].astype(np.int64), en_side=side[member].astype(np.uint8),
                en_factor=wa[member] / total[zone[member]])
