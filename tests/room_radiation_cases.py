"""The cases of the room radiation tests (include/heat_amd.h, heat_room_radiation), shared by tests/test_room_radiation_host.py
— which builds them on the CPU alone and asserts the coverage flags below — and tests/test_room_radiation_gpu.py.

A case starts from test_series_gpu.random_drives: eight channels and random drives. Then receivers are chosen — most sides that
face a zone, some that do not (any side may be a receiver) — and lose their long-wave channel; every receiver gets entries by
pattern: the members of its room, itself among them, sides of other zones, a channel. The rule in numpy
(heat_amd.room_radiation) applied to a state is `rule`. No device is needed to build a case."""
import numpy as np

from heat_amd import modeldict as mdl, room_radiation as rrm
from test_series_gpu import INPUTS, series_kwargs
from test_sky_gpu import GAINED

EMPTY, LONG, NOMASS, SELF = 0, 1, 2, 3     # receivers (after the shuffle) with a pattern of their own
N_LONG = 70                                # more than one wavefront's worth of entries on one lane


def nomass_surfaces(md):
    off = np.asarray(md["node_offset"], dtype=np.int64)
    heavy = np.add.reduceat((np.asarray(md["mass"]) >= 1e-5).astype(np.int64), off[:-1])
    return np.flatnonzero(heavy == 0)


def radiation_case(md, rng, n_steps, channel=None, drives=None):
    """Returns (channel, drives of the call — gains on GAINED only —, drives of the reference — ones for the NULL gains —,
    radiation: a dict of binding.make_room_radiation's arguments, info: the coverage flags)."""
    from test_series_gpu import random_drives
    S = int(md["n_surfaces"])
    if channel is None:
        channel, drives = random_drives(md, rng, n_steps)
    zone = np.concatenate([np.where(np.asarray(md["front_kind"]) == mdl.SPACE, md["front_zone"], -1),
                           np.where(np.asarray(md["back_kind"]) == mdl.SPACE, md["back_zone"], -1)]).astype(np.int64)   # [2 S] by side * S + s
    faces_zone = zone >= 0
    partition = np.flatnonzero(faces_zone[:S] & faces_zone[S:] & (zone[:S] != zone[S:]))
    pick = np.where(faces_zone, rng.random(2 * S) < 0.8, rng.random(2 * S) < 0.3)
    if len(partition):
        pick[partition[0]] = pick[S + partition[0]] = True
    keys = rng.permutation(np.flatnonzero(pick))
    if len(partition):   # (the partition's two sides stay when the list is trimmed)
        keys = np.concatenate([keys[np.isin(keys, (partition[0], S + partition[0]))], keys[~np.isin(keys, (partition[0], S + partition[0]))]])
        keys[[0, 4]], keys[[1, 5]] = keys[[4, 0]], keys[[5, 1]]
    if len(keys) % 64 == 0:
        keys = keys[:-1]
    NR = len(keys)
    rc_surface, rc_side = keys % S, (keys // S).astype(np.uint8)
    members = {z: np.flatnonzero(zone == z) for z in np.unique(zone[faces_zone])}
    light = nomass_surfaces(md)
    en = dict(en_receiver=[], en_surface=[], en_side=[], en_factor=[], en_chan=[])

    def add(r, sides, total):
        f = rng.uniform(0.5, 1.5, len(sides))
        en["en_receiver"].append(np.full(len(sides), r))
        en["en_surface"].append(sides % S)
        en["en_side"].append(sides // S)
        en["en_factor"].append(f * (total / f.sum()))
        en["en_chan"].append(np.full(len(sides), -1))

    n_self = 0
    for r, key in enumerate(keys):
        if r == EMPTY:
            continue
        if r == LONG:       # sides from anywhere: other zones, other sites
            add(r, rng.integers(0, 2 * S, N_LONG), 1.0)
            continue
        if zone[key] >= 0:
            room = members[int(zone[key])]
            sides = rng.choice(room, size=min(len(room), int(rng.integers(3, 10))), replace=False)
        else:
            sides = rng.integers(0, 2 * S, 4)
        if r == SELF or rng.random() < 0.4:
            sides = np.concatenate([sides[sides != key], [key]])
        if r == NOMASS and len(light):
            sides = np.concatenate([sides, [int(light[0]) + S * int(rng.integers(0, 2))]])
        n_self += int((sides == key).any())
        with_chan = rng.random() < 0.15 or r == SELF
        add(r, rng.permutation(sides), rng.uniform(0.85, 1.0) if with_chan else rng.uniform(0.9, 1.05))
        if with_chan:       # a radiant panel: a few per cent of a long-wave-like channel (4-7: 300-450 W/m2)
            en["en_receiver"].append(np.array([r]))
            en["en_surface"].append(np.array([-1]))
            en["en_side"].append(np.array([0]))
            en["en_factor"].append(rng.uniform(0.01, 0.08, 1))
            en["en_chan"].append(rng.integers(4, 8, 1))
    order = rng.permutation(sum(len(a) for a in en["en_receiver"]))       # entries come in any order
    dt = dict(en_receiver=np.int64, en_surface=np.int64, en_side=np.uint8, en_factor=np.float64, en_chan=np.int32)
    rad = {k: np.concatenate(v)[order].astype(dt[k]) for k, v in en.items()}
    rad.update(rc_surface=rc_surface.astype(np.int64), rc_side=rc_side)
    call, ref = {}, {}
    for name, _ in INPUTS:
        chan, gain = drives[name]
        chan = chan.copy()
        if name in ("ir_front", "ir_back"):     # an input has one source
            chan[rc_surface[rc_side == (name == "ir_back")]] = -1
        call[name] = (chan, gain if name in GAINED else None)
        ref[name] = (chan, gain if name in GAINED else np.ones(S))
    emitter = np.unique((rad["en_side"].astype(np.int64) * S + rad["en_surface"])[rad["en_surface"] >= 0])
    count = np.bincount(rad["en_receiver"], minlength=NR)
    is_light = np.zeros(S, bool)
    is_light[light] = True
    info = dict(ragged=NR % 64 != 0, crosses_a_block=NR > 256, empty=bool(count[EMPTY] == 0), long=bool(count.max() > 64),
                self_view=n_self > 0, partition=bool(len(partition)) and {int(partition[0]), int(S + partition[0])} <= set(keys.tolist()),
                nomass_emitter=bool(is_light[emitter % S].any()), emitter_no_receiver=bool((~np.isin(emitter, keys)).any()),
                channel_entry=bool((rad["en_surface"] < 0).any()), gained_receiver=bool((rc_side == 1).any()) and "ir_back" in GAINED)
    return channel, call, ref, rad, info


def face_temperatures(md, state):
    """[2, n_surfaces]: the first and the last node of every surface."""
    first = np.asarray(md["first_node_slot"], dtype=np.int64)
    return np.stack([state[first], state[first + np.diff(md["node_offset"]) - 1]])


def receiver_gain(rad, ref):
    """The gain of every receiver's long-wave input as the reference drives carry it (ones where the series has no array)."""
    return np.where(rad["rc_side"] == 1, ref["ir_back"][1][rad["rc_surface"]], ref["ir_front"][1][rad["rc_surface"]])


def receiver_slots(md, rad):
    return np.where(rad["rc_side"] == 1, md["ir_back_slot"][rad["rc_surface"]], md["ir_front_slot"][rad["rc_surface"]])


def rule(md, state, row, rad, ref):
    """heat_amd.room_radiation on a state: the raw long-wave value of every receiver, [n_receivers]."""
    return rrm.irradiance(rrm.emitted(face_temperatures(md, state)), row, len(rad["rc_surface"]), rad["en_receiver"], rad["en_surface"],
                          rad["en_side"], rad["en_factor"], rad["en_chan"], receiver_gain(rad, ref))


def radiant_kwargs(channel, call, probes, a0, b0, rad, steps=slice(None), sum_irradiance=None):
    return dict(series_kwargs(channel, call, probes, a0, b0, steps=steps), radiation=dict(rad, sum_irradiance=sum_irradiance))
