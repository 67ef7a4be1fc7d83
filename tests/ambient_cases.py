"""Cases of the ambient tests (tests/test_ambient_series_host.py asserts their coverage on the CPU, tests/test_ambient_series_gpu.py
marches them): models of heat_amd/modeldict.py with a share of the back sides turned to Boundary::AmbientTemperature
(helpers.ambient_backs) and, additionally, a share of those surfaces' FRONT sides, so that walls with an Ambient side on both
faces occur; a list of driven sides in random order that leaves some Ambient sides alone; a drive with gain, offset and mix on
different sides; the reference loops. No device, no library."""
import functools

import numpy as np

from helpers import ambient_backs
from heat_amd import ambient as amb, modeldict as mdl

# id -> (generator, batch options, zones per cluster where the generator has clusters); the smallest sizes at which each
# kernel family is reached (tests/test_ambient_back_gpu.py)
FAMILIES = {}
for _n in (2, 13, 32, 64):
    for _npl in (0, 4, 16):
        FAMILIES["uniform_massive-n%d-npl%d" % (_n, _npl)] = (functools.partial(mdl.uniform_massive, 420, _n, Z=6, dt=45.0, seed=3 * _n + _npl),
                                                             dict(nodes_per_lane=_npl), None)
for _name, _opts in (("planned", {}), ("force_general", dict(force_general=True)), ("no_fusion", dict(no_fusion=True)),
                     ("use_graph", dict(use_graph=True))):
    FAMILIES["ragged_mixed-" + _name] = (functools.partial(mdl.ragged_mixed, 1500, Z=15, dt=45.0, seed=20260402), _opts, None)
FAMILIES["glazing_cavity"] = (functools.partial(mdl.glazing_cavity, 400, Z=8, dt=45.0, seed=9), {}, None)
FAMILIES["clustered_massive-fuse_always"] = (functools.partial(mdl.clustered_massive, 900, Z=36, dt=45.0, seed=13), dict(fuse_always=True), 2)
FAMILIES["partitioned_buildings-8"] = (functools.partial(mdl.partitioned_buildings, 480, 20, rooms=8, dt=45.0, seed=28), {}, 8)
FAMILIES["partitioned_buildings-40-fuse_always"] = (functools.partial(mdl.partitioned_buildings, 1440, 7, rooms=40, dt=45.0, seed=47),
                                                    dict(fuse_always=True), 40)
ORACLE_FAMILIES = ("ragged_mixed-planned", "clustered_massive-fuse_always")
N_TEMPERATURE_CHANNELS = 5
# families whose first seed left a driven side that the oracle alone does not tell from an undriven one (discrimination(),
# checked on the CPU by tests/test_ambient_series_host.py): the seed they got instead
RESEEDED = {"ragged_mixed-no_fusion": 1}


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything of one family, built once; nothing of it is written afterwards (the tests copy the state)."""
    gen, opts, cluster = FAMILIES[name]
    index = sorted(FAMILIES).index(name)
    c = Case()
    c.name, c.opts, c.cluster = name, dict(opts), cluster
    md, st = gen()
    rng = np.random.default_rng(7000 + index + 100 * RESEEDED.get(name, 0))
    conv = ambient_backs(md, st, rng, 0.4)
    # additionally: the front of a share of the converted surfaces, so that both sides of a wall face an ambient temperature
    more = conv[(rng.random(len(conv)) < 0.35) & (md["front_kind"][conv] != mdl.AMBIENT)]
    md["front_kind"][more] = mdl.AMBIENT
    md["front_ambient"][more] = rng.uniform(5.0, 30.0, len(more))
    c.md, c.state, c.conv = md, st, conv
    S, Z = int(md["n_surfaces"]), int(md["n_zones"])
    c.n_steps, c.n_sub = 5 + index % 3, 2 + (2 * index) % 6
    c.weather = mdl.weather_series(c.n_steps * c.n_sub, md["dt"], wind_speed=3.5, wind_deg=200.0).reshape(c.n_steps, c.n_sub, 3)
    c.a0, c.b0 = rng.uniform(0.0, 60.0, Z), rng.uniform(0.1, 2.0, Z)
    # the driven sides: four in five of the Ambient sides, in random order
    fronts, backs = np.flatnonzero(md["front_kind"] == mdl.AMBIENT), np.flatnonzero(md["back_kind"] == mdl.AMBIENT)
    surface = np.concatenate([fronts, backs]).astype(np.int64)
    side = np.concatenate([np.zeros(len(fronts), np.uint8), np.ones(len(backs), np.uint8)])
    pick = rng.permutation(len(surface))[:max(1, 4 * len(surface) // 5)]
    c.surface, c.side = surface[pick], side[pick]
    N = len(pick)
    c.both = (md["front_kind"][c.surface] == mdl.AMBIENT) & (md["back_kind"][c.surface] == mdl.AMBIENT)
    c.descriptor = np.where(c.side == 0, md["front_ambient"][c.surface], md["back_ambient"][c.surface])
    # 1. the setter: per call the descriptor's temperature moved by 5 to 15 K, either way
    c.set_values = c.descriptor + rng.uniform(5.0, 15.0, (c.n_steps, N)) * rng.choice([-1.0, 1.0], (c.n_steps, N))
    # 2. the drive: eight channels of the series' own inputs (test_series_gpu.random_drives), then the temperature channels
    c.channel = np.concatenate([rng.uniform(-60.0, 600.0, (c.n_steps, 4)), rng.uniform(300.0, 450.0, (c.n_steps, 4)),
                                rng.uniform(-8.0, 32.0, (c.n_steps, N_TEMPERATURE_CHANNELS))], axis=1)
    c.inputs = {}
    for i, key in enumerate(("solar_front", "solar_back", "ir_front", "ir_back")):
        chan = (rng.integers(0, 4, S) + (4 if i >= 2 else 0)).astype(np.int32)
        chan[rng.random(S) < 0.25] = -1
        c.inputs[key] = (chan, rng.uniform(0.5, 1.5, S))
    use = rng.integers(0, 3, (3, N))                  # gain, offset, mix: each on its own third of the sides, overlapping freely
    own_zone = np.where((c.side == 1) & (md["front_kind"][c.surface] == mdl.SPACE), md["front_zone"][c.surface], -1)
    home = np.where(md["back_kind"][c.surface] == mdl.SPACE, md["back_zone"][c.surface],
                    np.where(md["front_kind"][c.surface] == mdl.SPACE, md["front_zone"][c.surface], rng.integers(0, Z, N)))
    far = (home + Z // 2) % Z                         # a zone half the model away: in another cluster where there are clusters
    mix_zone = np.where(use[2] == 0, np.where(own_zone >= 0, own_zone, far), np.where(use[2] == 1, far, -1)).astype(np.int32)
    c.own_zone, c.home, c.far = own_zone, home, far
    c.drive = dict(surface=c.surface, side=c.side, chan=(8 + rng.integers(0, N_TEMPERATURE_CHANNELS, N)).astype(np.int32),
                   gain=np.where(use[0] == 0, rng.uniform(0.8, 1.2, N), 1.0), offset=np.where(use[1] == 0, rng.uniform(-3.0, 3.0, N), 0.0),
                   mix_zone=mix_zone, mix=np.where(mix_zone >= 0, amb.b_factor(rng.uniform(0.2, 0.9, N)), np.nan))
    first = md["first_node_slot"][c.surface]
    c.probes = np.concatenate([md["flow_front_slot"][c.surface[c.side == 0]], md["flow_back_slot"][c.surface[c.side == 1]],
                               md["hs_back_slot"][c.surface[c.both]], first, first + np.diff(md["node_offset"])[c.surface] - 1,
                               md["zone_slot"]]).astype(np.int64)
    return c


def series_kwargs(c, steps=slice(None)):
    return dict(channel=c.channel[steps], probes=c.probes, zone_a0=c.a0, zone_b0=c.b0, **c.inputs)


def write_inputs(c, state, k):
    """The series' own driven inputs before call k (test_series_gpu.write_inputs)."""
    md = c.md
    for key, (chan, gain) in c.inputs.items():
        on = chan >= 0
        state[md[key + "_slot"][on]] = gain[on] * c.channel[k, chan[on]]


def flow_slots(c):
    md = c.md
    return np.where(c.side == 0, md["flow_front_slot"][c.surface], md["flow_back_slot"][c.surface])


def set_oracle_ambient(model, c, values, which=None):
    """Writes the temperatures of the driven sides (of those in the mask `which`) into the oracle's arrays, in place."""
    on = np.ones(len(c.surface), bool) if which is None else which
    for s, key in ((0, "front_ambient"), (1, "back_ambient")):
        m = on & (c.side == s)
        model.keep[key][c.surface[m]] = values[m]


def oracle_setter_run(oracle, c, which=None, values=None):
    """n_steps marches of the oracle with the temperatures of set_values written before each (None: the descriptor's
    constants throughout). Returns (state, no-mass passes)."""
    model = oracle.OracleModel(c.md)
    ref, iters = c.state.copy(), 0
    for k in range(c.n_steps):
        if values is not None:
            set_oracle_ambient(model, c, values[k], which)
        rc, it = model.march(ref, c.weather[k], c.a0, c.b0)
        assert rc == 0
        iters += it
    return ref, iters


def discrimination(oracle, c):
    """The oracle alone: does the setter's effect show? Returns (driven run, passes, share of the driven sides whose
    convective-flow slot differs from the run with the descriptor's constants, share of the both-sides-Ambient walls with a
    driven front whose hs_back or flow_back differs from the run where only back sides moved). 'Differs': by more than ten
    times the tolerance the device is then held to (atol = rtol = 1e-9), so a device that missed a value would fail. (The flow
    of a wall without mass whose faces balance absorbed radiation against convection hardly feels its air: there the
    difference is some 1e-7 relative, still a hundred times the tolerance.)"""
    md = c.md
    driven, iters = oracle_setter_run(oracle, c, None, c.set_values)
    constant, _ = oracle_setter_run(oracle, c)
    backs_only, _ = oracle_setter_run(oracle, c, c.side == 1, c.set_values)

    def differs(a, b):
        return np.abs(a - b) > 10.0 * (1e-9 + 1e-9 * np.maximum(np.abs(a), np.abs(b)))
    flow = flow_slots(c)
    sides = differs(driven[flow], constant[flow])
    w = c.surface[c.both & (c.side == 0)]
    walls = differs(driven[md["hs_back_slot"][w]], backs_only[md["hs_back_slot"][w]]) | \
        differs(driven[md["flow_back_slot"][w]], backs_only[md["flow_back_slot"][w]])
    return driven, iters, sides, walls


def oracle_drive_series(oracle, c):
    """The definition of a driven series against the oracle: ambient.apply between the oracle's marches."""
    md = c.md
    model = oracle.OracleModel(md)
    ref, iters = c.state.copy(), 0
    trace, ambient_t = np.zeros((c.n_steps, len(c.probes))), np.zeros((c.n_steps, len(c.surface)))
    for k in range(c.n_steps):
        write_inputs(c, ref, k)
        v = amb.apply(c.drive, c.channel[k], ref[md["zone_slot"]])
        set_oracle_ambient(model, c, v)
        rc, it = model.march(ref, c.weather[k], c.a0, c.b0)
        assert rc == 0
        iters += it
        trace[k], ambient_t[k] = ref[c.probes], v
    return ref, trace, ambient_t, iters
