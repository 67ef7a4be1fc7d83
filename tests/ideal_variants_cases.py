"""Cases for every ideal-loads instantiation of the cluster-resident march (tests/test_ideal_variants_host.py,
tests/test_ideal_variants_gpu.py, tests/ideal_resident_queue_worker.py). Importable without a GPU.

k_surfaces_fast has 18 IDEAL instantiations (kernels.hip, launch_surfaces_fused): blocking factor M in {4, 8, 16} x no-mass
facings nm in {0, 1} x 4 or 8 wavefronts per workgroup, and M x 4 or 8 wavefronts for the mixed workgroups (small-surface
wavefronts beside wall wavefronts). Which one a batch reaches follows from its plan: the class c of its workgroups and the
list g2 they are in (batch.hip, enqueue_fused): M = kFastM[c]; mixed if g2 >> 1, else nm = kFastNM[c]; 8 wavefronts if g2 & 1.
CASES names one small model per instantiation and the (class, list) -> workgroups its plan has; the host test holds the plan
to that and the union of the cases to all 18, so a change of the planner's cost model shows there and not as a GPU test that
quietly marches another kernel.

The inputs come from the reference itself (build): on models this small, setpoints placed around the INITIAL zone temperatures
and capacities drawn from a fixed range leave heating, cooling or saturation out."""
import functools

import numpy as np

import helpers
from heat_amd import modeldict as mdl
from ideal_loads_ref import cpu_series
from test_series_gpu import probes_of_every_kind, random_drives, zone_terms
from test_zone_loads_gpu import random_loads

CALLS = [(2, 24), (20, 8)]        # (n_sub, n_steps): the two call lengths every case is marched at


def with_facings(md, st, every=3):
    """Every `every`-th wall of a modeldict.partitioned_buildings model becomes a massive core between two no-mass facings, as
    modeldict.ragged_mixed builds them: first and last node without mass, their neighbours half an element's mass, u of the
    first and the second-to-last segment from U[0.5, 3], both emissivities x 0.2 / 0.9 (the no-mass update stays in its
    convergent regime). In place; returns (md, st)."""
    return helpers.faced_buildings(md, st, every=every)


def faced_walls(md, every=3):
    return np.flatnonzero(np.arange(int(md["n_surfaces"])) % every == 0)


def pb(S, n, rooms, faced=False, **kw):
    def make():
        md, st = mdl.partitioned_buildings(S, n, rooms=rooms, seed=18, **kw)
        return with_facings(md, st) if faced else (md, st)
    return make


def windows(S, Z, **kw):
    return lambda: mdl.rooms_with_windows(S, Z=Z, seed=6, **kw)


# case -> (model, nodes_per_lane, {(class, list): workgroups} as planned). Every batch with fuse_always=True.
CASES = {}
for _M, _n, (_c0, _c1) in ((4, 16, (1, 4)), (8, 32, (7, 10)), (16, 64, (13, 16))):
    for _w, _S, _rooms, _g2 in ((4, 96, 4, 0), (8, 192, 8, 1)):
        CASES["M%d-nm0-%dw" % (_M, _w)] = (pb(_S, _n, _rooms), _M, {(_c0, _g2): 2})
        CASES["M%d-nm1-%dw" % (_M, _w)] = (pb(_S, _n, _rooms, faced=True), _M, {(_c1, _g2): 2})
_W240 = windows(240, 8, n_lo=16, n_hi=32)
_W160 = windows(160, 8, n_lo=32, n_hi=64)
CASES["M4-mixed-4w"] = (windows(120, 8), 4, {(5, 2): 4})
CASES["M4-mixed-8w"] = (_W240, 4, {(5, 3): 4})
CASES["M8-mixed-4w"] = (_W240, 8, {(11, 2): 4})
CASES["M8-mixed-8w"] = (_W160, 8, {(11, 2): 2, (11, 3): 2})
CASES["M16-mixed-4w"] = (_W160, 16, {(16, 2): 4})
CASES["M16-mixed-8w"] = (windows(300, 6, n_lo=32, n_hi=64), 16, {(16, 3): 3})
INSTANTIATIONS = sorted(CASES)    # the 18 rows: one case per instantiation
# gas cavities (double glazing) in mixed workgroups, at both blocking factors that allow them; 32 zones in one workgroup
_GLAZING = lambda: mdl.glazing_cavity(300, Z=4, seed=7)
CASES["glazing-4"] = (_GLAZING, 4, {(5, 2): 2, (5, 3): 2})
CASES["glazing-8"] = (_GLAZING, 8, {(11, 2): 4})
CASES["zones32"] = (lambda: mdl.partitioned_buildings(192, 8, rooms=8, walls_per_room=6, seed=18), 8, {(7, 0): 1})
# the work queue (tests/ideal_resident_queue_worker.py): lists of more blocks than the three workgroups of HEAT_AMD_FUSED_ROOM=3
CASES["queue-mixed-8w"] = (_W240, 4, {(5, 3): 4})
CASES["queue-nm1-8w"] = (pb(480, 32, 8, faced=True), 8, {(10, 1): 5})


def options_of(name):
    return dict(nodes_per_lane=CASES[name][1], fuse_always=True)


@functools.lru_cache(maxsize=None)
def model_of(name):
    """(md, st) of a case, built once; nothing of it is written afterwards (the tests copy the state)."""
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def plan_of(name):
    return helpers.plan_lists(model_of(name)[0], **options_of(name))


def inputs(name, n_steps, n_sub, seed=None):
    """The drives, zone terms and zone loads of test_ideal_loads_gpu.ideal_case on the case's model."""
    md, st = model_of(name)
    # (the seed is an input like the others: with thousands of sub-timesteps compared against a capacity, one draw in a few
    # puts some `need` within 1e-7 S of its capacity in one of the cases; with this one the smallest margin of all is 1.8e-6)
    rng = np.random.default_rng(600 + n_sub if seed is None else seed)
    channel, drives = random_drives(md, rng, n_steps)
    a0, b0 = zone_terms(md, rng, n_steps, 2)
    channel, loads = random_loads(md, st, rng, n_steps, channel)
    probes = np.unique(np.concatenate([probes_of_every_kind(md, rng), md["zone_slot"]])).astype(np.int64)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    return rng, channel, drives, probes, a0, b0, loads, w


class Case:
    """args: (md, st, channel, drives, probes, a0, b0, loads, ideal, w), as ideal_case returns them; opts: the batch options
    beside the opt-in; ref, ref_state: the CPU reference of exactly these inputs and the state it ends in."""


_built = {}


def build(oracle, name, n_steps, n_sub, seed=None, caps="reference"):
    """An ideal load on EVERY zone, in shuffled order, cycling heating only, cooling only and both, its setpoints and
    capacities placed from the reference itself:
    1. the reference without ideal loads gives every zone's free trajectory;
    2. a zone's heating setpoint is the median of that trajectory + 0.7 K in the first half of the steps and - 1.5 K in the
       second, its cooling setpoint 1 K above — so every zone crosses its setpoints whatever it floats at;
    3. the reference with unlimited loads gives every load's power per sub-timestep; every second load's heating capacity and
       the other loads' cooling capacity is 0.9 x the median of the non-zero powers of that sign — so a limited load saturates
       in about half the sub-timesteps it acts in, and need stays clear of the capacity.
    (0.7, 1.5, 1 and 0.9 are choices of input, not tolerances: tests/test_ideal_variants_host.py decides whether they still
    discriminate.) caps="none": step 3 left out, every load unlimited and no reference kept. Built once per argument set."""
    key = (name, n_steps, n_sub, seed, caps)
    if key in _built:
        return _built[key]
    md, st = model_of(name)
    rng, channel, drives, probes, a0, b0, loads, w = inputs(name, n_steps, n_sub, seed)
    Z = int(md["n_zones"])
    free = cpu_series(oracle, md, st.copy(), w, n_sub, channel, drives, md["zone_slot"], loads, dict(zone=np.zeros(0, np.int32)), a0, b0)
    night = (np.arange(n_steps) >= n_steps // 2)[:, None]
    heat_sp = np.median(free["trace"], axis=0)[None, :] + np.where(night, -1.5, 0.7)
    c0 = channel.shape[1]
    channel = np.concatenate([channel, heat_sp, heat_sp + 1.0], axis=1)
    zone = rng.permutation(Z).astype(np.int32)
    kind = np.arange(Z) % 3                                        # heating only, cooling only, both
    ideal = dict(zone=zone, heat_chan=np.where(kind != 1, c0 + zone, -1).astype(np.int32),
                 cool_chan=np.where(kind != 0, c0 + Z + zone, -1).astype(np.int32))
    c = Case()
    c.name, c.opts, c.ref, c.ref_state = name, options_of(name), None, None
    if caps == "reference":
        q = cpu_series(oracle, md, st.copy(), w, n_sub, channel, drives, probes, loads, ideal, a0, b0)["q_sub"].reshape(-1, Z)
        med = lambda v: 0.9 * float(np.median(v)) if len(v) else np.inf
        limited = np.arange(Z) % 2 == 0
        ideal["heat_cap"] = np.array([med(q[:, i][q[:, i] > 0]) if limited[i] else np.inf for i in range(Z)])
        ideal["cool_cap"] = np.array([np.inf if limited[i] else med(-q[:, i][q[:, i] < 0]) for i in range(Z)])
        c.ref_state = st.copy()
        c.ref = cpu_series(oracle, md, c.ref_state, w, n_sub, channel, drives, probes, loads, ideal, a0, b0)
    else:
        assert caps == "none", caps
    c.args = (md, st, channel, drives, probes, a0, b0, loads, ideal, w)
    _built[key] = c
    return c


def preconditions(ref):
    """What hold_to_the_reference (tests/test_ideal_resident_gpu.py) asks of a reference before it compares anything: every
    branch of the rule taken, saturation in part of the acting sub-timesteps of both directions, a thermostat that acts, and
    no sub-timestep with `need` within 1e-7 S of a capacity. Returns {name: holds}."""
    return {"heats": ref["n_heat"] > 0, "cools": ref["n_cool"] > 0, "floats": ref["n_free"] > 0,
            "heating saturates in part": 0 < ref["n_sat_heating"].sum() < ref["n_heat"],
            "cooling saturates in part": 0 < ref["n_sat_cooling"].sum() < ref["n_cool"],
            "a thermostat acts": bool((ref["applied"] != 0).any()), "margin": ref["margin"] > 1e-7}
