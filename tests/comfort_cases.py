"""The cases of the comfort tests (include/heat_amd.h, heat_comfort), shared by tests/test_comfort_host.py — which builds them on
the CPU alone and asserts their coverage on a synthetic march and through the oracle — and tests/test_comfort_gpu.py.

A case starts from blinds_cases.blinds_case (channels, sky-driven inputs, apertures, receivers, shades, blinds) and adds zone
loads with thermostats (random_loads), air paths with controlled vents (random_air) and the comfort term: sensors of every
shape, some of them the control temperature of their zone, with occupancy and an adaptive band in channels of their own. The
reference is a LOOP WITH FEEDBACK (`loop`): before march call k it reads the zone and the face temperatures the state holds,
applies heat_amd.comfort.operative / control_temperatures / accumulate — the rule in numpy —, hands the control temperatures
to the thermostat rule (host_rule), to air_paths.apply(control_T=) and to blinds.apply, writes the inputs of the step and
marches once. No device is needed to build a case."""
from types import SimpleNamespace

import numpy as np

import blinds_cases as bc
from air_paths_cases import random_air, start_air
from heat_amd import air_paths, blinds as bl, comfort as cf
from test_series_gpu import term_row, write_inputs
from test_zone_loads_gpu import host_rule, n_thermostats, random_loads, start_modes

N_STEPS = bc.N_STEPS
N_SENSORS = 300        # past one 256-lane block, not a multiple of 64
EMPTY, LONG = 1, 2     # sensor 1 has no entry, sensor 2 has N_LONG
N_LONG = 130           # longer than a wavefront
AIR_ACC = ("state", "sum_q", "steps_open", "switches")


def sensors_of(md, rng, channel, T0, n_sensors=N_SENSORS):
    """The comfort term of a case and the channel table with its three kinds of channels appended: a dict of
    binding.make_comfort's arguments (without accumulators)."""
    S, Z = int(md["n_surfaces"]), int(md["n_zones"])
    n_steps = len(channel)
    steps = np.arange(n_steps)
    centre = float(np.median(T0))
    C0 = channel.shape[1]
    occ_a = np.where((steps // 4) % 2 == 0, 1.0, np.where(steps % 2 == 0, 0.0, -1.0))        # on for four steps, off for four
    occ_b = np.where((steps + 2) % 5 < 3, rng.uniform(0.1, 2.0, n_steps), 0.0)
    # an adaptive band: limits that move with the steps, narrow enough for operative temperatures on either side and inside
    mid = np.stack([centre + 0.6 * np.sin(0.5 * steps), centre + 0.13 + 0.04 * steps], axis=1)
    half = np.array([0.31, 0.17])
    channel = np.concatenate([channel, np.stack([occ_a, occ_b], axis=1), mid - half, mid + half], axis=1)
    OCC, LO, HI = C0, C0 + 2, C0 + 4
    n = n_sensors
    i = np.arange(n)
    Zs = max(1, Z - max(1, Z // 5))                                                            # the last zones have no sensor
    zone = (i % Zs).astype(np.int32)
    # the first sensor of two zones in three controls its zone; of the others, the SECOND sensor of every other one
    control = np.where(i < Zs, zone % 3 != 2, (i < 2 * Zs) & (zone % 6 == 2)).astype(np.uint8)
    air_weight = np.where(control == 1, rng.uniform(0.0, 0.5, n), rng.uniform(0.2, 0.9, n))
    air_weight[i % 11 == 4] = 0.0
    air_weight[i % 11 == 7] = 1.0
    count = 1 + rng.integers(0, 8, n)
    if n > LONG:
        count[EMPTY], count[LONG] = 0, N_LONG
    owner = np.repeat(i, count)
    ne = len(owner)
    surface = rng.integers(0, S, ne)
    nodes = np.diff(md["node_offset"])
    light = np.flatnonzero(nodes <= 2)
    if len(light):                                                                             # no-mass and two-node walls as faces
        surface[rng.integers(0, ne, min(ne, 40))] = light[rng.integers(0, len(light), min(ne, 40))]
    if n > LONG:
        at = np.flatnonzero(owner == LONG)
        surface[at[7]] = surface[at[3]]                                                        # the same face listed twice
    side = rng.integers(0, 2, ne).astype(np.uint8)
    if n > LONG:
        side[at[7]] = side[at[3]]
    raw = rng.uniform(0.2, 1.0, ne)
    total = np.zeros(n)
    np.add.at(total, owner, raw)
    weight = raw / total[owner]
    perm = rng.permutation(ne)                                                                 # entries in shuffled order
    sensors = dict(zone=zone, air_weight=air_weight, control=control, en_sensor=owner[perm].astype(np.int32),
                   en_surface=surface[perm].astype(np.int64), en_side=side[perm], en_weight=weight[perm],
                   occ_chan=np.where(i % 3 == 0, -1, OCC + i % 2).astype(np.int32),
                   lo_chan=np.where(i % 5 == 3, -1, LO + i % 2).astype(np.int32),
                   hi_chan=np.where(i % 7 == 5, -1, HI + (i // 2) % 2).astype(np.int32))
    # ---- the pattern ----
    if n > LONG:
        assert n % 64 != 0 and n > 256 and not np.array_equal(sensors["en_sensor"], np.sort(sensors["en_sensor"]))
        per = np.bincount(sensors["en_sensor"], minlength=n)
        assert per[EMPTY] == 0 and per[LONG] == N_LONG > 64
        assert len(np.unique(zone)) < Z and np.bincount(zone[control == 1], minlength=Z).max() == 1
        both = np.bincount(zone, minlength=Z) >= 2
        assert (both & (np.bincount(zone[control == 1], minlength=Z) == 1)).any()              # two sensors, one of them controls
        assert (control[Zs:2 * Zs] == 1).any()                                                 # ... and not always the first
        assert len(light) == 0 or np.isin(sensors["en_surface"], light).any()
        faced = np.where(sensors["en_side"] > 0, np.asarray(md["back_zone"])[sensors["en_surface"]], np.asarray(md["front_zone"])[sensors["en_surface"]])
        assert (faced != zone[sensors["en_sensor"]]).any()                                     # faces of other zones
    return channel, sensors


def comfort_case(md, st, rng, n_sensors=N_SENSORS):
    """Returns the namespace of blinds_cases.blinds_case with loads, air, comfort (dicts of the binding's arguments) added and
    the channel table widened by their channels."""
    c = bc.blinds_case(md, st, rng)
    T0 = np.asarray(st)[md["zone_slot"]]
    c.channel, c.loads = random_loads(md, np.asarray(st), rng, c.n_steps, c.channel)
    c.channel, c.air, c.air_info = random_air(md, np.asarray(st), rng, c.n_steps, c.channel)
    c.channel, c.comfort = sensors_of(md, rng, c.channel, T0, n_sensors)
    c.face = cf.face_slots(md, c.comfort)
    return c


def fresh(c):
    """What a run carries at its start: the comfort accumulators, the thermostat modes, the paths' and the blinds' state."""
    return dict(comfort=cf.fresh(cf.n_sensors(c.comfort)), modes=start_modes(c.loads), air=start_air(c.air),
                blinds=bc.fresh(len(c.blinds["shade"])), ap_sum=np.zeros(len(c.gains["ap_surface"])))


def _margin(out, key, values, keep):
    v = np.abs(np.asarray(values, dtype=np.float64))[keep]
    v = v[~np.isnan(v)]
    if len(v):
        out[key] = min(out.get(key, np.inf), float(v.min()))


def loop(c, state, march, probes, a0=None, b0=None, steps=None, carry=None, sense="operative", step_base=0):
    """The loop with feedback a series with comfort replaces. march(state, k, za, zb): one march call of step k on `state`, in
    place. carry: fresh(c) or what an earlier loop returned under "carry" (copied). sense: "operative" — the controls read
    the control temperatures — or "air": they read the zone temperatures, as without control sensors. Returns a dict of the
    rows of the steps run, the carry afterwards and margin: per kind of comparison the smallest distance from a tie (the
    first step of a run from step 0 aside: its temperatures are the uploaded bits whoever marches)."""
    md, sensors = c.md, c.comfort
    steps = range(c.n_steps) if steps is None else steps
    src = fresh(c) if carry is None else carry
    carry = dict(comfort={k: v.copy() for k, v in src["comfort"].items()}, modes=src["modes"].copy(),
                 air={k: v.copy() for k, v in src["air"].items()}, blinds={k: v.copy() for k, v in src["blinds"].items()},
                 ap_sum=np.array(src["ap_sum"], dtype=np.float64))
    n, NF, NT, NP, NB = len(steps), cf.n_sensors(sensors), n_thermostats(c.loads), air_paths.n_paths(c.air), len(c.blinds["shade"])
    out = dict(trace=np.zeros((n, len(probes))), operative=np.zeros((n, NF)), mrt=np.zeros((n, NF)), applied=np.zeros((n, NT)),
               path_q=np.zeros((n, NP)), position=np.zeros((n, NB)), incident=np.zeros((n, NB)),
               transmitted=np.zeros((n, len(c.gains["ap_surface"]))), Tc=np.zeros((n, int(md["n_zones"]))), Tz=np.zeros((n, int(md["n_zones"]))), margin={},
               occupied=np.zeros((n, NF), bool), below=np.zeros((n, NF), bool), above=np.zeros((n, NF), bool))
    th = c.loads["thermostats"]
    for j, k in enumerate(steps):
        T = state[md["zone_slot"]].copy()
        row = c.channel[k]
        r, top = cf.operative(state[c.face], T, sensors)
        Tc = cf.control_temperatures(T, top, sensors) if sense == "operative" else T
        live = {} if k == 0 else out["margin"]
        out["occupied"][j], out["below"][j], out["above"][j] = cf.accumulate(top, row, sensors, carry["comfort"], step_base + k, margin=live)
        # the distances of the thermostats' and the vents' comparisons from a tie
        ts, d = Tc[th["sensor_zone"]], th["band"] / 2.0
        for chan in (th["heat_chan"], th["cool_chan"]):
            v = row[np.maximum(chan, 0)]
            _margin(live, "thermostat", np.minimum(np.abs(ts - (v - d)), np.abs(ts - (v + d))), chan >= 0)
        ctl = c.air["open_chan"] >= 0
        s_, ts_air = c.air["sense"].astype(np.float64), np.where(c.air["source"] >= 0, T[np.maximum(c.air["source"], 0)], row[np.maximum(c.air["temp_chan"], 0)])
        e = s_ * (Tc[c.air["target"]] - row[np.maximum(c.air["open_chan"], 0)])
        g = s_ * (T[c.air["target"]] - ts_air)
        half = c.air["band"] / 2.0
        _margin(live, "air", np.minimum(np.minimum(np.abs(e - half), np.abs(e + half)), np.minimum(np.abs(g - c.air["min_delta"]), np.abs(g))), ctl)
        # the rules, each on the control temperatures
        za, zb, out["applied"][j] = host_rule(Tc, row, term_row(a0, k), term_row(b0, k), c.loads, carry["modes"])
        before = carry["air"]["state"].copy()
        za, zb, out["path_q"][j] = air_paths.apply(T, row, za, zb, c.air, carry["air"]["state"], control_T=Tc)
        air_paths.accumulate(out["path_q"][j], carry["air"]["state"], before, c.air, carry["air"]["sum_q"], carry["air"]["steps_open"],
                             carry["air"]["switches"])
        before = carry["blinds"]["state"].copy()
        p, fe, fde, fge = bl.apply(c.I[k], Tc, row, c.blinds, carry["blinds"]["state"], c.f[k], c.shades, margin=live)
        bl.accumulate(p, carry["blinds"]["state"], before, carry["blinds"]["sum_position"], carry["blinds"]["steps_closed"], carry["blinds"]["switches"])
        rows, drives, tp = bc.reference_rows(c, (fe[None], fde[None], fge[None]), [k])
        write_inputs(md, state, 0, rows, drives)
        march(state, k, za, zb)
        out["trace"][j], out["operative"][j], out["mrt"][j], out["Tc"][j], out["Tz"][j] = state[probes], top, r, Tc, T
        out["position"][j], out["incident"][j], out["transmitted"][j] = p, c.I[k][c.blinds["shade"]], tp[0]
        carry["ap_sum"] = carry["ap_sum"] + tp[0]
    out["carry"] = carry
    return out


def marcher(b, w):
    """march(state, k, za, zb) through the library's per-call path."""
    return lambda state, k, za, zb: b.march(state, w[k], za, zb, outputs=b.OUT_ALL)


def oracle_marcher(m, w, count=None):
    """march(state, k, za, zb) through the oracle; count (a list) collects the no-mass passes."""
    def march(state, k, za, zb):
        rc, it = m.march(state, w[k], za, zb)
        assert rc == 0
        if count is not None:
            count.append(it)
    return march


ORACLE_SEED, ORACLE_N_SUB = 531, 3
_ORACLE = {}


def oracle_case():
    """The case of the comparison with the oracle loop: ragged_mixed(700, Z=28), three sub-timesteps, zone terms per step.
    Returns (case, weather, probes, a0, b0). tests/test_comfort_host.py asserts on the CPU that no comparison of its oracle
    loop is within the margin of a tie."""
    from heat_amd import modeldict as mdl
    from test_series_gpu import probes_of_every_kind, zone_terms
    md, st = mdl.ragged_mixed(700, Z=28, seed=1)
    rng = np.random.default_rng(ORACLE_SEED)
    c = comfort_case(md, st, rng)
    probes = probes_of_every_kind(md, rng)
    a0, b0 = zone_terms(md, rng, c.n_steps, 2)
    w = mdl.weather_series(c.n_steps * ORACLE_N_SUB, md["dt"]).reshape(c.n_steps, ORACLE_N_SUB, 3)
    return c, w, probes, a0, b0


def oracle_loop(oracle, c, w, probes, a0, b0):
    """The loop of oracle_case through the oracle, once per session (left unchanged). Returns (loop result, final state);
    the result carries the count of no-mass passes under "iters"."""
    if "loop" not in _ORACLE:
        state, iters = c.state.copy(), []
        ref = loop(c, state, oracle_marcher(oracle.OracleModel(c.md), w, iters), probes, a0, b0)
        ref["iters"] = sum(iters)
        _ORACLE["loop"] = (ref, state)
    return _ORACLE["loop"]


def series_kwargs(c, probes, a0=None, b0=None, steps=slice(None), carry=None, comfort="case", step_base=0, **more):
    """The arguments of HeatBatch.march_series for the case: blinds_cases.blinded_kwargs plus loads, air and comfort, each
    with what `carry` (a loop's, or `carried` of a series) holds for it."""
    carry = carry or {}
    kw = bc.blinded_kwargs(c, probes, a0, b0, steps, carry.get("ap_sum"), carry=carry.get("blinds"))
    loads, air = c.loads, c.air
    if "modes" in carry:
        loads = dict(loads, thermostats=dict(loads["thermostats"], mode=carry["modes"]))
    if "air" in carry:
        air = dict(air, **{k: carry["air"][k] for k in AIR_ACC})
    sensors = c.comfort if isinstance(comfort, str) else comfort
    if sensors is not None and "comfort" in carry:
        sensors = dict(sensors, resume=carry["comfort"], step_base=step_base)
    return dict(kw, loads=loads, air=air, comfort=sensors, **more)


NAMES = ("trace", "failed_step", "applied", "modes", "transmitted", "ap_sum", "air", "sunlit", "blinds", "comfort")


def named(out):
    """The tuple a series with loads, gains, air paths, shades, blinds (and comfort) returns, by name."""
    assert len(out) in (len(NAMES) - 1, len(NAMES))
    return dict(zip(NAMES, out))


def carried(got):
    """What the next series of a cut takes from named(out) of the one before."""
    return dict(comfort={k: got["comfort"][k] for k in cf.ACC if k in got["comfort"]}, modes=got["modes"],
                air={k: got["air"][k] for k in AIR_ACC}, blinds={k: got["blinds"][k] for k in ("state",) + bc.ACC}, ap_sum=got["ap_sum"])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))


def same_as_loop(ref, got, what="", close=None):
    """A loop's result against named(out) of a series: every decision, count and step exactly; the real-valued rows and sums
    bit for bit, or through close(ref, got, what) where given (the oracle loop)."""
    real = same_bits if close is None else None

    def value(r, g, name):
        if close is None:
            assert real(r, g), "%s%s: %d values differ" % (what, name, int((np.asarray(r) != np.asarray(g)).sum()))
        else:
            close(r, g, what + name)

    assert got["failed_step"] == -1
    carry = ref["carry"]
    for key in ("n_occupied", "n_below", "n_above", "step_min", "step_max", "step_max_above"):
        assert np.array_equal(carry["comfort"][key], got["comfort"][key]), "%s%s: %d differ" % (what, key, int((carry["comfort"][key] != got["comfort"][key]).sum()))
    assert np.array_equal(carry["modes"], got["modes"]), what + "thermostat modes"
    for key in ("state", "steps_open", "switches"):
        assert np.array_equal(carry["air"][key], got["air"][key]), what + "air " + key
    for key in ("state", "steps_closed", "switches"):
        assert np.array_equal(carry["blinds"][key], got["blinds"][key]), what + "blinds " + key
    assert same_bits(ref["position"], got["blinds"]["position"]), what + "position"
    assert same_bits(ref["incident"], got["blinds"]["incident"]), what + "incident"
    value(ref["operative"], got["comfort"]["operative"], "operative")
    value(ref["mrt"], got["comfort"]["mrt"], "mrt")
    for key in ("sum_operative", "min_operative", "max_operative", "deg_below", "deg_above", "max_above"):
        r, g = carry["comfort"][key], got["comfort"][key]
        assert np.array_equal(np.isinf(r), np.isinf(g)) and np.array_equal(r[np.isinf(r)], g[np.isinf(g)]), what + key
        value(r[~np.isinf(r)], g[~np.isinf(g)], key)
    value(ref["applied"], got["applied"], "applied")
    value(ref["path_q"], got["air"]["path_q"], "path_q")
    value(carry["air"]["sum_q"], got["air"]["sum_q"], "sum_q")
    value(carry["blinds"]["sum_position"], got["blinds"]["sum_position"], "sum_position")
    value(ref["transmitted"], got["transmitted"], "transmitted")
    value(carry["ap_sum"], got["ap_sum"], "ap_sum")
    value(ref["trace"], got["trace"], "trace")


def coverage(c, ref):
    """What a loop's result took of the comfort rule, as a dict of counts (asserted by the tests on their own results)."""
    occ, below, above = ref["occupied"], ref["below"], ref["above"]
    top = ref["operative"]
    lo = np.where(c.comfort["lo_chan"] >= 0, True, False)
    inside = occ & ~below & ~above & lo & (c.comfort["hi_chan"] >= 0)
    with np.errstate(invalid="ignore"):
        return _coverage(c, occ, below, above, top, inside)


def _coverage(c, occ, below, above, top, inside):
    run_min = np.minimum.accumulate(np.where(occ, top, np.inf), axis=0)
    run_max = np.maximum.accumulate(np.where(occ, top, -np.inf), axis=0)
    new_min = (np.diff(run_min, axis=0) < 0).sum(axis=0) + (run_min[0] < np.inf)
    new_max = (np.diff(run_max, axis=0) > 0).sum(axis=0) + (run_max[0] > -np.inf)
    d = np.where(above, top - c.channel[:len(top)][:, np.maximum(c.comfort["hi_chan"], 0)], -np.inf) if len(top) == len(c.channel) else None
    new_above = None
    if d is not None:
        run = np.maximum.accumulate(d, axis=0)
        new_above = (np.diff(run, axis=0) > 0).sum(axis=0) + (run[0] > -np.inf)
    return dict(occupied=int(occ.sum()), unoccupied=int((~occ).sum()), below=int(below.sum()), above=int(above.sum()), inside=int(inside.sum()),
                min_twice=int((new_min >= 2).sum()), max_twice=int((new_max >= 2).sum()),
                above_twice=int((new_above >= 2).sum()) if new_above is not None else -1)
