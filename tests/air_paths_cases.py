"""The cases of the air-path tests (include/heat_amd.h, heat_air_paths), shared by tests/test_air_paths_host.py — which runs
them through the CPU oracle alone and asserts that they exercise the controllers — and tests/test_air_paths_gpu.py.

The expected result is DEFINED by `loop_with_rules`: per step the zone loads' rule (host_rule of tests/test_zone_loads_gpu.py),
then heat_amd.air_paths.apply, on the zone temperatures the march call before returned; the driven inputs written; one march
call. No device is needed to build a case or to run the loop through the oracle."""
import numpy as np

from heat_amd import air_paths, modeldict as mdl
from test_series_gpu import MODELS, probes_of_every_kind, random_drives, term_row, write_inputs, zone_terms
from test_zone_loads_gpu import host_rule, n_thermostats, random_loads, start_modes

HUB_PATHS = 70
SEED = 61


def random_air(md, st, rng, n_steps, channel):
    """Appends the paths' channels to `channel` and returns (channel, air, info). The paths: two to three per zone with zone
    sources and supply-air (-1) sources, about half of them controlled with both senses; one zone that receives HUB_PATHS; one
    zone in seven that receives none; an uncontrolled chain A -> B -> C; a pair A <-> B (a doorway); a controlled path whose
    setpoint channel holds a NaN at some steps. The whole list is shuffled. Setpoints are drawn around the zones' starting
    temperatures, as random_loads draws its thermostat setpoints; supply temperatures around them too, so that the source of a
    vent helps at some steps and not at others. info: the paths' numbers after the shuffle (chain, pair, nan) and the zones."""
    Z = int(md["n_zones"])
    T0 = st[md["zone_slot"]]
    t_mid, t_dev = float(np.median(T0)), float(max(np.std(T0), 0.25))
    c0 = channel.shape[1]
    n_vol, n_temp, n_set = 2, 3, 4
    volume = rng.uniform(0.0, 0.05, (n_steps, n_vol))
    supply = t_mid + rng.uniform(-4.0, 4.0, (n_steps, n_temp)) * t_dev
    # (setpoint channels 0-1 are the cooling vents', drawn rather below the zones, 2-3 the heating vents', rather above: a vent
    # also needs a source that helps, and with setpoints in the middle too few of them would ever open)
    setpoint = t_mid + np.concatenate([rng.uniform(-2.5, 1.0, (n_steps, 2)), rng.uniform(-1.0, 2.5, (n_steps, 2))], axis=1) * t_dev
    nan_set = t_mid + rng.uniform(-1.5, 1.5, n_steps) * t_dev
    nan_set[np.array([5, 6, 7, 15]) % n_steps] = np.nan
    channel = np.concatenate([channel, volume, supply, setpoint, nan_set[:, None]], axis=1)
    c_vol, c_temp, c_set, c_nan = c0, c0 + n_vol, c0 + n_vol + n_temp, c0 + n_vol + n_temp + n_set
    chain, pair, hub, nan_zone = (4, 5, 6), (8, 9), 1, 11
    none = np.arange(Z) % 7 == 3

    def other(z, n):  # n source zones, none of them z
        return (z + 1 + rng.integers(0, Z - 1, n)) % Z

    target, source = [], []
    for z in range(Z):
        if none[z] or z == hub:
            continue
        k = int(rng.integers(2, 4))
        target += [z] * k
        source += list(np.where(rng.random(k) < 0.35, -1, other(z, k)))
    target += [hub] * HUB_PATHS
    source += list(np.where(rng.random(HUB_PATHS) < 0.3, -1, other(hub, HUB_PATHS)))
    target, source = np.array(target, np.int32), np.array(source, np.int32)
    n = len(target)
    controlled = rng.random(n) < 0.5
    sense = np.where(rng.random(n) < 0.5, 1, -1)
    parts = [dict(target=target, source=source,
                  temp_chan=np.where(source < 0, c_temp + rng.integers(0, n_temp, n), -1),
                  volume_chan=c_vol + rng.integers(0, n_vol, n), volume_gain=rng.uniform(0.5, 1.5, n),
                  open_chan=np.where(controlled, c_set + np.where(sense > 0, 0, 2) + rng.integers(0, 2, n), -1),
                  sense=sense, band=rng.uniform(0.0, 0.6, n) * t_dev,
                  min_delta=rng.uniform(0.0, 0.3, n) * t_dev),
             dict(target=[chain[1], chain[2]], source=[chain[0], chain[1]], volume_chan=[c_vol, c_vol + 1]),
             air_paths.doorway(pair[0], pair[1], c_vol, 1.25),
             dict(target=[nan_zone], source=[-1], temp_chan=[c_temp], volume_chan=[c_vol], open_chan=[c_nan], sense=[1],
                  band=[0.1 * t_dev], min_delta=[0.0])]
    air = air_paths.concat(*parts)
    total = len(air["target"])
    perm = rng.permutation(total)
    air = {key: a[perm] for key, a in air.items()}
    where = np.argsort(perm)
    info = dict(chain=(int(where[n]), int(where[n + 1])), pair=(int(where[n + 2]), int(where[n + 3])), nan=int(where[n + 4]),
                chain_zones=chain, pair_zones=pair, hub=hub, none=np.flatnonzero(none), nan_steps=np.flatnonzero(np.isnan(nan_set)))
    return channel, air, info


def case(model, n_steps, n_sub, form, seed, with_loads=True):
    md, st = MODELS[model]()
    rng = np.random.default_rng(seed)
    channel, drives = random_drives(md, rng, n_steps)
    probes = np.concatenate([probes_of_every_kind(md, rng), md["zone_slot"]]).astype(np.int64)
    a0, b0 = zone_terms(md, rng, n_steps, form)
    loads = None
    if with_loads:
        channel, loads = random_loads(md, st, rng, n_steps, channel)
    channel, air, info = random_air(md, st, rng, n_steps, channel)
    w = mdl.weather_series(n_steps * n_sub, md["dt"]).reshape(n_steps, n_sub, 3)
    return dict(md=md, st=st, channel=channel, drives=drives, probes=probes, a0=a0, b0=b0, loads=loads, air=air, info=info, w=w,
                n_sub=n_sub, n_steps=n_steps)


def start_air(air, state=None):
    n = air_paths.n_paths(air)
    return dict(state=np.zeros(n, np.uint8) if state is None else np.array(state, dtype=np.uint8), sum_q=np.zeros(n),
                steps_open=np.zeros(n, np.int64), switches=np.zeros(n, np.int64))


def loop_with_rules(march, c, state, steps=slice(None), acc=None, modes=None):
    """The definition: per step the zone loads' rule, then the air paths' rule, on the zone temperatures the state holds; the
    inputs written; one march call. march(state, weather of the step, a0, b0). Returns a dict: trace, applied, modes, path_q
    and the paths' state, sum_q, steps_open, switches, states (the state bytes after every step)."""
    md, channel, loads, air = c["md"], c["channel"], c["loads"], c["air"]
    ks = range(c["n_steps"])[steps]
    acc = start_air(air) if acc is None else {k: v.copy() for k, v in acc.items()}
    if modes is None:
        modes = start_modes(loads) if loads else np.zeros(0, np.uint8)
    nt = n_thermostats(loads) if loads else 0
    trace, applied = np.zeros((len(ks), len(c["probes"]))), np.zeros((len(ks), nt))
    path_q = np.zeros((len(ks), air_paths.n_paths(air)))
    states = np.zeros(path_q.shape, np.uint8)
    for j, k in enumerate(ks):
        T = state[md["zone_slot"]]
        za, zb = term_row(c["a0"], k), term_row(c["b0"], k)
        if loads:
            za, zb, applied[j] = host_rule(T, channel[k], za, zb, loads, modes)
        before = acc["state"].copy()
        za, zb, path_q[j] = air_paths.apply(T, channel[k], za, zb, air, acc["state"])
        air_paths.accumulate(path_q[j], acc["state"], before, air, acc["sum_q"], acc["steps_open"], acc["switches"])
        states[j] = acc["state"]
        write_inputs(md, state, k, channel, c["drives"])
        march(state, c["w"][k], za, zb)
        trace[j] = state[c["probes"]]
    return dict(trace=trace, applied=applied, modes=modes, path_q=path_q, states=states, **acc)


def coverage(air, out):
    """What the controllers did in a run of loop_with_rules: (share of the controlled step-paths that are open, share of the
    controlled paths that switch at least once, the senses of the switching paths)."""
    ctl = air["open_chan"] >= 0
    open_share = float(out["states"][:, ctl].mean())
    switching = ctl & (out["switches"] > 0)
    return open_share, float(switching.sum()) / float(ctl.sum()), set(int(s) for s in air["sense"][switching])
