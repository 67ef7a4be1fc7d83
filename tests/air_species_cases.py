"""The cases of the air-species tests (include/heat_amd.h, heat_air_species), shared by tests/test_air_species_host.py — which
runs them through the CPU oracle alone and asserts that they open and close paths, saturate and release vents and cross a limit
— and tests/test_air_species_gpu.py. They build on the air handlers' cases: zone loads, air paths, handlers, and two species.

The expected result is DEFINED by `loop_with_rules`: per step the zone loads' rule (host_rule of tests/test_zone_loads_gpu.py),
then heat_amd.air_paths.apply, heat_amd.air_handlers.apply and heat_amd.air_species.apply, on the zone temperatures the march call
before returned and the concentrations the step before left; the driven inputs written; one march call. No device is needed to
build a case or to run the loop through the oracle.

A concentration depends on temperatures through the paths' state bytes alone, so the oracle loop — 1e-9 from the device in its
temperatures — yields the same discrete outputs wherever it yields the same states; every threshold here is a random draw, none
sits on a value the rule produces."""
import numpy as np

from heat_amd import air_handlers as ah, air_paths, air_species as asp, modeldict as mdl
import air_handlers_cases as ahc
from air_paths_cases import start_air
from test_series_gpu import term_row, write_inputs
from test_zone_loads_gpu import host_rule, n_thermostats, start_modes

SEED = 67
N_STEPS = 24
N_SPECIES = 2
AIR_ACC = ahc.AIR_ACC
DISCRETE = ("n_occupied", "step_max", "n_above", "steps_saturated")
REAL = ("conc", "sum_conc", "max_conc", "excess_above", "sum_volume", "sum_q")


def random_species(md, st, rng, n_steps, n_sub, channel):
    """Appends the species' channels to `channel` and returns (channel, species, info). Species 0 is CO2-like (an outdoor level
    from one of two channels — two weather sites —, a limit, sources that follow an occupancy pattern), species 1 moisture-like
    (no outdoor level in one zone in four, sources and sinks, no limit). Sources are scaled by vol / h, so a source of amplitude
    A moves its zone by about A per step whatever the zone's size. Zones z % 3 == 0 have two or three vents, driven by either
    species, z % 3 == 1 one, the others none; half of the vents have an enable channel that is off at a third of the steps. The
    starting concentrations are drawn from below c_lo to above c_hi: some vents start saturated and release, others rise. The
    source and vent lists are shuffled."""
    Z = int(md["n_zones"])
    vol = np.asarray(md["zone_volume"], dtype=np.float64)
    h = float(n_sub) * float(md["dt"])
    T0 = st[md["zone_slot"]]
    t_mid, t_dev = float(np.median(T0)), float(max(np.std(T0), 0.25))
    c0 = channel.shape[1]
    outdoor = np.concatenate([rng.uniform(400.0, 450.0, (n_steps, 2)), rng.uniform(4.0, 9.0, (n_steps, 1))], axis=1)
    strength = rng.uniform(0.0, 1.0, (n_steps, 3)) * (rng.random((n_steps, 3)) < 0.7)        # an occupancy pattern: off at times
    t_out = t_mid + rng.uniform(-8.0, 4.0, (n_steps, 2)) * t_dev
    enable = (rng.random((n_steps, 1)) < 0.67).astype(np.float64)
    limit = rng.uniform(850.0, 1150.0, (n_steps, 1))
    occupied = (rng.random((n_steps, 1)) < 0.6).astype(np.float64)
    channel = np.concatenate([channel, outdoor, strength, t_out, enable, limit, occupied], axis=1)
    c_out, c_src, c_temp, c_en, c_lim, c_occ = c0, c0 + 3, c0 + 6, c0 + 8, c0 + 9, c0 + 10
    outdoor_chan = np.stack([c_out + (np.arange(Z) % 2), np.where(np.arange(Z) % 4 == 3, -1, c_out + 2)]).astype(np.int32)
    # ---- the sources: two to three per zone and species, a sink among the moisture's ----
    src_zone, src_species, amplitude = [], [], []
    for s in range(N_SPECIES):
        for z in range(Z):
            k = int(rng.integers(2, 4))
            src_zone += [z] * k
            src_species += [s] * k
            amplitude += list(rng.uniform(20.0, 160.0, k) if s == 0 else rng.uniform(-0.4, 1.2, k))
    nq = len(src_zone)
    perm = rng.permutation(nq)
    src_zone, src_species = np.array(src_zone, np.int32)[perm], np.array(src_species, np.int32)[perm]
    sources = dict(src_zone=src_zone, src_species=src_species, src_chan=(c_src + rng.integers(0, 3, nq)).astype(np.int32),
                   src_factor=np.array(amplitude)[perm] * vol[src_zone] / max(h, 1.0))
    # ---- the vents ----
    vent_zone = []
    for z in range(Z):
        vent_zone += [z] * (int(rng.integers(2, 4)) if z % 3 == 0 else (1 if z % 3 == 1 else 0))
    vent_zone = rng.permutation(np.array(vent_zone, np.int32))
    nv = len(vent_zone)
    vent_species = (rng.random(nv) < 0.3).astype(np.int32)
    co2 = vent_species == 0
    v_min = np.where(rng.random(nv) < 0.3, 0.0, rng.uniform(0.0, 0.02, nv))
    vents = dict(vent_zone=vent_zone, vent_species=vent_species, vent_temp_chan=(c_temp + rng.integers(0, 2, nv)).astype(np.int32),
                 vent_enable_chan=np.where(rng.random(nv) < 0.5, c_en, -1).astype(np.int32), vent_v_min=v_min,
                 vent_v_max=v_min + rng.uniform(0.05, 0.4, nv),
                 vent_c_lo=np.where(co2, rng.uniform(500.0, 700.0, nv), rng.uniform(5.0, 7.0, nv)),
                 vent_c_hi=np.where(co2, rng.uniform(900.0, 1200.0, nv), rng.uniform(9.0, 12.0, nv)))
    conc = np.stack([rng.uniform(300.0, 1500.0, Z), rng.uniform(3.0, 15.0, Z)])
    species = dict(outdoor_chan=outdoor_chan, conc=conc, limit_chan=np.array([c_lim, -1], np.int32),
                   occ_chan=np.where(np.arange(Z) % 5 == 0, -1, c_occ).astype(np.int32), **sources, **vents)
    return channel, species, dict(h=h, n_sources=nq, n_vents=nv)


def case(model, n_steps, n_sub, form, seed, with_loads=True, with_air=True, with_handlers=True):
    c = ahc.case(model, n_steps, n_sub, form, seed, with_loads=with_loads, with_air=with_air)
    rng = np.random.default_rng(seed + 1000)
    c["channel"], c["species"], c["species_info"] = random_species(c["md"], c["st"], rng, n_steps, n_sub, c["channel"])
    if not with_handlers:
        c["handlers"] = None
    return c


def rule_args(species):
    """The species dict without what the binding alone takes."""
    return {k: v for k, v in species.items() if k not in ("conc", "stats", "resume", "step_base")}


def loop_with_rules(march, c, state, steps=slice(None), carry=None, step_base=0):
    """The definition: per step the zone loads', the air paths', the air handlers' and the air species' rules, on the zone
    temperatures the state holds and the concentrations the step before left; the inputs written; one march call.
    march(state, weather of the step, a0, b0). carry: what an earlier loop returned under "carry", copied. Returns a dict: trace,
    applied, path_q, the handlers' rows, conc_rows, vent_v, vent_q, saturated, states (the paths' bytes after every step), and
    carry (modes, air, handlers, species)."""
    md, channel, loads, air, handlers, species = c["md"], c["channel"], c["loads"], c["air"], c["handlers"], c["species"]
    ks = range(c["n_steps"])[steps]
    carry = carry or {}
    Z = int(md["n_zones"])
    modes = np.array(carry["modes"]) if "modes" in carry else (start_modes(loads) if loads else np.zeros(0, np.uint8))
    air_acc = {k: v.copy() for k, v in carry["air"].items()} if "air" in carry else start_air(air or {})
    h_acc = {k: v.copy() for k, v in carry["handlers"].items()} if "handlers" in carry else ah.fresh(handlers)
    acc = {k: v.copy() for k, v in carry["species"].items()} if "species" in carry else asp.fresh(species, Z, species.get("conc"))
    n, U, B, S, V = len(ks), ah.n_units(handlers), ah.n_branches(handlers), asp.n_species(species), asp.n_vents(species)
    rule = rule_args(species)
    out = dict(trace=np.zeros((n, len(c["probes"]))), applied=np.zeros((n, n_thermostats(loads) if loads else 0)),
               path_q=np.zeros((n, air_paths.n_paths(air))), supply_t=np.zeros((n, U)), recovered=np.zeros((n, U)), coil_q=np.zeros((n, U)),
               branch_q=np.zeros((n, B)), conc_rows=np.zeros((n, S, Z)), vent_v=np.zeros((n, V)), vent_q=np.zeros((n, V)),
               saturated=np.zeros((n, V), bool), states=np.zeros((n, air_paths.n_paths(air)), np.uint8), zone_T=np.zeros((n, Z)))
    for j, k in enumerate(ks):
        T = state[md["zone_slot"]].copy()
        za, zb = term_row(c["a0"], k), term_row(c["b0"], k)
        if loads:
            za, zb, out["applied"][j] = host_rule(T, channel[k], za, zb, loads, modes)
        if air:
            before = air_acc["state"].copy()
            za, zb, out["path_q"][j] = air_paths.apply(T, channel[k], za, zb, air, air_acc["state"])
            air_paths.accumulate(out["path_q"][j], air_acc["state"], before, air, air_acc["sum_q"], air_acc["steps_open"], air_acc["switches"])
            out["states"][j] = air_acc["state"]
        if handlers:
            za, zb, rows = ah.apply(T, channel[k], za, zb, handlers, h_acc["bypass"])
            ah.accumulate(rows, h_acc)
            for key in ah.ROWS:
                out[key][j] = rows[key]
        za, zb, rows = asp.apply(T, acc["conc"], channel[k], za, zb, rule, md["zone_volume"], float(c["n_sub"]) * float(md["dt"]), loads=loads,
                                 air=air, air_state=air_acc["state"], handlers=handlers)
        asp.accumulate(rows, acc, rule, channel[k], step_base + k)
        out["conc_rows"][j], out["vent_v"][j], out["vent_q"][j], out["saturated"][j] = rows["conc"], rows["vent_v"], rows["vent_q"], rows["saturated"]
        out["zone_T"][j] = T
        write_inputs(md, state, k, channel, c["drives"])
        march(state, c["w"][k], za, zb)
        out["trace"][j] = state[c["probes"]]
    out["carry"] = dict(modes=modes, air=air_acc, handlers=h_acc, species=acc)
    return out


def coverage(c, out):
    """What a run of loop_with_rules exercised, as a dict: the share of the controlled step-paths that are open and of the
    controlled paths that switch; of the vent-steps the saturated and the disabled share; the share of the vents that are
    saturated at some step and not at a later one where they are enabled (released); the share of the CO2 lanes above the limit
    at some step and not at another; the share of occupied lane-steps."""
    species, air = c["species"], c["air"]
    res = {}
    if air:
        ctl = np.asarray(air["open_chan"]) >= 0
        res["open"] = float(out["states"][:, ctl].mean())
        res["switching"] = float((out["carry"]["air"]["switches"][ctl] > 0).mean())
    ec = np.asarray(species["vent_enable_chan"])
    enabled = (ec[None, :] < 0) | (c["channel"][:, np.maximum(ec, 0)] > 0)
    sat = out["saturated"]
    res["saturated"] = float(sat.mean())
    res["disabled"] = float((~enabled).mean())
    first = np.where(sat.any(axis=0), sat.argmax(axis=0), len(sat))
    later = np.arange(len(sat))[:, None] > first[None, :]
    res["released"] = float((later & enabled & ~sat).any(axis=0).mean())
    res["modulating"] = float(((out["vent_v"] > np.asarray(species["vent_v_min"])) & ~sat & enabled).mean())
    limit = c["channel"][:, species["limit_chan"][0]][:, None]
    above = out["conc_rows"][:, 0, :] > limit
    res["crossing"] = float((above.any(axis=0) & (~above).any(axis=0)).mean())
    res["occupied"] = float(out["carry"]["species"]["n_occupied"].mean() / max(1, len(sat)))
    return res


def assert_coverage(cov, what=""):
    """The conditions of every case (conditions, not measurements)."""
    print("%s: %s" % (what, ", ".join("%s %.2f" % kv for kv in cov.items())))
    if "open" in cov:
        assert 0.10 <= cov["open"] <= 0.90 and cov["switching"] >= 0.20, (what, cov)
    assert 0.05 <= cov["saturated"] <= 0.80, (what, cov)
    assert 0.05 <= cov["disabled"] <= 0.40, (what, cov)
    assert cov["released"] >= 0.10 and cov["modulating"] >= 0.10, (what, cov)
    assert cov["crossing"] >= 0.20, (what, cov)
    assert 0.3 <= cov["occupied"] <= 0.95, (what, cov)


def species_with(species, acc, step_base):
    """The species' dict with what a loop's carry or a series' result holds: conc, and the accumulators as resume."""
    return dict(species, conc=acc["conc"], resume={k: acc[k] for k in asp.ACC if k in acc}, step_base=step_base)
