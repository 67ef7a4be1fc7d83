"""Every optional term of a series march in ONE call, and a plain series through every exported entry point (include/heat_amd.h,
heat_batch_march_series ... heat_batch_march_series_ambient).

The terms have tests of their own against the oracle and the per-call path; what is held here is how the call ARRANGES them: the
ten entry points forward to one implementation, and that implementation stages, marches and fetches all the terms side by side.
1. A series without any optional term gives the same bits through each of the ten symbols (a forwarder that misplaces an
   argument shows).
2. Loads, a report, sky, shades, gains, air paths, room radiation and an ambient drive together — with and without ideal loads —
   give the same bits in one call and cut in two with every memory carried.
3. The same call with none of the per-step rows asked for leaves the accumulators and the state as they were.
The cases are ambient_cases' (a few hundred to 1500 walls, 5 to 7 steps), widened by the other terms' own case builders."""
import ctypes as C
import functools

import numpy as np
import pytest

import ambient_cases as ac
import shades_cases as sc
from air_paths_cases import random_air
from heat_amd import HeatBatch, binding, modeldict as mdl, room_radiation as rrm
from heat_amd.binding import AIR_STATS, IDEAL_STATS, TH_STATS
from test_series_gpu import owned_slots
from test_zone_loads_gpu import random_loads

pytestmark = pytest.mark.gpu

CUT = 2
CASES = [("clustered_massive-fuse_always", False), ("ragged_mixed-planned", True)]
ROWS = ("trace", "applied", "group_trace", "transmitted", "path_q", "sunlit", "irradiance", "ambient_t")
Q_KEYS = ("q_min", "q_max", "q_sum", "q_n_above")
# the arguments of the ten entry points behind the batch, in the header's order
SYMBOLS = {}
SYMBOLS["heat_batch_march_series"] = ("s", "trace", "failed")
SYMBOLS["heat_batch_march_series_loads"] = ("s", "l", "trace", "applied", "failed")
SYMBOLS["heat_batch_march_series_report"] = ("s", "l", "r", "trace", "applied", "failed")
SYMBOLS["heat_batch_march_series_ideal"] = ("s", "l", "il", "r", "trace", "applied", "ideal_q", "failed")
SYMBOLS["heat_batch_march_series_sky"] = ("s", "sky", "l", "il", "r", "trace", "applied", "ideal_q", "failed")
SYMBOLS["heat_batch_march_series_gains"] = ("s", "sky", "gains", "l", "il", "r", "trace", "applied", "ideal_q", "transmitted", "failed")
SYMBOLS["heat_batch_march_series_air"] = ("s", "sky", "gains", "l", "air", "il", "r", "trace", "applied", "ideal_q", "transmitted",
                                          "path_q", "failed")
SYMBOLS["heat_batch_march_series_shaded"] = ("s", "sky", "shades", "gains", "l", "air", "il", "r", "trace", "applied", "ideal_q",
                                             "transmitted", "path_q", "sunlit", "failed")
SYMBOLS["heat_batch_march_series_radiation"] = SYMBOLS["heat_batch_march_series_shaded"][:-1] + ("radiation", "irradiance", "failed")
SYMBOLS["heat_batch_march_series_ambient"] = SYMBOLS["heat_batch_march_series_radiation"][:-1] + ("ambient", "ambient_t", "failed")
OUTPUTS = ("applied", "ideal_q", "transmitted", "path_q", "sunlit", "irradiance", "ambient_t")


def same(a, b):
    """Bit for bit (a NaN equals itself, -0.0 does not equal 0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. a plain series through each of the ten symbols ----
def test_a_plain_series_gives_the_same_bits_through_every_entry_point():
    c = ac.case("ragged_mixed-planned")
    md = c.md
    own = owned_slots(md)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    runs = {}
    for symbol, names in SYMBOLS.items():
        s, keep = binding.make_series(c.weather, c.n_sub, **ac.series_kwargs(c))
        trace = np.zeros((c.n_steps, len(c.probes)))
        untouched = {k: np.full((c.n_steps, 3), 7.0) for k in OUTPUTS}      # (no term: none of them is written, whatever its position)
        failed = C.c_int32(5)
        given = dict(s=C.byref(s), trace=dp(trace), failed=C.byref(failed), **{k: dp(v) for k, v in untouched.items()})
        state = c.state.copy()
        with HeatBatch(md) as b:
            b.upload_state(state)
            rc = getattr(b._L, symbol)(b._h, *[given.get(n) for n in names])
            b.download_state(state)
        assert rc == 0 and failed.value == -1, symbol
        assert all(np.all(v == 7.0) for v in untouched.values()), symbol
        runs[symbol] = (trace, state[own])
    first = runs["heat_batch_march_series"]
    assert np.all(np.isfinite(first[0])) and not np.array_equal(first[0][0], first[0][-1])
    assert not np.array_equal(first[1], c.state[own])
    for symbol, (trace, state) in runs.items():
        assert same(trace, first[0]) and same(state, first[1]), symbol


# ---- 2. every term in one call ----
@functools.lru_cache(maxsize=None)
def everything(name, with_ideal):
    """The ambient case `name` widened by every other term; nothing of it is written afterwards. Returns a function
    kwargs(steps, carried) -> the arguments of march_series for those steps, `carried` being what the call before returned."""
    c = ac.case(name)
    md, n_steps = c.md, c.n_steps
    Z = int(md["n_zones"])
    rng = np.random.default_rng(606)
    channel, loads = random_loads(md, c.state, rng, n_steps, c.channel)
    channel, air, _ = random_air(md, c.state, rng, n_steps, channel)
    t_mid = float(np.median(c.state[md["zone_slot"]]))
    channel = np.concatenate([channel, np.full((n_steps, 1), t_mid + 0.7), np.full((n_steps, 1), t_mid + 1.9)], axis=1)
    nc = channel.shape[1]
    zone = np.arange(0, Z, 2, dtype=np.int32)
    ideal = dict(zone=zone, heat_chan=np.full(len(zone), nc - 2, np.int32), cool_chan=np.full(len(zone), nc - 1, np.int32),
                 heat_cap=np.where(np.arange(len(zone)) % 2 == 0, 2000.0, np.inf), cool_cap=np.full(len(zone), np.inf))
    # (shades_case lays its suns out over N_SUNS steps and asserts the pattern on them: the call takes the first n_steps)
    _, call, _, args, gains, shades = sc.shades_case(md, rng, sc.N_SUNS, channel, dict(c.inputs))
    args = dict(args, record=args["record"][:n_steps].copy(), mode=args["mode"].copy())
    rad = rrm.exchange_by_area(md)
    for bit, key, kind in ((4, "ir_front", "front_kind"), (8, "ir_back", "back_kind")):   # an input has one source: the room
        chan = call[key][0].copy()
        chan[md[kind] == mdl.SPACE] = -1
        call[key] = (chan, call[key][1])
        args["mode"][md[kind] == mdl.SPACE] &= ~np.uint8(bit)
    assert (args["mode"] & 3).any() and (args["mode"] & 12).any()
    a0, b0 = c.a0[None, :] * rng.uniform(0.5, 1.5, (n_steps, 1)), c.b0[None, :] * rng.uniform(0.5, 1.5, (n_steps, 1))
    P = len(c.probes)
    group = (c.probes[rng.integers(0, P, 40)], rng.uniform(-2.0, 3.0, 40))
    hi = np.append(c.state[c.probes], np.nan)              # (counted: the steps a probe spends above its starting value)
    report = dict(stats=("min", "max", "sum", "n_above"), limits=dict(hi=hi), thermostat_stats=TH_STATS, group_trace=True, groups=[group])

    def kwargs(steps=slice(None), carried=None, **rows):
        base = steps.start or 0
        kw = sc.shaded_kwargs(channel, call, c.probes, a0, b0, args, gains, shades, steps, None if carried is None else carried["ap_sum"])
        kw.update(loads=loads, report=report, air=air, radiation=rad, ambient=c.drive, **rows)
        if with_ideal:
            kw["ideal"] = ideal
        if carried is not None:
            kw["loads"] = dict(loads, thermostats=dict(loads["thermostats"], mode=carried["modes"]))
            kw["report"] = dict(report, resume=carried["report"], step_base=base)
            kw["air"] = dict(air, **{k: carried["air"][k] for k in ("state",) + AIR_STATS})
            kw["radiation"] = dict(rad, sum_irradiance=carried["sum_irradiance"])
            kw["ambient"] = dict(c.drive, sum_temperature=carried["sum_temperature"])
            if with_ideal:
                kw["ideal"] = dict(ideal, resume=carried["ideal"], step_base=base)
        return kw
    return kwargs


def named(out):
    """The tuple a call without ideal loads returns, under the keys of the dict a call with them returns."""
    if isinstance(out, dict):
        return out
    keys = ("trace", "failed_step", "applied", "modes", "report", "transmitted", "ap_sum", "air", "sunlit", "irradiance", "sum_irradiance",
            "ambient_t", "sum_temperature")
    assert len(out) == len(keys)
    return dict(zip(keys, out))


def rows_of(out):
    return dict({k: out[k] for k in ROWS if k in out}, group_trace=out["report"]["group_trace"], path_q=out["air"]["path_q"],
                **({"ideal_q": out["ideal_q"]} if "ideal_q" in out else {}))


def accumulators_of(out):
    acc = {k: out["report"][k] for k in Q_KEYS + tuple("th_" + k for k in TH_STATS)}
    acc.update({"air_" + k: out["air"][k] for k in ("state",) + AIR_STATS})
    acc.update({k: out[k] for k in ("modes", "ap_sum", "sum_irradiance", "sum_temperature")})
    acc.update({"ideal_" + k: out["ideal"][k] for k in IDEAL_STATS} if "ideal" in out else {})
    return acc


def run(name, calls):
    """A fresh batch, the case's state uploaded, the calls made one after the other (each a function of the result before).
    Returns (the calls' results, the final state)."""
    c = ac.case(name)
    state, outs = c.state.copy(), []
    with HeatBatch(c.md, **c.opts) as b:
        if c.opts.get("fuse_always"):
            assert b.n_fused_surfaces > 0, b.class_counts()
        b.upload_state(state)
        for call in calls:
            w, kw = call(outs[-1] if outs else None)
            outs.append(named(b.march_series(w, c.n_sub, **kw)))
            assert outs[-1]["failed_step"] == -1
        b.download_state(state)
    return outs, state


@functools.lru_cache(maxsize=None)
def uncut(name, with_ideal):
    c, kwargs = ac.case(name), everything(name, with_ideal)
    (out,), state = run(name, [lambda _: (c.weather, kwargs())])
    return out, state


@pytest.mark.parametrize("name,with_ideal", CASES, ids=["fused", "streamed-ideal"])
def test_every_term_in_one_call_equals_the_call_cut_in_two(name, with_ideal):
    c, kwargs = ac.case(name), everything(name, with_ideal)
    own = owned_slots(c.md)
    one, state1 = uncut(name, with_ideal)
    assert isinstance(one, dict) and ("ideal_q" in one) == with_ideal
    (first, second), state2 = run(name, [lambda _: (c.weather[:CUT], kwargs(slice(0, CUT))),
                                         lambda before: (c.weather[CUT:], kwargs(slice(CUT, None), before))])
    r1, ra, rb = rows_of(one), rows_of(first), rows_of(second)
    assert set(r1) == set(ROWS) | ({"ideal_q"} if with_ideal else set())
    for k, v in r1.items():
        assert v.shape[0] == c.n_steps and v.shape[1] > 0, k
        assert same(v, np.concatenate([ra[k], rb[k]])), "%s: %d values differ" % (k, int((v != np.concatenate([ra[k], rb[k]])).sum()))
        # the case discriminates: the term acts, and not alike at every step
        assert np.any(np.nan_to_num(v) != 0) and not same(v[0], v[-1]), k
    a1, a2 = accumulators_of(one), accumulators_of(second)
    for k, v in a1.items():
        assert same(v, a2[k]), k
    assert same(state1[own], state2[own]) and not same(state1[own], c.state[own])
    assert one["report"]["th_switches"].sum() > 0 and one["air"]["switches"].sum() > 0
    assert ((one["sunlit"] > 0) & (one["sunlit"] < 1)).any() and (one["report"]["q_n_above"] > 0).any()


# ---- 3. none of the per-step rows asked for ----
def test_rows_not_asked_for_leave_every_other_bit():
    name, with_ideal = CASES[0]
    c, kwargs = ac.case(name), everything(name, with_ideal)
    own = owned_slots(c.md)
    one, state1 = uncut(name, with_ideal)
    off = dict(trace=False, applied=False, path_q=False, sunlit=False, irradiance=False, ambient_t=False)
    (none,), state0 = run(name, [lambda _: (c.weather, kwargs(**off))])
    for k in off:
        v = none["air"]["path_q"] if k == "path_q" else none[k]
        assert v.shape[0] == 0 and v.size == 0, k
    a1, a0 = accumulators_of(one), accumulators_of(none)
    for k, v in a1.items():
        assert same(v, a0[k]), k
    assert same(one["transmitted"], none["transmitted"]) and same(one["report"]["group_trace"], none["report"]["group_trace"])
    assert same(state1[own], state0[own])
