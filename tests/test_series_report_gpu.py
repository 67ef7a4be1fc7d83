"""Report of a series on the GPU (include/heat_amd.h, heat_batch_march_series_report): statistics, weighted group sums and
thermostat statistics maintained on the device at every step.

The expected statistics are DEFINED by `replay` and `replay_thermostats` below — the header's rules in numpy, one rounded
operation each, applied in step order to the call's own trace, group trace, applied powers and modes: the device must agree
bit for bit. A group's value is compared with math.fsum over the host's products weight * slot within the header's bound
n * 2^-52 * sum |weight * slot| (any order of n rounded products and additions, with or without contraction)."""
import math

import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, binding, modeldict as mdl
from test_series_gpu import assert_close, owned_slots, series_kwargs
from test_zone_loads_gpu import CYCLING, case, closed_form_zone, host_rule, loop_with_host_rule, start_modes

pytestmark = pytest.mark.gpu

SEGMENT, ROW = 1024, 64  # plan.hpp: kGroupSegment, kGroupRowEntries
Q_KEYS = tuple("q_" + k for k in binding.Q_STATS)
TH_KEYS = tuple("th_" + k for k in binding.TH_STATS)


def replay(values, lo=None, hi=None, step_base=0, acc=None):
    """The header's table over values [n_steps, Q], in step order. acc: the accumulators to resume from (not modified)."""
    n, Q = values.shape
    if acc is None:
        acc = dict(q_min=np.full(Q, np.inf), q_step_min=np.full(Q, -1, np.int64), q_max=np.full(Q, -np.inf),
                   q_step_max=np.full(Q, -1, np.int64), q_sum=np.zeros(Q), q_n_below=np.zeros(Q, np.int64), q_deg_below=np.zeros(Q),
                   q_n_above=np.zeros(Q, np.int64), q_deg_above=np.zeros(Q))
    a = {k: np.array(v) for k, v in acc.items()}
    lo = np.full(Q, np.nan) if lo is None else lo
    hi = np.full(Q, np.nan) if hi is None else hi
    with np.errstate(invalid="ignore"):
        for k in range(n):
            v = values[k]
            m = v < a["q_min"]
            a["q_min"][m], a["q_step_min"][m] = v[m], step_base + k
            m = v > a["q_max"]
            a["q_max"][m], a["q_step_max"][m] = v[m], step_base + k
            a["q_sum"] = a["q_sum"] + v
            m = v < lo
            a["q_n_below"][m] += 1
            a["q_deg_below"][m] = a["q_deg_below"][m] + (lo[m] - v[m])
            m = v > hi
            a["q_n_above"][m] += 1
            a["q_deg_above"][m] = a["q_deg_above"][m] + (v[m] - hi[m])
    return a


def modes_of(applied):
    """The mode after every step, from the sign of the applied power (the powers of these tests are positive)."""
    return np.where(applied > 0, 1, np.where(applied < 0, 2, 0)).astype(np.uint8)


def replay_thermostats(applied, mode_before, acc=None):
    n, nt = applied.shape
    if acc is None:
        acc = dict(th_steps_heating=np.zeros(nt, np.int64), th_steps_cooling=np.zeros(nt, np.int64), th_switches=np.zeros(nt, np.int64),
                   th_sum_heating=np.zeros(nt), th_sum_cooling=np.zeros(nt))
    a = {k: np.array(v) for k, v in acc.items()}
    prev = np.array(mode_before, dtype=np.uint8)
    modes = modes_of(applied)
    for k in range(n):
        m, p = modes[k], applied[k]
        a["th_steps_heating"][m == 1] += 1
        a["th_steps_cooling"][m == 2] += 1
        a["th_switches"][m != prev] += 1
        a["th_sum_heating"][p > 0] = a["th_sum_heating"][p > 0] + p[p > 0]
        a["th_sum_cooling"][p < 0] = a["th_sum_cooling"][p < 0] + p[p < 0]
        prev = m
    return a


def assert_same(want, got, keys, what):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(want[k], got[k]), "%s: %s differs in %d places" % (
            what, k, int((want[k] != got[k]).sum()))


def random_groups(md, rng, sizes, kinds=None):
    """Groups of the given sizes over slots of every kind, weights of both signs; a third of them without a repeat-free
    guarantee (a slot may enter a group twice)."""
    pool = owned_slots(md).astype(np.int64) if kinds is None else kinds
    return [(pool[rng.integers(0, len(pool), n)], rng.uniform(-2.0, 3.0, n)) for n in sizes]


def group_bound_check(groups, probes, trace, group_trace, what):
    """group_trace against math.fsum of the host's products, per step, within n * 2^-52 * sum |w * x|."""
    where = {int(s): i for i, s in enumerate(probes)}
    worst = 0.0
    for g, (slots, weights) in enumerate(groups):
        cols = np.array([where[int(s)] for s in slots], dtype=np.int64)
        for k in range(len(trace)):
            prod = weights * trace[k, cols] if len(cols) else np.zeros(0)
            exact = math.fsum(prod)
            bound = len(cols) * 2.0 ** -52 * math.fsum(np.abs(prod))
            err = abs(group_trace[k, g] - exact)
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
            assert err <= bound, "%s: group %d (%d entries) step %d: |%.17g - %.17g| = %.3e > %.3e" % (
                what, g, len(cols), k, group_trace[k, g], exact, err, bound)
    print("%s: worst |device - fsum| = %.3g of the bound" % (what, worst))


def limits_inside(values, rng):
    """Limits between the minimum and maximum of every quantity; a constant quantity gets limits it sits on (never crossed:
    the comparisons are strict)."""
    lo_v, hi_v = values.min(axis=0), values.max(axis=0)
    return lo_v + rng.uniform(0.2, 0.5, len(lo_v)) * (hi_v - lo_v), lo_v + rng.uniform(0.5, 0.8, len(lo_v)) * (hi_v - lo_v)


FULL = dict(stats=binding.Q_STATS, thermostat_stats=binding.TH_STATS, group_trace=True)


@pytest.mark.parametrize("model", ["ragged_mixed", "rooms_with_windows"])
def test_statistics_equal_the_rules_applied_to_the_calls_own_trace(model):
    n_steps, n_sub = 40, 2
    md, st, channel, drives, probes, a0, b0, loads, w = case(model, n_steps, n_sub, 2, 61)
    rng = np.random.default_rng(8)
    groups = random_groups(md, rng, (5, 0, 300, 1, SEGMENT + 40))
    kw = series_kwargs(channel, drives, probes, a0, b0)
    P, G = len(probes), len(groups)
    with HeatBatch(md) as b:   # a first run for the ranges the limits are chosen in
        b.upload_state(st.copy())
        trace0, _, _, _, rep0 = b.march_series(w, n_sub, loads=loads, report=dict(groups=groups, group_trace=True), **kw)
    values0 = np.concatenate([trace0, rep0["group_trace"]], axis=1)
    lo, hi = limits_inside(values0, rng)
    lo[1], hi[2] = np.nan, np.nan                         # a NaN limit never counts
    lo[P + 2], hi[P + 2] = values0[:, P + 2].min() - 1.0, values0[:, P + 2].max() + 1.0   # limits never crossed
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, applied, modes, rep = b.march_series(w, n_sub, loads=loads, report=dict(FULL, groups=groups, limits=dict(lo=lo, hi=hi)), **kw)
    assert failed == -1 and np.array_equal(trace, trace0) and np.array_equal(rep["group_trace"], rep0["group_trace"])
    values = np.concatenate([trace, rep["group_trace"]], axis=1)
    want = replay(values, lo, hi)
    assert_same(want, rep, Q_KEYS, model)
    # both branches of every rule occur, the NaN limits and the limits outside the range never count
    for k in ("q_n_below", "q_n_above"):
        assert (rep[k] > 0).any() and (rep[k] < n_steps).any() and (rep[k] == 0).any(), k
    assert rep["q_n_below"][1] == 0 and rep["q_n_above"][2] == 0 and rep["q_n_below"][P + 2] == 0 and rep["q_n_above"][P + 2] == 0
    assert (rep["q_step_min"] > 0).any() and (rep["q_step_max"] > 0).any() and (rep["q_step_min"] >= 0).all()
    assert np.all(rep["group_trace"][:, 1] == 0.0)        # the empty group
    assert_same(replay_thermostats(applied, start_modes(loads)), rep, TH_KEYS, model)
    assert np.array_equal(modes_of(applied)[-1], modes)
    assert (rep["th_switches"] > 1).any() and (rep["th_steps_heating"] > 0).any() and (rep["th_steps_cooling"] > 0).any()


def test_no_trace_and_no_applied_give_the_same_report_and_the_plain_series_state():
    n_steps, n_sub = 24, 3
    md, st, channel, drives, probes, a0, b0, loads, w = case("rooms_with_windows", n_steps, n_sub, 2, 62)
    rng = np.random.default_rng(9)
    groups = random_groups(md, rng, (9, 500, 2 * SEGMENT + 3))
    Q = len(probes) + len(groups)
    report = dict(FULL, groups=groups, limits=dict(lo=rng.uniform(15.0, 25.0, Q), hi=rng.uniform(15.0, 25.0, Q)))
    kw = series_kwargs(channel, drives, probes, a0, b0)
    plain = st.copy()
    with HeatBatch(md) as b:
        b.upload_state(plain)
        trace_p, _, applied_p, modes_p = b.march_series(w, n_sub, loads=loads, **kw)
        b.download_state(plain)
    results = []
    for want_trace, want_applied, group_trace in ((True, True, True), (False, False, True), (False, False, False), (True, False, False)):
        state = st.copy()
        with HeatBatch(md) as b:
            b.upload_state(state)
            trace, failed, applied, modes, rep = b.march_series(w, n_sub, loads=loads, report=dict(report, group_trace=group_trace),
                                                                trace=want_trace, applied=want_applied, **kw)
            b.download_state(state)
        assert failed == -1 and np.array_equal(state, plain) and np.array_equal(modes, modes_p)
        assert trace.shape == ((n_steps if want_trace else 0), len(probes)) and applied.shape[0] == (n_steps if want_applied else 0)
        if want_trace:
            assert np.array_equal(trace, trace_p)
        if want_applied:
            assert np.array_equal(applied, applied_p)
        results.append(rep)
    for rep in results[1:]:
        assert_same(results[0], rep, Q_KEYS + TH_KEYS, "without trace / applied")
    assert np.array_equal(results[0]["group_trace"], results[1]["group_trace"])
    assert_same(replay_thermostats(applied_p, start_modes(loads)), results[2], TH_KEYS, "without applied")


def test_cut_and_resume_give_the_bits_of_the_series_in_one():
    n_steps, n_sub, cut, base = 30, 2, 11, 1000
    md, st, channel, drives, probes, a0, b0, loads, w = case("ragged_mixed", n_steps, n_sub, 2, 63)
    rng = np.random.default_rng(10)
    groups = random_groups(md, rng, (3, 77, SEGMENT + 1))
    Q = len(probes) + len(groups)
    report = dict(FULL, groups=groups, limits=dict(lo=rng.uniform(10.0, 30.0, Q), hi=rng.uniform(10.0, 30.0, Q)), group_trace=False)
    one, two = st.copy(), st.copy()
    with HeatBatch(md) as b:
        b.upload_state(one)
        _, _, applied1, modes1, rep1 = b.march_series(w, n_sub, loads=loads, report=dict(report, step_base=base),
                                                      **series_kwargs(channel, drives, probes, a0, b0))
        b.download_state(one)
    with HeatBatch(md) as b:
        b.upload_state(two)
        _, _, aa, ma, ra = b.march_series(w[:cut], n_sub, loads=loads, report=dict(report, step_base=base), trace=False,
                                          **series_kwargs(channel, drives, probes, a0, b0, steps=slice(0, cut)))
        second = dict(loads, thermostats=dict(loads["thermostats"], mode=ma))
        _, _, ab, mb, rb = b.march_series(w[cut:], n_sub, loads=second, report=dict(report, step_base=base + cut, resume=ra), trace=False,
                                          **series_kwargs(channel, drives, probes, a0, b0, steps=slice(cut, None)))
        b.download_state(two)
    assert ma.any(), "no thermostat is on at the cut: the modes carry nothing over it"
    assert_same(rep1, rb, Q_KEYS + TH_KEYS, "cut at %d" % cut)
    assert np.array_equal(modes1, mb) and np.array_equal(applied1, np.concatenate([aa, ab])) and np.array_equal(one, two)
    # the cut matters: extrema on both sides of it, and steps numbered from step_base
    assert (rep1["q_step_min"] >= base + cut).any() and (rep1["q_step_min"] < base + cut).any() and (rep1["q_step_min"] >= base).all()
    assert not all(np.array_equal(ra[k], rb[k]) for k in Q_KEYS)


def test_group_sums_are_within_the_derived_bound_and_fixed_by_the_tables():
    n_steps, n_sub = 6, 2
    md, st, channel, drives, _, a0, b0, loads, w = case("rooms_with_windows", n_steps, n_sub, 2, 64)
    rng = np.random.default_rng(11)
    sizes = (1, 7, 0, ROW - 1, ROW, ROW + 1, SEGMENT - 1, SEGMENT, SEGMENT + 1, 3 * SEGMENT + 500)
    groups = random_groups(md, rng, sizes)
    # one group per kind of slot as well, and one of everything this path owns, without weights
    kinds = [mdl.node_slots(md), md["hs_front_slot"], md["flow_back_slot"], md["zone_slot"]]
    groups += [(np.asarray(k, dtype=np.int64), rng.uniform(-1.0, 1.0, len(k))) for k in kinds]
    everything = owned_slots(md).astype(np.int64)
    probes = np.unique(np.concatenate([g[0] for g in groups] + [everything]))
    kw = series_kwargs(channel, drives, probes, a0, b0)

    def run(gs, pr):
        with HeatBatch(md) as b:
            b.upload_state(st.copy())
            trace, failed, _, _, rep = b.march_series(w, n_sub, loads=loads, report=dict(groups=gs, group_trace=True),
                                                      **dict(kw, probes=pr))
        assert failed == -1
        return trace, rep["group_trace"]

    trace, gt = run(groups + [everything], probes)
    assert np.all(np.isfinite(trace)) and np.abs(trace).max() > 1.0
    group_bound_check(groups + [(everything, np.ones(len(everything)))], probes, trace, gt, "groups")
    assert np.all(gt[:, 2] == 0.0)                                        # the empty group
    assert np.array_equal(gt[:, 0], groups[0][1][0] * trace[:, np.searchsorted(probes, groups[0][0][0])])   # one entry: the product
    trace2, gt2 = run(groups + [everything], probes)                      # the same bits in a second run
    assert np.array_equal(gt, gt2) and np.array_equal(trace, trace2)
    # ... and when other groups and probes are added or removed: every second group, in another order, without probes
    keep = [9, 1, 12, 7, 3, 14]
    _, gt3 = run([(groups + [everything])[i] for i in keep], probes[:0])
    assert np.array_equal(gt[:, keep], gt3)
    # the caller's order of the entries does not matter (the tables are sorted into device order)
    perm = rng.permutation(sizes[-1])
    _, gt4 = run([(groups[9][0][perm], groups[9][1][perm])], probes[:5])
    assert np.array_equal(gt[:, 9], gt4[:, 0])


@pytest.mark.parametrize("name", sorted(CYCLING))
def test_thermostat_statistics_of_the_cycling_case(name, oracle):
    """The thermostat case of DESIGN.md §1a (tests/test_zone_loads_gpu.py, CYCLING): its switch count, so far counted on the host
    from the applied rows, comes from the device — with and without the applied rows."""
    t_out, th, setpoint = CYCLING[name]
    steps = 800
    md, st, n_sub = closed_form_zone(oracle)
    loads = dict(thermostats=dict(sensor_zone=[0], target_zone=[0], **th))
    channel = np.full((steps, 1), setpoint)
    w = np.tile([t_out, 0.0, 0.0], (steps, n_sub, 1))
    report = dict(thermostat_stats=binding.TH_STATS, stats=("min", "max"))
    reps = []
    for want_applied in (True, False):
        with HeatBatch(md) as b:
            b.upload_state(st.copy())
            trace, failed, applied, modes, rep = b.march_series(w, n_sub, loads=loads, report=report, channel=channel,
                                                                probes=md["zone_slot"], trace=want_applied, applied=want_applied)
        assert failed == -1
        reps.append(rep)
        if want_applied:
            acting = np.concatenate([[False], applied[:, 0] != 0])
            changes = int((acting[1:] != acting[:-1]).sum())
            print("%s: %d switches (%d after the first step), %d steps acting" % (name, changes, changes - int(acting[1]), int(acting.sum())))
            assert changes >= 50 and rep["th_switches"][0] == changes
            assert rep["th_steps_heating"][0] + rep["th_steps_cooling"][0] == int(acting.sum())
            assert_same(replay_thermostats(applied, [0]), rep, TH_KEYS, name)
            assert rep["q_min"][0] == trace.min() and rep["q_max"][0] == trace.max()
    assert_same(reps[0], reps[1], TH_KEYS + ("q_min", "q_max"), name)


def test_a_thermostat_of_zero_power_is_counted_by_its_mode():
    """A thermostat whose power is zero heats or cools with applied == 0: its steps and switches follow the mode bytes, not the
    powers. The modes of every step come from host_rule replayed over the traced zone temperatures (the temperatures at the
    start of step k are the state's for k = 0 and row k - 1 of the trace after that)."""
    n_steps, n_sub = 30, 2
    md, st, channel, drives, _, a0, b0, loads, w = case("ragged_mixed", n_steps, n_sub, 2, 65)
    th = {k: np.array(v) for k, v in loads["thermostats"].items()}
    heats, cools = np.flatnonzero(th["heat_chan"] >= 0), np.flatnonzero(th["cool_chan"] >= 0)
    th["heat_power"][heats[:3]] = 0.0
    th["cool_power"][cools[:3]] = 0.0
    loads = dict(loads, thermostats=th)
    zone = md["zone_slot"]
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, applied, modes, rep = b.march_series(w, n_sub, loads=loads, report=dict(thermostat_stats=binding.TH_STATS),
                                                            **series_kwargs(channel, drives, zone, a0, b0))
    assert failed == -1
    nt = len(th["sensor_zone"])
    want = dict(th_steps_heating=np.zeros(nt, np.int64), th_steps_cooling=np.zeros(nt, np.int64), th_switches=np.zeros(nt, np.int64),
                th_sum_heating=np.zeros(nt), th_sum_cooling=np.zeros(nt))
    mode = start_modes(loads)
    silent = 0
    for k in range(n_steps):
        before = mode.copy()
        T = st[zone] if k == 0 else trace[k - 1]
        power = host_rule(T, channel[k], a0[k], b0[k], loads, mode)[2]
        assert np.array_equal(power, applied[k])
        want["th_steps_heating"][mode == 1] += 1
        want["th_steps_cooling"][mode == 2] += 1
        want["th_switches"][mode != before] += 1
        want["th_sum_heating"][power > 0] = want["th_sum_heating"][power > 0] + power[power > 0]
        want["th_sum_cooling"][power < 0] = want["th_sum_cooling"][power < 0] + power[power < 0]
        silent += int(((mode != 0) & (power == 0)).sum())
    assert silent > 0, "no thermostat of zero power was ever on: the case shows nothing"
    assert np.array_equal(mode, modes)
    assert_same(want, rep, TH_KEYS, "zero powers")


def test_zone_statistics_match_the_oracle_loop(oracle):
    """q_min, q_max and the mean of the zone temperatures against the same reductions over the oracle's trace, at the project's
    1e-9 (step numbers and counts are not compared: ties and limits sit on last bits)."""
    n_steps, n_sub = 24, 3
    md, st, channel, drives, _, a0, b0, loads, w = case("ragged_mixed", n_steps, n_sub, 2, 77)
    probes = md["zone_slot"]
    m = oracle.OracleModel(md)

    def march(s, wk, za, zb):
        assert m.march(s, wk, za, zb)[0] == 0

    ref_trace, _, _ = loop_with_host_rule(march, md, st.copy(), w, channel, drives, probes, loads, a0, b0)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        _, failed, _, _, rep = b.march_series(w, n_sub, loads=loads, report=dict(stats=("min", "max", "sum")), trace=False,
                                              **series_kwargs(channel, drives, probes, a0, b0))
    assert failed == -1
    assert_close(ref_trace.min(axis=0), rep["q_min"], "zone minima")
    assert_close(ref_trace.max(axis=0), rep["q_max"], "zone maxima")
    assert_close(np.add.accumulate(ref_trace, axis=0)[-1] / n_steps, rep["q_sum"] / n_steps, "zone means")


@pytest.mark.parametrize("want_trace", [True, False])
def test_a_numerical_failure_is_reported_as_by_the_series(want_trace):
    """The NaN flow volume of tests/test_zone_loads_gpu.py: failed_step, the code and the zone, with and without a trace."""
    md, st = mdl.clustered_massive(700, Z=28, dt=45.0, seed=3)
    n_steps, j, z = 9, 5, 13
    channel = np.tile([0.02, 10.0], (n_steps, 1))
    channel[j, 0] = np.nan
    loads = dict(flows=dict(zone=[z], volume_chan=[0], temp_chan=[1]))
    report = dict(stats=("min", "sum"), groups=[md["zone_slot"]])
    for n_sub in (0, 2):
        w = mdl.weather_series(n_steps * n_sub, 45.0).reshape(n_steps, n_sub, 3) if n_sub else None
        with HeatBatch(md) as b:
            b.upload_state(st.copy())
            with pytest.raises(HeatError) as e:
                b.march_series(w, n_sub, n_steps=n_steps, loads=loads, report=report, channel=channel, probes=md["zone_slot"], trace=want_trace)
            assert e.value.failed_step == j and e.value.code == 3, str(e.value)   # HEAT_N_NAN_ZONE
            assert b.failed_surface() == (z, 3) and "zone %d" % z in str(e.value)
            if want_trace:
                assert np.all(np.isfinite(e.value.trace[:j]))
            # the batch survives: a healthy series with a report afterwards
            b.upload_state(st.copy())
            healthy = np.tile([0.02, 10.0], (n_steps, 1))
            out = b.march_series(w, n_sub, n_steps=n_steps, loads=loads, report=report, channel=healthy, probes=md["zone_slot"], trace=want_trace)
            assert out[1] == -1 and np.all(np.isfinite(out[-1]["q_sum"]))


def test_a_year_of_steps_without_a_trace():
    """35 040 steps (a year of quarter hours) x 4 000 probes: the trace the old entry points would allocate is 1.12 GB; here no
    trace exists. n_sub = 0, so every step sees the state of the start and the expected values follow by construction:
    q_sum is v added 35 040 times, one rounded addition each (the same loop in numpy), min = max = v found at the first step,
    the counts are 0 or all steps, the degree sums the same repeated addition of (v - hi)."""
    n_steps, P, base = 35040, 4000, 5
    md, st = mdl.ragged_mixed(700, Z=20, seed=5)
    probes = owned_slots(md).astype(np.int64)
    assert len(probes) >= P
    probes = probes[np.random.default_rng(3).permutation(len(probes))[:P]]
    assert n_steps * P * 8 >= 1 << 30
    v = st[probes]
    hi = np.concatenate([np.full(P, float(np.median(v))), [np.nan]])     # (the group's limit: never)
    groups = [md["zone_slot"]]
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, rep = b.march_series(None, 0, n_steps=n_steps, probes=probes, trace=False,
                                            report=dict(stats=binding.Q_STATS, groups=groups, limits=dict(lo=hi, hi=hi), step_base=base))
    assert failed == -1 and trace.size == 0
    vg = np.concatenate([v, [rep["q_min"][P]]])                         # (the group's value: checked against fsum below)
    zone_sum = math.fsum(st[md["zone_slot"]])
    assert abs(vg[P] - zone_sum) <= len(md["zone_slot"]) * 2.0 ** -52 * math.fsum(np.abs(st[md["zone_slot"]]))
    total, deg_above, deg_below = np.zeros(P + 1), np.zeros(P + 1), np.zeros(P + 1)
    with np.errstate(invalid="ignore"):
        above, below = vg > hi, vg < hi
        for _ in range(n_steps):
            total = total + vg
            deg_above[above] = deg_above[above] + (vg - hi)[above]
            deg_below[below] = deg_below[below] + (hi - vg)[below]
    assert above.any() and below.any()
    assert np.array_equal(rep["q_sum"], total) and np.array_equal(rep["q_min"], vg) and np.array_equal(rep["q_max"], vg)
    assert np.all(rep["q_step_min"] == base) and np.all(rep["q_step_max"] == base)
    assert np.array_equal(rep["q_n_above"], np.where(above, n_steps, 0)) and np.array_equal(rep["q_n_below"], np.where(below, n_steps, 0))
    assert np.array_equal(rep["q_deg_above"], deg_above) and np.array_equal(rep["q_deg_below"], deg_below)


def test_no_step_touches_nothing_and_no_sub_timestep_still_reports():
    n_steps = 6
    md, st, channel, drives, probes, a0, b0, loads, w = case("ragged_mixed", n_steps, 1, 2, 21)
    rng = np.random.default_rng(12)
    groups = random_groups(md, rng, (4, 150))
    P, G = len(probes), len(groups)
    nt = len(loads["thermostats"]["sensor_zone"])
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        # n_steps == 0, resume == 0: the caller's arrays keep what they held
        s, keep = binding.make_series(np.zeros((0, 3)), 1, **series_kwargs(channel[:0], drives, probes))
        l, lkeep = binding.make_zone_loads(**loads)
        r, rkeep = binding.make_report(n_probes=P, n_thermostats=nt, n_steps=0, groups=groups, stats=binding.Q_STATS,
                                       thermostat_stats=binding.TH_STATS, limits=dict(lo=np.zeros(P + G), hi=np.zeros(P + G)))
        for k in Q_KEYS + TH_KEYS:
            rkeep[k][:] = 7
        f = binding.C.c_int32(9)
        rc = b._L.heat_batch_march_series_report(b._h, binding.C.byref(s), binding.C.byref(l), binding.C.byref(r), None, None, binding.C.byref(f))
        assert rc == 0 and f.value == -1 and s.n_steps == 0
        assert all(np.all(rkeep[k] == 7) for k in Q_KEYS + TH_KEYS)
        state = st.copy()
        b.download_state(state)
        assert np.array_equal(state, st)
        # n_sub == 0: every step reports on the state of the start
        trace, failed, applied, modes, rep = b.march_series(None, 0, n_steps=n_steps, loads=loads,
                                                            report=dict(FULL, groups=groups, limits=dict(lo=np.full(P + G, 20.0), hi=np.full(P + G, 20.0))),
                                                            **series_kwargs(channel, drives, probes, a0, b0))
        b.download_state(state)
    assert failed == -1 and np.array_equal(state, st) and np.array_equal(trace, np.tile(st[probes], (n_steps, 1)))
    assert np.array_equal(rep["group_trace"], np.tile(rep["group_trace"][0], (n_steps, 1)))
    for g, (slots, weights) in enumerate(groups):
        prod = weights * st[slots]
        assert abs(rep["group_trace"][0, g] - math.fsum(prod)) <= len(slots) * 2.0 ** -52 * math.fsum(np.abs(prod))
    values = np.concatenate([trace, rep["group_trace"]], axis=1)
    assert_same(replay(values, np.full(P + G, 20.0), np.full(P + G, 20.0)), rep, Q_KEYS, "n_sub = 0")
    assert_same(replay_thermostats(applied, start_modes(loads)), rep, TH_KEYS, "n_sub = 0")
    want_modes = start_modes(loads)
    want = np.array([host_rule(st[md["zone_slot"]], channel[k], a0[k], b0[k], loads, want_modes)[2] for k in range(n_steps)])
    assert np.array_equal(want, applied) and (want != 0).any()


def test_bad_reports_and_sharded_batches_are_refused_by_the_march():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    series = dict(channel=np.zeros((2, 1)), probes=md["zone_slot"])
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        with pytest.raises(HeatError) as e:
            b.march_series(np.zeros((2, 1, 3)), 1, report=dict(groups=[md["zone_slot"], md["solar_front_slot"][:3]]), **series)
        assert e.value.code == -4 and "group entry %d" % len(md["zone_slot"]) in str(e.value)
        with pytest.raises(HeatError) as e:
            b.march_series(np.zeros((2, 1, 3)), 1, report=dict(thermostat_stats=("switches",)), **series)
        assert e.value.code == -1 and "thermostat" in str(e.value)
        got = st.copy()
        b.download_state(got)
        assert np.array_equal(got, st)
        # r == NULL through the new entry point is the series with loads; the old entry points still refuse a NULL trace
        s, keep = binding.make_series(np.zeros((2, 1, 3)), 1, **series)
        trace, f = np.zeros((2, len(md["zone_slot"]))), binding.C.c_int32(7)
        assert b._L.heat_batch_march_series_report(b._h, binding.C.byref(s), None, None, trace.ctypes.data_as(binding._dp), None, binding.C.byref(f)) == 0
        b.upload_state(st.copy())
        want, _ = b.march_series(np.zeros((2, 1, 3)), 1, **series)
        assert np.array_equal(trace, want)
        assert b._L.heat_batch_march_series(b._h, binding.C.byref(s), None, binding.C.byref(f)) == -1
        assert b._L.heat_batch_march_series_loads(b._h, binding.C.byref(s), None, None, None, binding.C.byref(f)) == -1
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(np.zeros((2, 1, 3)), 1, report=dict(stats=("min",)), **series)
        assert e.value.code == -1 and "sharded" in str(e.value)
