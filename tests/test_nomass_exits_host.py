"""The no-mass loop's exits on the host: tests/nomass_ref.py (the loop of surface.rs:790-898 in longdouble, with its trace)
against the CPU oracle, and the conditions the cases of tests/nomass_exit_cases.py have to meet before a GPU result on
them says anything — every exit reached in every family, no decision of any pass near its threshold, and a neighbouring
pass count that shows in the temperatures.

Measured here (x86-64, longdouble of 64 mantissa bits), the worst |T oracle - T nomass_ref| over the no-mass nodes of a
family, first sub-timestep: panel2 2.6e-14, panel4 2.1e-14, long_run 1.7e-14, facing_* 2.7e-14, chunk2_* 3.0e-14,
glazing 2.9e-12, still_air:panel2 7.0e-14, still_air:panel4 4.2e-14, still_air:glazing 4.3e-12 K. The glazings are the
oracle's own f64 rounding: a pane's conductance (333 W/m2K) beside a film coefficient of 0.5 conditions K at about 700,
and every pass of a diverging loop multiplies what the pass before left by |lambda|. With faces 0.05 K off still air
(hs = 0.5, three passes kept) it reaches 1.4e-11 K: the still-air glazings start 0.2 K off at least.

`glazing` reaches B at a count of 2 and more (4 surfaces: the line between two faces 0.3 ... 0.43 K beyond their airs,
overrides of 0.9 ... 1.1 W/m2K; the other families get the same inputs and leave by C or by B at the second pass)."""
import functools

import numpy as np
import pytest

import nomass_exit_cases as nec
import nomass_ref as nr
from heat_amd import modeldict as mdl

TOL_REF = 1e-11            # a hundredth of the parity tolerance
MARGIN = 1e-6
MOVES = 1e-6


def cell_of(ch):
    if ch.exit == "B":
        return "B1" if ch.count == 1 else "B2+"
    if ch.exit == "C":
        return "C0" if ch.count == 0 else ("C20+" if ch.count >= 20 else "C")
    if ch.exit == "D":
        return "D100" if ch.count == 100 else "D>100"
    return ch.exit


def weather_row(k):
    w = nec.WEATHER[k]
    return float(w[1]), float(w[2]), float(w[0])


@functools.lru_cache(maxsize=None)
def states(oracle, family, batch):
    """The oracle's state before each of the three sub-timesteps of one batch of a family, the batch's model, and the
    state after the last."""
    c = nec.case(family)
    idx = dict(nec.batches(c))[batch]
    md = mdl.subset(c.md, idx)
    om = oracle.OracleModel(md)
    out = [c.st.copy()]
    for k in range(len(nec.WEATHER)):
        st = out[-1].copy()
        rc, _ = om.march(st, nec.WEATHER[k:k + 1])
        assert rc == 0
        out.append(st)
    return md, out


@pytest.mark.parametrize("family", nec.CASES)
def test_reference_against_the_oracle_surface_by_surface(oracle, family):
    c = nec.case(family)
    om = oracle.OracleModel(c.md)
    worst = 0.0
    for s, r in enumerate(c.ref):
        st = c.st.copy()
        rc, iters = om.iterate_surfaces(st, *weather_row(0), s0=s, s1=s + 1)
        assert rc == 0
        assert iters == r.passes, (s, iters, r.chunks)
        first = int(c.md["first_node_slot"][s])
        for i in r.nomass:
            worst = max(worst, abs(float(nr.LD.num(st[first + i]) - r.T[i])))
    print("%s: worst |T oracle - T nomass_ref| = %.3e K over %d surfaces" % (family, worst, c.n_own))
    assert worst <= TOL_REF


@pytest.mark.parametrize("family", ["facing_front", "facing_back", "facing_both"])
def test_closed_form_of_the_one_node_chunk(oracle, family):
    """T_k = T* + (T_0 - T*) lambda^k: exit, count and temperature follow without running the loop, and agree with the
    loop of nomass_ref and with the oracle."""
    c = nec.case(family)
    om = oracle.OracleModel(c.md)
    exits = set()
    for s, r in enumerate(c.ref):
        st = c.st.copy()
        rc, _ = om.iterate_surfaces(st, *weather_row(0), s0=s, s1=s + 1)
        assert rc == 0
        first = int(c.md["first_node_slot"][s])
        wall = nr.wall_of(c.md, s)
        T0 = [nr.LD.num(c.st[first + i]) for i in range(len(wall["mass"]))]
        solar = nr.solar_per_node(c.md, c.st, s)
        for ch in r.chunks:
            assert ch.fin - ch.ini == 1
            form = nr.one_node_form(wall, ch.ini, T0, r.front, r.back, solar)
            exit_, count, t = form.outcome(T0[ch.ini])
            assert (exit_, count) == (ch.exit, ch.count), (s, ch, exit_, count, float(form.lam))
            assert abs(float(t - r.T[ch.ini])) <= TOL_REF and abs(float(t - nr.LD.num(st[first + ch.ini]))) <= TOL_REF
            for k in range(0, len(ch.trace), 7):
                assert abs(float(form.err(T0[ch.ini], k) / ch.trace_ld[k] - 1)) < 1e-9
            exits.add(ch.exit)
    assert exits == set("ABCD")


@pytest.mark.parametrize("family", nec.CASES)
def test_every_exit_is_reached(family):
    c = nec.case(family)
    cells = {}
    for r in c.ref:
        for ch in r.chunks:
            cells[cell_of(ch)] = cells.get(cell_of(ch), 0) + 1
    print(family, sorted(cells.items()))
    if family.startswith("still_air"):
        assert cells.get("B1", 0) + cells.get("B2+", 0) >= c.n_own // 2     # free convection alone
        return
    for cell in ("A", "B1", "C0", "C20+", "D100", "D>100"):
        assert cells.get(cell, 0) >= 2, (cell, cells)
    if family == "glazing":
        assert cells.get("B2+", 0) >= 2, cells
    one_sided = np.isnan(c.md["front_hs_fix"][:c.n_own]) != np.isnan(c.md["back_hs_fix"][:c.n_own])
    assert one_sided.sum() >= 4 and np.isnan(c.md["front_hs_fix"][:c.n_own])[one_sided].any() \
        and np.isnan(c.md["back_hs_fix"][:c.n_own])[one_sided].any()             # (a NaN override is none)
    # ... and both orders hold what they say: one exit per grouped batch, every exit in every tile of the interleaved one
    order = nec.interleaved(c)
    assert sorted(order) == list(range(int(c.md["n_surfaces"])))
    own = [s for s in order if s < c.n_own]
    for t in range(0, len(own) - 63, 64):
        assert {c.exit_of[s][0] for s in own[t:t + 64]} >= set("ABCD"), t
    assert sorted(s for idx in nec.grouped(c).values() for s in idx if s < c.n_own) == list(range(c.n_own))


@pytest.mark.parametrize("family", nec.CASES)
def test_no_decision_near_its_threshold_in_any_batch_at_any_sub_timestep(oracle, family):
    """The fast-path kernels form K and q in another order than the oracle: a decision closer than 1e-6 (relative) to
    its threshold may fall the other way there. A condition on the inputs — met by choosing them, for every batch the
    GPU test marches and each of its three sub-timesteps (the reference's loop on the oracle's state before that
    sub-timestep; the grouped batches start as the whole family does, so their first one is the family's). Also: the
    reference's temperatures stay within -100 ... 200 C."""
    c = nec.case(family)
    worst = min(nr.margins(ch) for r in c.ref for ch in r.chunks)
    for batch, idx in nec.batches(c):
        md, sts = states(oracle, family, batch)
        nodes = mdl.node_slots(md)
        for st in sts:
            assert st[nodes].min() > -100.0 and st[nodes].max() < 200.0, (batch, st[nodes].min(), st[nodes].max())
        for k in (1, 2):
            for s in range(int(md["n_surfaces"])):
                if idx[s] >= c.n_own:
                    continue
                r = nr.march_surface(md, sts[k], s, *weather_row(k))
                worst = min([worst] + [nr.margins(ch) for ch in r.chunks])
                assert worst >= MARGIN, (batch, k, int(idx[s]), r.chunks)
    print("%s: smallest margin %.3e" % (family, worst))
    assert worst >= MARGIN


@pytest.mark.parametrize("family", nec.CASES)
def test_a_neighbouring_pass_count_shows_in_the_temperatures(family):
    c = nec.case(family)
    least = np.inf
    for s, r in enumerate(c.ref):
        for ch in r.chunks:
            if ch.exit == "C" and ch.count == 0:
                continue
            kept = r.T[ch.ini:ch.fin]
            assert ch.later is not None
            for other in (ch.earlier, ch.later):
                if other is None:
                    assert ch.exit == "A", (s, ch)         # (no pass came before the first)
                    continue
                moved = max(abs(float(a - b)) for a, b in zip(kept, other))
                least = min(least, moved)
                assert moved > MOVES, (s, ch, moved)
    print("%s: a pass more or less moves a node by %.3e K at least" % (family, least))


@pytest.mark.parametrize("family", nec.E_FAMILIES)
def test_the_oracle_answers_nan_in_the_no_mass_loop(oracle, family):
    """Exit E: a NaN long-wave irradiance on an Outdoor front leaves the coefficient finite and makes err NaN at the
    first pass (surface.rs:850) — OR_ERR_NAN_NOMASS, and E in nomass_ref."""
    md, healthy, bad, s = nec.damaged(family)
    rc, _ = oracle.OracleModel(md).march(bad.copy(), nec.WEATHER[:1])
    assert rc == 2, rc                                  # OR_ERR_NAN_NOMASS
    rc, _ = oracle.OracleModel(md).march(healthy.copy(), nec.WEATHER[:1])
    assert rc == 0
    r = nr.march_surface(md, bad, s, *weather_row(0))
    assert [ch.exit for ch in r.chunks] == ["E"] and len(r.chunks[0].trace) == 1 and float(r.front["hs"]) > 0.0


def test_glazing_without_wind_leaves_exit_c(oracle):
    """A generator the suite has had all along, once the wind drops: its loops run past the 100th pass."""
    md, st = mdl.glazing_cavity(400, Z=8, dt=45.0)
    om = oracle.OracleModel(md)
    totals = {}
    for wind in (3.0, 0.0):
        state = st.copy()
        rc, totals[wind] = om.march(state, mdl.weather_series(25, 45.0, wind_speed=wind))
        assert rc == 0
    assert totals[0.0] > totals[3.0], totals
    state = st.copy()
    w = mdl.weather_series(25, 45.0, wind_speed=0.0)
    most = 0
    for k in range(25):
        before = state.copy()
        rc, _ = om.march(state, w[k:k + 1])
        assert rc == 0
        if k % 6:
            continue                     # (every sixth sub-timestep: surface by surface on the state before it)
        for s in np.flatnonzero(np.diff(md["node_offset"]) == 4):
            probe = before.copy()
            rc, it = om.iterate_surfaces(probe, float(w[k, 1]), float(w[k, 2]), float(w[k, 0]), s0=int(s), s1=int(s) + 1)
            most = max(most, it)
    print("passes: %s; most in one surface and sub-timestep: %d" % (totals, most))
    assert most - 1 >= 100, most         # (passes = count + 1)
