"""Controllers of a series on the host (include/heat_amd.h, heat_controllers): no GPU here.

The rule in numpy (heat_amd/controllers.py, apply) against hand-worked single-controller cases, line by line; the ABI (symbols,
struct layout); every refusal of heat_controllers_check with its code and message; and the generator's cases
(tests/controllers_cases.py) through the CPU oracle alone: they are accepted, the loops respond — u strictly inside (0, 1) in
some steps and at both clamps in others, limits trip and release, the heated node of a slab is the wall's warmest while it
heats — no decision comes within 1e-6 K of its threshold, a cut loop equals the loop in one, and the planner routes a wall that
absorbs inside to the general class."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import heat_amd
from heat_amd import binding, controllers as ctl, modeldict as mdl
import controllers_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_controllers_check", "heat_batch_march_series_controllers")
E_INVALID_ARG, E_SIZE = -1, -4
FIELDS = ("n_controllers", "sense_kind", "sense_index", "sense_node", "set_chan", "action", "en_chan", "lim_kind", "lim_index", "lim_node",
          "out_chan", "kp", "ki", "bias", "out_lo", "out_hi", "lim_hi", "lim_lo", "resume", "integral", "tripped", "sum_u", "sum_out",
          "steps_on", "steps_sat", "trips")
OUT_OF_SCOPE = ("sensing the comfort term's operative temperature", "cascades, where a controller reads a controller",
                "minimum on and off times", "derivative action", "any change to the march kernels")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "typedef struct heat_controllers {" in header
    assert "heat_controllers_check" in binding.HOST_ONLY_SYMBOLS
    assert "heat_batch_march_series_controllers" not in binding.HOST_ONLY_SYMBOLS
    assert all(hasattr(binding, n) for n in ("Controllers", "make_controllers", "controllers_check"))
    assert all(hasattr(heat_amd, n) for n in ("Controllers", "make_controllers", "controllers_check", "controllers"))
    assert all(hasattr(ctl, n) for n in ("apply", "accumulate", "fresh", "concat", "proportional", "pi", "with_limit", "embed"))
    flat = " ".join(header.replace("*", " ").split())
    for words in OUT_OF_SCOPE:
        assert words in flat, words                                     # what is out of scope is stated
    assert "first behind the controllers" in open(os.path.join(ROOT, "heat_amd", "csrc", "series_kernels.hip")).read()
    assert L.heat_amd_abi_version() == 1
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
    assert all(re.search(r"\bfn %s\(" % name, rust) for name in NEW) and "pub struct HeatControllers" in rust


def test_controllers_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    args = ["sizeof(heat_controllers)", "sizeof(heat_openings)", "sizeof(heat_series_call)"] + ["offsetof(heat_controllers, %s)" % f for f in FIELDS]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "heat_amd.h"\n'
                   'int main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == ([C.sizeof(binding.Controllers), C.sizeof(binding.Openings), C.sizeof(binding.SeriesCall)] +
                   [getattr(binding.Controllers, f).offset for f in FIELDS])
    assert [f for f, _ in binding.Controllers._fields_] == list(FIELDS)
    # every field is 8 bytes wide; the structs beside it are as they were
    assert got[0] == 8 * len(FIELDS) and got[3:] == [8 * i for i in range(len(FIELDS))]
    assert got[1] == 8 * 17 and got[2] == 8 * 24


# ---- the rule in numpy: hand-worked single-controller cases ----
# two zones; channel 0 the setpoint, 1 the enable, 2 an outside temperature, 3 the derived channel, 4 a bystander
T = np.array([19.0, 23.5])
ROW = np.array([21.0, 1.0, 4.0, np.nan, 7.0])


def one(**more):
    return dict(dict(sense_index=[0], set_chan=[0], out_chan=[3], kp=[0.25], out_hi=[1200.0]), **more)


def run(ct, row=ROW, T=T, N=None, md=None, state=None):
    state = ctl.fresh(ct) if state is None else state
    new, u, out = ctl.apply(T, N, row, ct, state, md)
    return new, float(u[0]), float(out[0]), state


def test_a_proportional_loop_follows_the_rule_line_by_line():
    new, u, out, st = run(one(bias=[0.125], out_lo=[100.0]))
    e = 21.0 - 19.0
    want_u = (0.25 * e + 0.0) + 0.125
    assert u == want_u == 0.625 and out == 100.0 + want_u * (1200.0 - 100.0)
    assert new[3] == out and np.array_equal(np.delete(new, 3), np.delete(ROW, 3)) and np.isnan(ROW[3])      # the row itself is not written
    assert st["integral"][0] == 0.0 and st["tripped"][0] == 0
    # cooling action: the sign of the error flips, nothing else
    _, u2, _, _ = run(one(action=[-1], sense_index=[1]))
    assert u2 == 0.25 * (23.5 - 21.0)
    # sensing a channel
    _, u3, _, _ = run(one(sense_kind=[2], sense_index=[2], kp=[0.03125]))
    assert u3 == 0.03125 * (21.0 - 4.0)
    # both clamps, and a negative out_hi (a cooled slab)
    assert run(one(kp=[2.0]))[1:3] == (1.0, 1200.0)
    assert run(one(kp=[2.0], action=[-1]))[1:3] == (0.0, 0.0)
    assert run(one(kp=[0.25], out_hi=[-800.0]))[2] == -400.0


def test_a_pi_loop_integrates_clamps_its_integral_and_resets_when_disabled():
    ct = one(ki=[0.125])
    st = ctl.fresh(ct)
    seen = []
    for k in range(6):
        _, u, _, _ = run(ct, state=st)
        seen.append((u, float(st["integral"][0])))
    # e = 2: p = 0.5, the integral grows by 0.25 a step and stops at 1 (the anti-windup); u saturates
    assert seen == [(0.75, 0.25), (1.0, 0.5), (1.0, 0.75), (1.0, 1.0), (1.0, 1.0), (1.0, 1.0)]
    # a negative error takes the integral down again, and not below 0
    down = np.array([15.0, 1.0, 4.0, np.nan, 7.0])
    assert [run(ct, row=down, state=st)[3]["integral"][0] for _ in range(3)] == [0.5, 0.0, 0.0]
    st["integral"][0] = 0.5
    off = np.array([21.0, 0.0, 4.0, np.nan, 7.0])
    _, u, out, _ = run(dict(ct, en_chan=[1], out_lo=[50.0]), row=off, state=st)
    assert (u, out, st["integral"][0]) == (0.0, 50.0, 0.0)                                    # disabled: I = 0, u = 0, out = out_lo
    on = np.array([21.0, 0.5, 4.0, np.nan, 7.0])
    assert run(dict(ct, en_chan=[1]), row=on, state=st)[1] == 0.75                            # enabled where the channel is > 0


def test_a_limit_trips_holds_the_integral_and_releases_below_its_lower_threshold():
    md, st0 = mdl.uniform_massive(2, 8, Z=2)
    N = st0.copy()
    last = md["first_node_slot"][1] + 7
    ct = ctl.with_limit(one(ki=[0.125]), 1, [1], 29.0, 27.0)
    assert ct["lim_node"].tolist() == [-1]
    st = ctl.fresh(ct)
    log = []
    for t_face in (28.0, 29.0, 29.5, 28.0, 27.0, 26.5, 29.5):
        N[last] = t_face
        _, u, _, _ = run(ct, N=N, md=md, state=st)
        log.append((u, float(st["integral"][0]), int(st["tripped"][0]), int(st["trips"][0])))
    assert log == [(0.75, 0.25, 0, 0), (1.0, 0.5, 0, 0),      # 29.0 is not above 29.0
                   (0.0, 0.5, 1, 1), (0.0, 0.5, 1, 1),        # tripped: u = 0, the integral is held; 28 is inside the hysteresis
                   (0.0, 0.5, 1, 1),                          # 27.0 is not below 27.0
                   (1.0, 0.75, 0, 1), (0.0, 0.75, 1, 2)]      # released; tripped again
    # a node named by number, and the sensed node
    N[md["first_node_slot"][0] + 3] = 18.5
    assert run(one(sense_kind=[1], sense_index=[0], sense_node=[3]), N=N, md=md)[1] == 0.25 * (21.0 - 18.5)


def test_a_nan_setpoint_gives_a_nan_signal_and_nothing_else_changes():
    ct = ctl.concat(one(ki=[0.125]), one(sense_index=[1], set_chan=[4], out_chan=[2]))
    row = np.array([np.nan, 1.0, 4.0, np.nan, 27.5])
    st = ctl.fresh(ct)
    new, u, out = ctl.apply(T, None, row, ct, st)
    assert np.isnan(u[0]) and np.isnan(out[0]) and np.isnan(st["integral"][0]) and u[1] == 1.0 and new[2] == 1200.0
    acc = ctl.fresh(ct)
    ctl.accumulate(u, out, acc)
    assert np.isnan(acc["sum_u"][0]) and acc["steps_on"].tolist() == [0, 1] and acc["steps_sat"].tolist() == [0, 1]


def test_the_conveniences():
    assert ctl.proportional(4.0) == dict(kp=0.25, bias=0.5) and ctl.proportional(4.0, full_at="band")["bias"] == 0.0
    p = ctl.pi([4.0, 8.0], 10.0)
    assert p["kp"].tolist() == [0.25, 0.125] and p["ki"].tolist() == [0.025, 0.0125]
    both = ctl.concat(one(), one(ki=[0.5], out_chan=[4], en_chan=[1]))
    assert both["ki"].tolist() == [0.0, 0.5] and both["en_chan"].tolist() == [-1, 1] and both["action"].tolist() == [1, 1]
    assert ctl.n_controllers(both) == 2 and ctl.n_controllers({}) == 0 and set(ctl.fresh(both)) == set(ctl.STATE + ctl.ACC)
    md, _ = mdl.uniform_massive(3, 8, Z=1)
    md2, drive = ctl.embed(md, [2, 0], [4, -1])
    o = md["node_offset"]
    assert md2["back_alpha"][o[2]:o[3]].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and md2["back_alpha"][o[0]:o[1]].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert np.array_equal(md2["back_alpha"][o[1]:o[2]], md["back_alpha"][o[1]:o[2]]) and md["back_alpha"][o[3] - 1] == 0.7      # a copy
    assert drive["chan_key"] == "solar_back" and np.array_equal(drive["gain"], 1.0 / md["area"][[2, 0]]) and drive["general"] == 1
    with pytest.raises(ValueError):
        ctl.embed(md, [1, 1], [2, 3])
    with pytest.raises(ValueError):
        ctl.embed(md, [1], [8])


def test_the_planner_routes_a_wall_that_absorbs_inside_to_the_general_class():
    """The fast classes absorb at the two face nodes only. embed() says how many walls it moves; heat_plan_check's class counts
    (those of heat_batch_class_counts) show them in the general class, and a wall embedded at its own face node stays."""
    md, _ = mdl.clustered_massive(200, Z=8, seed=3)
    before = binding.plan_check(md)[:5]
    assert before[4] == 0
    md2, drive = ctl.embed(md, [5, 17, 40], [3, -1, 1])
    after = binding.plan_check(md2)[:5]
    assert drive["general"] == 2 and after[4] == 2 and sum(after) == sum(before)


def test_an_embedded_node_is_the_warmest_of_its_slab_while_heated_and_the_coldest_around_while_cooled(oracle):
    """Two identical 12-node walls of one zone, everything at 22 C, through the oracle alone: controller 0 puts 200 W/m2 into
    node 6 of wall 0, controller 1 takes 200 W/m2 out of node 6 of wall 1 (a negative out_hi through the back side), both
    saturated. At every step the heated node is the warmest of its wall and the cooled one colder than both of its neighbours
    (the front face, in outside air at 10 C, may be colder still); the first step moves the node by less than q h / m, the rise
    without conduction, and by more than half of it."""
    md, st = mdl.uniform_massive(2, 12, Z=1, identical=True)
    md2, drive = ctl.embed(md, [0, 1], [6, 6])
    q, n = 200.0, 10
    ct = dict(sense_index=[0, 0], set_chan=[0, 1], action=[1, -1], out_chan=[2, 3], kp=[1.0, 1.0], out_hi=q * md["area"][[0, 1]] * [1.0, -1.0])
    channel = np.tile([40.0, 0.0, np.nan, np.nan], (n, 1))
    state, acc = st.copy(), ctl.fresh(ct)
    m = oracle.OracleModel(md2)
    w = mdl.weather_series(n * 2, md["dt"]).reshape(n, 2, 3)
    first = md2["first_node_slot"]
    free = q * 2 * md["dt"] / md["mass"][md["node_offset"][0] + 6]
    for k in range(n):
        row, u, out = ctl.apply(state[md2["zone_slot"]], state, channel[k], ct, acc, md2)
        assert u.tolist() == [1.0, 1.0] and np.allclose(drive["gain"] * out, [q, -q], rtol=1e-15)
        state[md2["solar_back_slot"][[0, 1]]] = drive["gain"] * out
        assert m.march(state, w[k])[0] == 0
        hot, cold = state[first[0]:first[0] + 12], state[first[1]:first[1] + 12]
        assert np.argmax(hot) == 6 and (np.delete(hot, 6) < hot[6]).all() and cold[6] < cold[5] and cold[6] < cold[7], k
        if k == 0:
            assert 0.5 * free < hot[6] - 22.0 < free and 0.5 * free < 22.0 - cold[6] < free
    assert hot[6] > 24.5 and cold[6] < 19.5 and acc["sum_u"].tolist() == [0.0, 0.0]      # (the test accumulates nothing)


# ---- refusals ----
@pytest.fixture(scope="module")
def model():
    return mdl.clustered_massive(200, Z=8, seed=3)[0]


N_CHANNELS = 14


def series(**more):
    return dict(dict(weather=np.zeros((2, 1, 3)), n_sub=1, channel=np.zeros((2, N_CHANNELS))), **more)


def good():
    """Four controllers in 8 zones: channels 0-1 setpoints, 2 an enable, 3 a temperature, 4-5 the openings' derived channels,
    8-11 the controllers'."""
    return dict(sense_kind=[0, 1, 2, 0], sense_index=[3, 17, 3, 7], sense_node=[-1, 2, -1, -1], set_chan=[0, 1, 0, 1], action=[1, 1, -1, 1],
                en_chan=[-1, 2, -1, 2], lim_kind=[-1, 1, 2, 0], lim_index=[-1, 17, 3, 6], lim_node=[-1, -1, -1, -1], out_chan=[8, 11, 9, 10],
                kp=[0.25, 0.5, 0.0, 1.0], ki=[0.0, 0.05, 0.1, 0.0], bias=[0.5, 0.0, -0.25, 0.0], out_lo=[0.0, 0.0, 0.0, 1.0],
                out_hi=[1000.0, -500.0, 1.0, 0.0], lim_hi=[0.0, 29.0, 30.0, 26.0], lim_lo=[0.0, 27.0, 30.0, 25.0])


def good_openings():
    return dict(zone_a=[0, 3], zone_b=[-1, 4], temp_chan=[3, -1], frac_chan=[8, -1], out_chan=[4, 5], area=[0.5, 1.0], cs=[5.0, 20.0], c0=[0.01, 0.01])


def changed(g, key, i, value):
    a = np.array(g[key], dtype=np.float64 if isinstance(value, float) else None)
    a[i] = value
    return dict(g, **{key: a})


def _code(call):
    with pytest.raises(binding.HeatError) as e:
        call()
    return e.value.code, str(e.value)


def _raw(model, g, **fields):
    """heat_controllers_check with fields of the struct overwritten (a count, or None for a NULL array)."""
    L = binding.load_library()
    desc, keep = binding.make_desc(model)
    s, skeep = binding.make_series(**series())
    ct, ckeep = binding.make_controllers(**g)
    for k, v in fields.items():
        setattr(ct, k, v)
    rc = L.heat_controllers_check(C.byref(desc), C.byref(s), None, C.byref(ct))
    return rc, L.heat_last_error().decode("utf-8", "replace")


def test_a_good_term_no_term_and_an_empty_term_are_accepted(model):
    g = good()
    binding.controllers_check(model, g, **series())
    binding.controllers_check(model, g, openings=good_openings(), **series())          # an opening's frac_chan is a controller's output
    binding.controllers_check(model, None, **series())
    binding.controllers_check(model, {}, openings=good_openings(), **series())
    binding.controllers_check(model, dict(sense_index=[1], set_chan=[0], out_chan=[8], kp=[0.5], out_hi=[1.0]), **series())
    binding.controllers_check(model, dict(g, stats=(), state=()), **series())
    fresh = ctl.fresh(g)
    binding.controllers_check(model, dict(g, resume=dict(fresh, integral=[0.0, 1.0, 0.5, np.nan], tripped=[0, 1, 1, 0])), **series())
    with pytest.raises(ValueError):
        binding.make_controllers(**dict(g, stats=("sum_v",)))
    with pytest.raises(ValueError):
        binding.make_controllers(**dict(g, kp=[1.0]))
    with pytest.raises(ValueError):
        binding.make_controllers(**dict(g, resume=dict(sum_u=np.zeros(4))))


def test_counts_and_null_arrays_are_invalid_arguments(model):
    g = good()
    rc, msg = _raw(model, g, n_controllers=-1)
    assert rc == E_INVALID_ARG and "controller" in msg and "negative" in msg, msg
    for field in ("sense_index", "set_chan", "out_chan", "kp", "out_hi"):
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "controller 0:" in msg and field in msg, (field, msg)
    for field in ("lim_index", "lim_hi", "lim_lo"):                                      # needed where a limit is
        rc, msg = _raw(model, g, **{field: None})
        assert rc == E_INVALID_ARG and "controller 1:" in msg and "lim_index, lim_hi and lim_lo" in msg, (field, msg)
    for field in ("action", "en_chan", "lim_node", "ki", "bias", "out_lo") + binding.CONTROLLER_STATE + binding.CONTROLLER_STATS:   # nullable
        rc, msg = _raw(model, g, **{field: None})
        assert rc == 0, (field, msg)
    rc, msg = _raw(model, g, lim_kind=None, lim_index=None, lim_hi=None, lim_lo=None)
    assert rc == 0, msg
    rc, msg = _raw(model, g, n_controllers=0, sense_index=None, set_chan=None, out_chan=None, kp=None, out_hi=None)
    assert rc == 0, msg
    # sense_kind NULL: every controller senses a zone, and 17 is none of the 8
    rc, msg = _raw(model, g, sense_kind=None)
    assert rc == E_SIZE and "controller 1:" in msg and "zone 17" in msg, msg


@pytest.mark.parametrize("key", ["kp", "ki", "bias", "out_lo", "out_hi", "lim_hi", "lim_lo"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_constant_that_is_not_finite_is_refused(model, key, bad):
    code, msg = _code(lambda: binding.controllers_check(model, changed(good(), key, 2, bad), **series()))
    assert code == E_INVALID_ARG and "controller 2:" in msg and key in msg, msg


def test_every_other_refusal_names_its_controller(model):
    g, op = good(), good_openings()
    n_nodes = int(np.diff(model["node_offset"])[17])
    Z, S = int(model["n_zones"]), int(model["n_surfaces"])
    resumed = lambda **kw: dict(g, resume=dict(ctl.fresh(g), **kw))   # noqa: E731
    for bad, code, needle in ((changed(g, "kp", 1, -1e-9), E_INVALID_ARG, "controller 1: kp"),
                              (changed(g, "ki", 3, -0.5), E_INVALID_ARG, "controller 3: ki"),
                              (changed(g, "lim_lo", 1, 29.5), E_INVALID_ARG, "controller 1: lim_lo"),
                              (changed(g, "sense_kind", 0, 3), E_INVALID_ARG, "controller 0: sense_kind"),
                              (changed(g, "sense_kind", 0, -1), E_INVALID_ARG, "controller 0: sense_kind"),
                              (changed(g, "lim_kind", 2, 3), E_INVALID_ARG, "controller 2: lim_kind"),
                              (changed(g, "lim_kind", 2, -2), E_INVALID_ARG, "controller 2: lim_kind"),
                              (resumed(tripped=[0, 2, 0, 0]), E_INVALID_ARG, "controller 1: tripped"),
                              (resumed(integral=[0.0, 0.0, 1.0000001, 0.0]), E_INVALID_ARG, "controller 2: integral"),
                              (resumed(integral=[0.0, 0.0, 0.0, -1e-12]), E_INVALID_ARG, "controller 3: integral"),
                              (changed(g, "sense_index", 0, Z), E_SIZE, "controller 0: sense zone"),
                              (changed(g, "sense_index", 3, -1), E_SIZE, "controller 3: sense zone"),
                              (changed(g, "sense_index", 1, S), E_SIZE, "controller 1: sense surface"),
                              (changed(g, "sense_index", 2, N_CHANNELS), E_SIZE, "controller 2: sense channel"),
                              (changed(g, "sense_node", 1, n_nodes), E_SIZE, "controller 1: sense node"),
                              (changed(g, "sense_node", 1, -2), E_SIZE, "controller 1: sense node"),
                              (changed(g, "lim_index", 3, Z), E_SIZE, "controller 3: limit zone"),
                              (changed(g, "lim_index", 1, -1), E_SIZE, "controller 1: limit surface"),
                              (changed(g, "lim_index", 2, N_CHANNELS), E_SIZE, "controller 2: limit channel"),
                              (changed(g, "lim_node", 1, n_nodes), E_SIZE, "controller 1: limit node"),
                              (changed(g, "set_chan", 2, -1), E_SIZE, "controller 2: no setpoint channel"),
                              (changed(g, "set_chan", 2, N_CHANNELS), E_SIZE, "controller 2: setpoint channel"),
                              (changed(g, "en_chan", 0, N_CHANNELS), E_SIZE, "controller 0: enable channel"),
                              (changed(g, "en_chan", 0, -2), E_SIZE, "controller 0: enable channel"),
                              (changed(g, "out_chan", 3, N_CHANNELS), E_SIZE, "controller 3: derived channel"),
                              (changed(g, "out_chan", 3, -1), E_SIZE, "controller 3: derived channel"),
                              (changed(g, "out_chan", 2, 8), E_SIZE, "controller 2: its derived channel out_chan 8 is also controller 0's"),
                              (changed(g, "out_chan", 1, 5), E_SIZE, "controller 1: its derived channel out_chan 5 is also opening 1's"),
                              (changed(g, "sense_index", 2, 10), E_SIZE, "controller 2: its sense channel 10 is the derived channel of controller 3"),
                              (changed(g, "set_chan", 0, 9), E_SIZE, "controller 0: its set_chan 9 is the derived channel of controller 2"),
                              (changed(g, "en_chan", 3, 10), E_SIZE, "controller 3: its en_chan 10 is the derived channel of controller 3"),
                              (changed(g, "lim_index", 2, 11), E_SIZE, "controller 2: its limit channel 11 is the derived channel of controller 1"),
                              (changed(g, "sense_index", 2, 4), E_SIZE, "controller 2: its sense channel 4 is the derived channel of opening 0"),
                              (changed(g, "set_chan", 1, 5), E_SIZE, "controller 1: its set_chan 5 is the derived channel of opening 1"),
                              (changed(g, "en_chan", 1, 4), E_SIZE, "controller 1: its en_chan 4 is the derived channel of opening 0"),
                              (changed(g, "lim_index", 2, 5), E_SIZE, "controller 2: its limit channel 5 is the derived channel of opening 1")):
        got, msg = _code(lambda: binding.controllers_check(model, bad, openings=op, **series()))
        assert got == code and needle in msg, (msg, needle)
    # a bad opening is the openings' refusal; a series without channels
    got, msg = _code(lambda: binding.controllers_check(model, g, openings=dict(op, area=[0.5, -1.0]), **series()))
    assert got == E_INVALID_ARG and "opening 1:" in msg
    got, msg = _code(lambda: binding.controllers_check(model, g, **series(channel=np.zeros((2, 0)))))
    assert got == E_SIZE and "controller 0:" in msg


# ---- the generator's cases: accepted, and — through the CPU oracle alone — they exercise what they promise ----
COVERAGE_CASES = cc.ORACLE_CASES + [("rooms_with_windows", 2)]
_LOOPS = {}


def oracle_loop(oracle, model_name, n_sub):
    if (model_name, n_sub) not in _LOOPS:
        c = cc.case(model_name, cc.N_STEPS, n_sub, 2, cc.SEED)
        m = oracle.OracleModel(c["md"])

        def march(s, wk, za, zb):
            assert m.march(s, wk, za, zb, threads=1)[0] == 0

        state = c["st"].copy()
        _LOOPS[(model_name, n_sub)] = (c, march, cc.loop_with_rules(march, c, state), state)
    return _LOOPS[(model_name, n_sub)]


@pytest.mark.parametrize("model_name,n_sub", COVERAGE_CASES)
def test_the_generators_cases_are_accepted_respond_and_keep_their_margin(oracle, model_name, n_sub):
    c, march, out, _ = oracle_loop(oracle, model_name, n_sub)
    md, ct, info = c["md"], c["controllers"], c["controllers_info"]
    kw = dict(weather=c["w"], n_sub=n_sub, channel=c["channel"], probes=c["probes"])
    binding.controllers_check(md, ct, openings=c["openings"], **kw)
    binding.air_species_check(md, c["species"], loads=c["loads"], air=c["air"], handlers=c["handlers"], **kw)
    # what the generator promises: two controllers per zone, shuffled, every kind of consumer reads a derived channel
    Z, n = int(md["n_zones"]), ctl.n_controllers(ct)
    assert n == 2 * Z and sorted(ct["out_chan"].tolist()) == info["derived"].tolist() and np.isnan(c["channel"][:, info["derived"]]).all()
    assert not np.array_equal(np.argsort(ct["sense_index"], kind="stable"), np.arange(n))
    derived = set(info["derived"].tolist())
    read_by = dict(gain=set(c["loads"]["gains"]["chan"].tolist()), frac=set(np.asarray(c["openings"]["frac_chan"]).tolist()),
                   path=set(np.asarray(c["air"]["volume_chan"]).tolist()), panel=set(np.asarray(c["radiation"]["en_chan"]).tolist()),
                   slab=set(c["drives"]["solar_back"][0].tolist()))
    assert all(len(v & derived) >= Z // 4 for v in read_by.values()), {k: len(v & derived) for k, v in read_by.items()}
    assert set().union(*read_by.values()) >= derived and len(read_by["slab"] & derived) == Z
    assert set(np.unique(ct["sense_kind"]).tolist()) == {0, 1, 2} and (ct["ki"] > 0).any() and (ct["ki"] == 0).any()
    assert (ct["out_hi"] < 0).any() and (ct["action"] < 0).any() and (ct["en_chan"] >= 0).any() and (ct["lim_kind"] == 1).sum() == Z
    # the walls that absorb inside are in the general class, those embedded at their face node are where they were
    before, after = binding.plan_check(c["md_plain"])[:5], binding.plan_check(md)[:5]
    assert 0 < info["general"] < Z and after[4] == before[4] + info["general"] and sum(after) == sum(before)
    # the oracle loop alone
    cc.assert_coverage(cc.coverage(c, out), "%s n_sub=%d, %d controllers" % (model_name, n_sub, n))
    for key in ("trace", "control_u", "control_out", "opening_v", "path_q", "conc_rows", "irradiance"):
        assert np.all(np.isfinite(out[key])), key
    u = out["control_u"]
    assert (u >= 0.0).all() and (u <= 1.0).all() and np.isfinite(out["rows"][:, info["derived"]]).all()
    assert np.array_equal(out["rows"][:, ct["out_chan"]], out["control_out"])
    # the enable channel drops mid-series: those controllers are off there, with their integrals at zero, and on before and after
    en = ct["en_chan"] >= 0
    off = c["channel"][:, info["c_en"]] == 0.0
    assert 0 < off.sum() < len(off) and not off[0] and not off[-1] and (u[off][:, en] == 0.0).all() and (u[~off][:, en] > 0.0).any()
    # the accumulators are the sums of the returned rows
    acc = out["carry"]["controllers"]
    total = np.zeros(n)
    for r in u:
        total = total + r
    assert np.array_equal(acc["sum_u"], total) and np.array_equal(acc["steps_on"], (u > 0).sum(axis=0)) and np.array_equal(acc["steps_sat"], (u >= 1).sum(axis=0))
    # the margin condition of the cases used against the oracle on the GPU
    gap = cc.margin(c, out)
    print("%s n_sub=%d: least distance of a decision from its threshold %.3e K" % (model_name, n_sub, gap))
    if (model_name, n_sub) in cc.ORACLE_CASES:
        assert gap >= cc.MARGIN, gap


def test_a_cut_loop_equals_the_loop_in_one(oracle):
    c, march, one_, s1 = oracle_loop(oracle, "ragged_mixed", 2)
    s2 = c["st"].copy()
    first = cc.loop_with_rules(march, c, s2, steps=slice(0, 9))
    second = cc.loop_with_rules(march, c, s2, steps=slice(9, None), carry=first["carry"], step_base=0)
    assert np.array_equal(s1, s2)
    for key in ("control_u", "control_out", "opening_v", "irradiance", "trace"):
        assert np.array_equal(one_[key], np.concatenate([first[key], second[key]])), key
    for key in ctl.STATE + ctl.ACC:
        assert np.array_equal(one_["carry"]["controllers"][key], second["carry"]["controllers"][key]), key
    assert np.array_equal(one_["carry"]["sum_irradiance"], second["carry"]["sum_irradiance"])
    mid = first["carry"]["controllers"]
    assert mid["tripped"].any() and (mid["integral"] > 0).any() and (mid["trips"] < one_["carry"]["controllers"]["trips"]).any()
