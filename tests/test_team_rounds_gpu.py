"""Teams of workgroups (layout.hpp, FusedSuper; kernels.hip, fused_zone_phase<TEAM> and the kTeam block loop; batch.hip,
enqueue_fused) where the rest of the suite does not reach them: a team that marches SEVERAL clusters one after the other
(rounds: the round field of the tag, the walk sb += n_teams, the barrier between two clusters in one workgroup's LDS,
the reversed walk), clusters with fewer members than the team (the surplus workgroups skip the round), the three team
kernels for walls with no-mass facings (classes 4 / 10 / 16 beside 1 / 7 / 13), the wrap of the 10-bit launch number in
the tag, calls of one sub-timestep, and a refusal that comes before anything of the call is launched.

A chip holds 56 teams at least, so rounds happen only when HEAT_AMD_TEAM_ROOM shrinks the room. The library reads it once
per process: every case runs in a child of its own (tests/team_rounds_worker.py), one child at a time, started once and
never again. The child marches in calls of 1, 3, 2, 5 and 4 sub-timesteps and holds its state to the oracle at
rtol = atol = 1e-9 with equal no-mass pass counts; the parent reads the team launches off the child's trace — the proof
that the rounds, the team size and the class were the ones meant — and compares the states of the runs of one model BIT
FOR BIT: the members add the partial sums in member order, so how many clusters are marched at a time changes nothing.
"""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "team_rounds_worker.py")

# HEAT_AMD_TEAM_ROOM: workgroups a team launch may hold at once. It may only ever be set BELOW what the chip really holds
# (one or two team workgroups per compute unit: 256 or 512 on an MI355X): a member waits — bounded — for the other members of its team,
# which is sound only while every workgroup of the launch is on the chip at the same time. A value above the real room
# would break that co-residency. The teams a room R gives a class of W members each: (R - R // 8) // W.
#   W = 4: R = 8 -> 1, R = 12 -> 2 (no power of two gives 2: R = 16 -> 3);   W = 6: R = 8 -> 1, R = 16 -> 2, R = 4 -> 0
ROOM_ONE_TEAM = {4: "8", 6: "8"}
ROOM_TWO_TEAMS = {4: "12", 6: "16"}
ROOM_NO_TEAM = "4"
assert all((int(r) - int(r) // 8) // w == 1 for w, r in ROOM_ONE_TEAM.items())
assert all((int(r) - int(r) // 8) // w == 2 for w, r in ROOM_TWO_TEAMS.items())
assert (int(ROOM_NO_TEAM) - int(ROOM_NO_TEAM) // 8) // 6 == 0

CALLS = [1, 3, 2, 5, 4]
TEAM_LINE = re.compile(r"heat_amd: team launch: (\d+) teams of (\d+) workgroups for (\d+) clusters \(class (\d+), (\d+) sub-timesteps\)")

# (rooms, nodes) -> (members per cluster, class of the plain model, class of the faced model): M = 4 / 8 / 16
SHAPES = {(24, 9): (4, 1, 4), (40, 20): (6, 7, 10), (40, 32): (4, 13, 16)}
ROUND_MODELS = ["rounds-%d-%d-%s" % (r, n, f) for (r, n) in SHAPES for f in ("plain", "faced")]
UNEVEN_MODELS = ["uneven-plain", "uneven-faced"]

CONTROL_OF = {"uneven-plain-graph": "uneven-plain", "refuse-room": "uneven-plain"}   # same model, same march
FIRST_TIMEOUT = 600.0   # the control run of a case, whose wall time sets the limit of the runs that follow it
_runs = {}              # (case, env items) -> Run: a child is started once
_control_seconds = {}   # case -> wall time of its control run (the variable unset)
_stopped = []           # why no further child is started (a child that died or hung)


class Run:
    def __init__(self, returncode, stdout, stderr, seconds, out_path):
        self.returncode, self.stdout, self.stderr, self.seconds, self.out_path = returncode, stdout, stderr, seconds, out_path
        self.launches = [tuple(int(x) for x in m.groups()) for m in TEAM_LINE.finditer(stderr)]  # (T, W, C, class, n_sub)
        self.figures = {}
        for line in stdout.splitlines():
            if line.startswith("{"):
                self.figures = json.loads(line)

    def state(self):
        return np.load(self.out_path)

    def check_ok(self):
        assert self.returncode == 0 and "TEAM OK" in self.stdout, "exit %s\n%s\n%s" % (
            self.returncode, self.stdout[-2000:], "\n".join(l for l in self.stderr.splitlines() if "launch:" not in l)[-4000:])


def child(tmp, case, **env):
    """The case in a child with `env` on top of the environment; memoized, and no child is started after one that died."""
    key = (case, tuple(sorted(env.items())))
    if key in _runs:
        return _runs[key]
    if _stopped:
        pytest.fail("not started: " + _stopped[0])
    control = not env
    family = CONTROL_OF.get(case, case)
    if not control and family not in _control_seconds:
        child(tmp, family)
    timeout = FIRST_TIMEOUT if family not in _control_seconds else max(60.0, 10.0 * _control_seconds[family])
    out_path = os.path.join(str(tmp), "%s%s.npy" % (case, "".join("-%s%s" % (k[9:], v) for k, v in key[1])))
    full_env = {k: v for k, v in os.environ.items() if k not in ("HEAT_AMD_TEAM_ROOM", "HEAT_AMD_NO_TEAMS")}
    full_env.update(env, HEAT_AMD_TRACE="1")
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, WORKER, case, out_path], capture_output=True, text=True, timeout=timeout, env=full_env)
    except subprocess.TimeoutExpired:
        _stopped.append("%s %s ran into its limit of %.0f s" % (case, env, timeout))
        _runs[key] = Run(-999, "", "timeout", timeout, out_path)
        pytest.fail(_stopped[0])
    seconds = time.perf_counter() - t0
    if r.returncode < 0 or r.returncode in (134, 139):
        _stopped.append("%s %s died with %d" % (case, env, r.returncode))
    elif r.returncode != 0 and ("gave up waiting" in r.stdout + r.stderr or "illegal memory access" in r.stdout + r.stderr):
        _stopped.append("%s %s reported a device failure" % (case, env))
    run = _runs[key] = Run(r.returncode, r.stdout, r.stderr, seconds, out_path)
    if control:
        _control_seconds[case] = seconds   # (sets the limit of the runs that follow: ten times this, 60 s at least)
    print("%s %s: %.1f s, %s" % (case, env, seconds, run.figures))
    return run


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("team_rounds")


def check_trace(run, teams, members, clusters, klass):
    assert [l[4] for l in run.launches] == CALLS, run.launches
    for T, W, Cn, K, _ in run.launches:
        assert (T, W, Cn, K) == (teams, members, clusters, klass), run.launches


def rooms_of(members):
    return [None, ROOM_ONE_TEAM[members], ROOM_TWO_TEAMS[members]]


def env_of(room):
    return {} if room is None else dict(HEAT_AMD_TEAM_ROOM=room)


@pytest.mark.parametrize("teams", [0, 1, 2], ids=["control", "one_team", "two_teams"])
@pytest.mark.parametrize("model", ROUND_MODELS)
def test_rounds_in_every_team_class(tmp, model, teams):
    """Five clusters marched five, one and two at a time: with one team a workgroup marches five clusters one after the
    other (rounds 0-4), with two the teams take three and two. Plain walls run k_surfaces_fast<M,0,1,0,4,2> (classes 1 /
    7 / 13), walls with facings <M,1,1,0,4,2> (4 / 10 / 16)."""
    _, rooms, n, kind = model.split("-")
    members, plain, faced = SHAPES[(int(rooms), int(n))]
    run = child(tmp, model, **env_of(rooms_of(members)[teams]))
    run.check_ok()
    check_trace(run, teams or 5, members, 5, faced if kind == "faced" else plain)
    if teams:
        assert all(Cn > T for T, _, Cn, _, _ in run.launches)


@pytest.mark.parametrize("model", ROUND_MODELS)
def test_rounds_give_the_same_bits(tmp, model):
    _, rooms, n, _ = model.split("-")
    runs = [child(tmp, model, **env_of(r)) for r in rooms_of(SHAPES[(int(rooms), int(n))][0])]
    states = [r.state() for r in runs]
    assert len({r.launches[0][0] for r in runs}) == 3
    assert np.array_equal(states[0], states[1]) and np.array_equal(states[0], states[2])


@pytest.mark.parametrize("teams", [0, 1, 2], ids=["control", "one_team", "two_teams"])
@pytest.mark.parametrize("model", UNEVEN_MODELS)
def test_uneven_teams(tmp, model, teams):
    """Clusters of 6, 4, 5, 6, 4 and 6 members marched by teams of six: the surplus workgroups of a team skip the cluster
    (and run ahead into the next round); the building of 20 rooms is a plain resident workgroup of another class in the
    same call."""
    run = child(tmp, model, **env_of(rooms_of(6)[teams]))
    run.check_ok()
    check_trace(run, teams or 6, 6, 6, 10 if model == "uneven-faced" else 7)
    assert "of 6 workgroups for 6 clusters" in run.stderr
    assert run.figures["n_fused_launches"] >= 2 * len(CALLS)   # the teams' launch and the plain workgroup's, every call


@pytest.mark.parametrize("model", UNEVEN_MODELS)
def test_uneven_teams_give_the_same_bits(tmp, model):
    runs = [child(tmp, model, **env_of(r)) for r in rooms_of(6)]
    states = [r.state() for r in runs]
    assert len({r.launches[0][0] for r in runs}) == 3
    assert np.array_equal(states[0], states[1]) and np.array_equal(states[0], states[2])


def test_uneven_teams_beside_a_graph(tmp):
    """use_graph=True on the same calls (their lengths differ): the same bits as without."""
    run = child(tmp, "uneven-plain-graph", HEAT_AMD_TEAM_ROOM=ROOM_TWO_TEAMS[6])
    run.check_ok()
    check_trace(run, 2, 6, 6, 7)
    assert np.array_equal(run.state(), child(tmp, "uneven-plain").state())


def test_uneven_teams_over_weather_sites(tmp):
    """Every building a weather site, two teams: a team changes site from round to round."""
    run = child(tmp, "sites", HEAT_AMD_TEAM_ROOM=ROOM_TWO_TEAMS[6])
    run.check_ok()
    check_trace(run, 2, 6, 6, 7)
    control = child(tmp, "sites")
    control.check_ok()
    check_trace(control, 6, 6, 6, 7)
    assert np.array_equal(run.state(), control.state())


def test_launch_number_in_the_tag_wraps(tmp):
    """1030 team launches on one batch: the 10-bit launch number of the tag wraps at the 1024th (the exchange areas are
    cleared, the number skips 0). All in one round, then with one team for the two clusters: the same bits."""
    control = child(tmp, "wrap")
    control.check_ok()
    assert control.figures["n_fused_launches"] >= 1030
    assert len(control.launches) == 1030 and set(control.launches) == {(2, 4, 2, 1, 2)}
    one = child(tmp, "wrap", HEAT_AMD_TEAM_ROOM=ROOM_ONE_TEAM[4])
    one.check_ok()
    assert len(one.launches) == 1030 and set(one.launches) == {(1, 4, 2, 1, 2)}
    assert np.array_equal(control.state(), one.state())


def test_teams_switched_off(tmp):
    """HEAT_AMD_NO_TEAMS: the clusters larger than a workgroup are streamed, and held to the same oracle."""
    run = child(tmp, "uneven-plain", HEAT_AMD_NO_TEAMS="1")
    run.check_ok()
    assert "team launch" not in run.stderr
    assert run.figures["fused_surfaces"] < run.figures["surfaces"]


def test_call_too_long_for_the_tag_is_refused_before_any_launch(tmp):
    """4096 sub-timesteps in one call: refused, the plain resident workgroup of the same call has not marched either (the
    state comes back bit for bit), and the batch then marches a legal series to the oracle's result."""
    run = child(tmp, "refuse-nsub")
    run.check_ok()
    assert run.figures["slots_moved"] == 0 and "4095" in run.figures["message"]
    assert [l[4] for l in run.launches] == CALLS   # the refused call launched no team either


def test_room_for_no_team_is_refused_before_any_launch(tmp):
    run = child(tmp, "refuse-room", HEAT_AMD_TEAM_ROOM=ROOM_NO_TEAM)
    run.check_ok()
    assert run.figures["slots_moved"] == 0 and "not one team" in run.figures["message"]
    assert run.launches == [] and "fused launch" not in run.stderr
