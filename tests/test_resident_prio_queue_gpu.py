"""The cluster-resident march where its zone work runs at raised priority (kernels.hip, fused_zone_phase) and where its
workgroups take their blocks from the work queue (batch.hip, enqueue_fused; layout.hpp, FusedArgs::queue), at the
smallest shapes that reach each placement:

  priority   the wavefront-per-zone branch with wavefronts that have a zone and wavefronts that have none, a cluster of
             fewer zones than wavefronts with a partly filled last wavefront, the row-per-zone branch with rows that
             hold no zone (rooms of 12 and 9 walls), workgroups with small-surface wavefronts, and teams, whose members
             poll for each other's sums and therefore stay at priority 0 — one pass (10 zones a member) and two passes
             (more than 16 zones in a member), odd and even numbers of sub-timesteps
  queue      ten clusters on three workgroups (HEAT_AMD_FUSED_ROOM=3, and HEAT_AMD_FUSED_PERSIST=1: from calls of one
             sub-timestep on), blocks of 1, 3 and 4 working wavefronts mixed, so that wavefronts without a tile stay and
             loop; two consecutive calls (the second walks the list from its end, and starts from the tickets the first
             one drew) of 1, 2 and 5 sub-timesteps

Every case runs in a child of its own (tests/resident_prio_queue_worker.py) under a time limit, started once: a
priority or a barrier count that went wrong shows as a march that does not come back. The child holds its state to the
oracle at rtol = atol = 1e-9 (as tests/test_resident_lds_gpu.py does) and asserts that every wall was marched resident;
the parent reads the launches off the child's trace and holds a queue case to the same model marched without the queue
BIT FOR BIT: clusters are independent, so which workgroup takes which block, and in which order, changes nothing.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "resident_prio_queue_worker.py")
TIMEOUT = 180.0
FUSED_LINE = re.compile(r"heat_amd: fused launch( on the work queue)?: (\d+) workgroups for (\d+) blocks \(class (\d+), list (\d+), (\d+) sub-timesteps\)")
TEAM_LINE = re.compile(r"heat_amd: team launch: (\d+) teams of (\d+) workgroups for (\d+) clusters \(class (\d+), (\d+) sub-timesteps\)")
_runs = {}
_stopped = []  # why no further child is started (a child that died or hung)


class Run:
    def __init__(self, returncode, stdout, stderr, out_path):
        self.returncode, self.stdout, self.stderr, self.out_path = returncode, stdout, stderr, out_path
        # (queued, workgroups, blocks, class, list, n_sub) / (teams, members, clusters, class, n_sub)
        self.fused = [(bool(m.group(1)),) + tuple(int(x) for x in m.groups()[1:]) for m in FUSED_LINE.finditer(stderr)]
        self.teams = [tuple(int(x) for x in m.groups()) for m in TEAM_LINE.finditer(stderr)]
        self.figures = {}
        for line in stdout.splitlines():
            if line.startswith("{"):
                self.figures = json.loads(line)

    def state(self):
        return np.load(self.out_path)

    def check_ok(self):
        assert self.returncode == 0 and "RESIDENT OK" in self.stdout, "exit %s\n%s\n%s" % (
            self.returncode, self.stdout[-2000:], "\n".join(l for l in self.stderr.splitlines() if "launch" not in l)[-4000:])


def child(tmp, case, **env):
    key = (case, tuple(sorted(env.items())))
    if key in _runs:
        return _runs[key]
    if _stopped:
        pytest.fail("not started: " + _stopped[0])
    out_path = os.path.join(str(tmp), "%s%s.npy" % (case, "".join("-%s" % v for _, v in key[1])))
    full_env = {k: v for k, v in os.environ.items() if k not in ("HEAT_AMD_FUSED_ROOM", "HEAT_AMD_FUSED_RESERVE", "HEAT_AMD_FUSED_PERSIST")}
    full_env.update(env, HEAT_AMD_TRACE="1")
    try:
        r = subprocess.run([sys.executable, WORKER, case, out_path], capture_output=True, text=True, timeout=TIMEOUT, env=full_env)
    except subprocess.TimeoutExpired:
        _stopped.append("%s %s ran into its limit of %.0f s" % (case, env, TIMEOUT))
        _runs[key] = Run(-999, "", "timeout", out_path)
        pytest.fail(_stopped[0])
    if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in r.stdout + r.stderr:
        _stopped.append("%s %s died with %d" % (case, env, r.returncode))
    run = _runs[key] = Run(r.returncode, r.stdout, r.stderr, out_path)
    return run


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("resident_prio_queue")


@pytest.mark.parametrize("case", ["chain", "fewzones", "rows-12", "rows-9", "small"])
def test_zone_work_at_raised_priority(tmp, case):
    run = child(tmp, case)
    run.check_ok()
    assert run.fused and not run.teams and not any(q for q, *_ in run.fused), run.fused


@pytest.mark.parametrize("n_sub", [3, 4])
@pytest.mark.parametrize("rooms,n,per_room,two_pass", [(40, 32, 12, False), (60, 8, 6, True)])
def test_teams_never_wait_at_raised_priority(tmp, rooms, n, per_room, two_pass, n_sub):
    """Two clusters marched by teams, an odd and an even number of sub-timesteps (the exchange areas alternate). 40 rooms
    of 12 walls of 32 nodes: four members of 10 zones each, a row meets one zone (one pass); 60 rooms of 6 walls of 8
    nodes: three members of 20 zones — more than 16 — which sum and publish in one pass and gather in a second."""
    run = child(tmp, "teams-%d-%d-%d-%d" % (rooms, n, per_room, n_sub))
    run.check_ok()
    assert len(run.teams) == 1, run.stderr[-2000:]
    teams, members, clusters, _, subs = run.teams[0]
    assert (teams, clusters, subs) == (2, 2, n_sub), run.teams
    assert (rooms / members > 16) == two_pass, run.teams


@pytest.mark.parametrize("n_sub", [1, 2, 5])
def test_work_queue_gives_the_bits_of_one_workgroup_per_block(tmp, n_sub):
    queued = child(tmp, "queue-%d" % n_sub, HEAT_AMD_FUSED_ROOM="3", HEAT_AMD_FUSED_PERSIST="1")
    queued.check_ok()
    assert queued.fused == [(True, 3, 10, queued.fused[0][3], queued.fused[0][4], n_sub)] * 2, queued.fused
    plain = child(tmp, "queue-%d" % n_sub)
    plain.check_ok()
    assert plain.fused == [(False, 10, 10, queued.fused[0][3], queued.fused[0][4], n_sub)] * 2, plain.fused
    assert np.array_equal(queued.state(), plain.state())
