"""The iteration count of the air networks' rule (include/heat_amd.h, heat_air_networks; heat_amd/air_networks.py, apply) on random
networks: the figure max_iter of the tests' cases rests on ("Air networks"). No device, no library.

300 networks of 1 to 40 zones — a random tree of links between zones plus up to n more that close loops, 1 to n / 2 links to
outside behind one of two wind pressures, flow coefficients up to 1.5, heights up to 9 m, p_lin 0.1 Pa, a mass source at one
node in five — are solved at tol = 1e-7 with the rule itself (the elimination of the header, not a library solve): once from
P = 0, and once more from the pressures that solve left after the zone temperatures, the outside temperature and the wind
pressures have moved a little. Prints the worst count of each, the mean of the second and how many solves did not converge
within 40 iterations; every converged solve is checked to leave at most tol of mass at every node.
  python tools/air_networks_prototype.py [networks] [seed]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heat_amd import air_networks as an  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 300
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
TOL = 1e-7
worst0 = worst1 = unconverged = 0
second = []
t0 = time.time()
for trial in range(N):
    n = int(rng.integers(1, 41))
    za, zb = [], []
    for i in range(1, n):
        za.append(i), zb.append(int(rng.integers(0, i)))
    for _ in range(int(rng.integers(0, n + 1))):
        a, b = rng.integers(0, n, 2)
        if a != b:
            za.append(int(a)), zb.append(int(b))
    for _ in range(int(rng.integers(1, max(2, n // 2) + 1))):
        za.append(int(rng.integers(0, n))), zb.append(-1)
    L = len(za)
    zb = np.array(zb)
    nw = dict(net_offset=[0, n], tol=[TOL], max_iter=[40], g_min=[1e-9], node_zone=np.arange(n), zone_a=za, zone_b=zb,
              temp_chan=np.where(zb < 0, 0, -1), wp_chan=np.where(zb < 0, 1 + rng.integers(0, 2, L), -1), c=rng.uniform(0.001, 1.5, L),
              gh=an.G * rng.uniform(0, 9, L), p_lin=np.full(L, 0.1), src_chan=np.where(rng.random(n) < 0.2, 3, -1), src_gain=rng.uniform(-1, 1, n))
    plan = an.structure(nw)
    state = an.fresh(nw)
    T = rng.uniform(15, 30, n)
    row = np.array([rng.uniform(-5, 30), rng.uniform(-10, 10), rng.uniform(-10, 10), 0.05])   # outside C, two wind pressures Pa, a source kg/s
    _, rec = an.apply(T, row, nw, state, plan)
    worst0 = max(worst0, int(rec["net_iters"][0]))
    unconverged += int(not rec["converged"][0])
    assert not rec["converged"][0] or np.abs(an.mass_in(T, row, nw, rec, plan)).max() <= TOL
    T2 = T + rng.uniform(-0.5, 0.5, n)
    row2 = row + np.array([rng.uniform(-1, 1), rng.uniform(-2, 2), rng.uniform(-2, 2), 0])
    _, rec = an.apply(T2, row2, nw, state, plan)
    worst1 = max(worst1, int(rec["net_iters"][0]))
    second.append(int(rec["net_iters"][0]))
    unconverged += int(not rec["converged"][0])
    assert not rec["converged"][0] or np.abs(an.mass_in(T2, row2, nw, rec, plan)).max() <= TOL
print("%d networks, %d solves: at most %d iterations from P = 0, at most %d from the previous pressures (mean %.2f), %d unconverged; %.1f s"
      % (N, 2 * N, worst0, worst1, float(np.mean(second)), unconverged, time.time() - t0))
