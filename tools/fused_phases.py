"""Where a cluster-resident workgroup spends its time, and the clock the chip holds meanwhile (diagnostic build with
in-kernel stamps, heat_amd/build.py build_stamps; the product library carries none):
    python tools/fused_phases.py [CONFIG] [P] [SLOTS]
Per FusedBlock: shader-clock ticks of init (loads, palette decode, zone data -> LDS), of the P sub-timesteps, and of the
final write-back; in-kernel clock = d(s_memtime) / d(s_memrealtime) x 100 MHz over the block's lifetime. Wavefront 0
also adds up, over the march, the ticks it waited at the zone phase's opening barrier and the ticks between the phase's
two barriers (the serial zone chain the whole workgroup waits for): p10 / median / p90 per sub-timestep. The launch is
set against n_blocks x median life / slots, the time the workgroups would take packed without a gap."""
import os, sys, types, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from heat_amd import build as _hb
# (built on demand: __graft_entry__.build() treats it as optional; HEAT_AMD_LIB names another stamped build, for an A/B)
os.environ["HEAT_AMD_LIB"] = os.environ.get("HEAT_AMD_LIB") or _hb.build_stamps()
import numpy as np
import bench
from heat_amd import HeatBatch, modeldict as mdl, binding
cfg = sys.argv[1] if len(sys.argv) > 1 else "headline"
P = int(sys.argv[2]) if len(sys.argv) > 2 else 20
md, st, _ = bench.build_config(cfg, types.SimpleNamespace(surfaces=1_000_000, nodes=32), 45.0, 20260401)
w = mdl.weather_series(P, float(md["dt"]))
with HeatBatch(md, use_graph=True) as b:
    b.upload_state(st)
    for _ in range(60):          # the clock the chip settles at under this load, not the one it starts with
        b.march_resident(w)
    b.synchronize()
    b.set_timing(True)
    b.march_resident(w); b.synchronize()
    us, _, _ = b.get_timing()
    L = binding.load_library()
    nb = 65536
    SPB = 16  # kStampsPerBlock
    buf = np.zeros(nb * SPB, dtype=np.uint64)
    L.heat_debug_stamps.restype = C.c_int
    assert L.heat_debug_stamps(buf.ctypes.data_as(C.c_void_p), C.c_int(nb)) == 0
    s = buf.reshape(nb, SPB)
    s = s[s[:, 3] > 0].astype(np.float64)
    n_blocks = len(s)
    ok = (s[:, 1] > s[:, 0]) & (s[:, 2] > s[:, 1]) & (s[:, 3] > s[:, 2]) & (s[:, 5] > s[:, 4])
    s = s[ok]  # (a slot is indexed by first tile / 4: workgroups of fewer than four tiles can share one — dropped where they mixed)
    clk = (s[:, 3] - s[:, 0]) / np.maximum(s[:, 5] - s[:, 4], 1.0) * 100e6
    print("%s, %d sub-timesteps per launch: %d stamped workgroups, launch %.1f us (%.2f us per sub-timestep)"
          % (cfg, P, len(s), us * P, us))
    print("in-kernel clock: median %.3f GHz (p10 %.3f, p90 %.3f)" % (np.median(clk) / 1e9, np.percentile(clk, 10) / 1e9, np.percentile(clk, 90) / 1e9))
    whole = s[:, 3] - s[:, 0]
    if (s[:, 6] > s[:, 0]).all() and (s[:, 7] >= s[:, 6]).all() and (s[:, 1] >= s[:, 7]).all():
        for name, a, e in (("  init: loads arrived", 0, 6), ("  init: palettes decoded", 6, 7), ("  init: zone data, barrier", 7, 1)):
            x = s[:, e] - s[:, a]
            print("%-28s median %9.0f ticks" % (name, np.median(x)))
    for name, a, e in (("init", 0, 1), ("sub-timesteps", 1, 2), ("write-back", 2, 3), ("whole", 0, 3)):
        x = s[:, e] - s[:, a]
        print("%-14s median %9.0f ticks = %6.2f us (%5.1f %% of the workgroup's life)%s" % (
            name, np.median(x), np.median(x) / np.median(clk) * 1e6, 100.0 * np.median(x) / np.median(whole),
            "   %.0f ticks per sub-timestep" % (np.median(x) / P) if name == "sub-timesteps" else ""))
    for name, k in (("zone chain per sub-timestep", 9), ("wait at its opening barrier", 8)):
        x = s[:, k] / P
        print("%-28s p10 %7.0f  median %7.0f  p90 %7.0f ticks" % (name, np.percentile(x, 10), np.median(x), np.percentile(x, 90)))
    life_us = np.median(whole) / np.median(clk) * 1e6
    slots = int(sys.argv[3]) if len(sys.argv) > 3 else 512  # workgroups the chip holds at once (256 compute units x 2)
    print("launch %.1f us against n_blocks x life / slots = %d x %.2f / %d = %.1f us packed" % (
        us * P, n_blocks, life_us, slots, n_blocks * life_us / slots))
