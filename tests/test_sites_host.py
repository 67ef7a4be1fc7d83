"""Weather sites on the host (include/heat_amd.h, heat_batch_create_sites): the new entry points are exported and bound,
bad arguments are refused with the documented codes before any device work, and the planner keeps every tile, workgroup
and team of one site — under AddressSanitizer / UBSan in a child process, like tests/test_planner_host.py. No GPU needed.

Reference: a batch of K sites is K reference models (src/model.rs:359-427) marched in lockstep, each reading its own
weather (model.rs:369-382)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from heat_amd import binding, build as hb, modeldict as mdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("heat_batch_create_sites", "heat_batch_n_sites", "heat_plan_check_sites")


def _asan_runtime():
    out = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return out if os.path.isabs(out) and os.path.exists(out) else None


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "heat_amd.h")).read()
    bound = {name for name, _, _ in binding.SYMBOLS}
    L = binding.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in bound, name
        assert getattr(L, name) is not None
    assert "heat_plan_check_sites" in binding.HOST_ONLY_SYMBOLS


@pytest.fixture(scope="module")
def model():
    md, _ = mdl.clustered_massive(200, Z=8, seed=3)
    return md


def _code(fn):
    with pytest.raises(binding.HeatError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("n_sites", [0, -1, 65537])
def test_bad_site_count_is_refused(model, n_sites):
    code, _ = _code(lambda: binding.plan_check_sites(model, n_sites, np.zeros(200, np.int32)))
    assert code == -1  # HEAT_E_INVALID_ARG


@pytest.mark.parametrize("bad", [-1, 4, 1 << 20])
def test_site_out_of_range_is_refused_naming_the_surface(model, bad):
    site = np.zeros(200, np.int32)
    site[137] = bad
    code, msg = _code(lambda: binding.plan_check_sites(model, 4, site))
    assert code == -4 and "surface 137" in msg, msg  # HEAT_E_SIZE


def test_sharded_batch_of_sites_is_refused(model):
    code, _ = _code(lambda: binding.plan_check_sites(model, 2, np.zeros(200, np.int32), n_ranks=2))
    assert code == -1


def test_create_sites_refuses_before_any_device_work(model):
    """The argument checks come first: they answer the same with or without a device."""
    L = binding.load_library()
    desc, keep = binding.make_desc(model)
    opt = binding.make_options()
    h = C.c_void_p()
    site = np.zeros(200, np.int32)
    site[5] = 9
    assert L.heat_batch_create_sites(C.byref(desc), C.byref(opt), 4, site.ctypes.data_as(binding._i32p), C.byref(h)) == -4
    assert b"surface 5" in L.heat_last_error()
    assert L.heat_batch_create_sites(C.byref(desc), C.byref(opt), 0, site.ctypes.data_as(binding._i32p), C.byref(h)) == -1
    assert not h.value


def test_one_site_is_the_plan_without_sites(model):
    for opts in (dict(), dict(fuse_always=True), dict(no_fusion=True)):
        assert binding.plan_check_sites(model, 1, np.zeros(200, np.int32), **opts) == binding.plan_check(model, **opts)


def test_sites_split_workgroups_and_mixed_site_clusters_stream():
    parts = [mdl.clustered_massive(300, Z=12, seed=s)[0] for s in range(3)]
    md, site = mdl.concat(parts)
    one = binding.plan_check(md, fuse_always=True)
    three = binding.plan_check_sites(md, 3, site, fuse_always=True)
    assert three[5] == one[5] > 0     # every cluster is of one site: all of them still fused
    assert three[6] >= one[6]         # ... in workgroups that never mix two sites
    # every surface of a cluster on another site than its neighbour: the clusters stream
    alt = (np.arange(md["n_surfaces"]) % 2).astype(np.int32)
    mixed = binding.plan_check_sites(md, 2, alt, fuse_always=True)
    assert mixed[5] < one[5]


def test_concat_renumbers_zones_cavities_and_slots():
    a, sa = mdl.glazing_cavity(30, Z=2, seed=1)
    b, sb = mdl.clustered_massive(40, Z=4, seed=2)
    for interleave in (False, True):
        md, site = mdl.concat([a, b], interleave=interleave)
        assert md["n_surfaces"] == 70 and md["n_zones"] == 6 and md["n_state"] == len(sa) + len(sb)
        assert np.bincount(site).tolist() == [30, 40]
        if interleave:
            assert site[:4].tolist() == [0, 1, 0, 1]
        on_b = site == 1
        assert md["first_node_slot"][on_b].min() >= len(sa) and md["first_node_slot"][~on_b].max() < len(sa)
        sp = md["back_kind"] == mdl.SPACE
        assert (md["back_zone"][sp & on_b] >= 2).all() and (md["back_zone"][sp & ~on_b] < 2).all()
        assert len(md["cavities"]) == len(a["cavities"])
        assert md["seg_cavity"].max() < len(md["cavities"])
        binding.plan_check_sites(md, 2, site)


def test_multi_site_weather_must_name_its_sites():
    """A batch of several sites takes weather [n_sub, n_sites, 3] only: flat records would be read as fewer
    sub-timesteps of all sites."""
    arr, n = binding.as_weather(np.zeros((7, 4, 3)), 4)
    assert n == 7 and len(arr) == 28
    for bad in (np.zeros((8, 3)), np.zeros((28, 3)), np.zeros((7, 2, 3)), np.zeros((7, 4, 2))):
        with pytest.raises(ValueError):
            binding.as_weather(bad, 4)
    assert binding.as_weather(np.zeros((5, 3)), 1)[1] == 5
    assert binding.as_weather(np.zeros((5, 1, 3)), 1)[1] == 5


def test_weather_sites_differ_and_turn_walls_windward_and_leeward():
    w = mdl.weather_sites(20, 45.0, 16, seed=4)
    assert w.shape == (20, 16, 3)
    assert np.ptp(w[0, :, 0]) > 1.0 and np.ptp(w[0, :, 2]) > 0.5 and (w[:, :, 2] >= 0).all()
    # a wall facing +x is windward where sin(wd) > 0 (surface.rs:37-46): some sites one way, some the other
    windward = np.sin(w[0, :, 1]) > 0
    assert windward.any() and (~windward).any()


def test_sites_planner_under_address_and_ub_sanitizers():
    asan = _asan_runtime()
    if asan is None:
        pytest.skip("gcc has no libasan here")
    lib = hb.build_plan_host()
    env = dict(os.environ)
    env["LD_PRELOAD"] = asan
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sites_host_worker.py"), lib], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-6000:])
    assert "plans verified" in out.stdout
