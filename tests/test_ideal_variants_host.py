"""Every ideal-loads instantiation of the cluster-resident march, on the host: the cases of tests/ideal_variants_cases.py plan
as their table says, together they reach all 18 IDEAL instantiations of k_surfaces_fast, and their inputs discriminate — the
CPU reference of every case heats, cools, floats and saturates in part at both call lengths. What fails here would otherwise
show on the GPU as a test that marches another kernel than it names, or one whose loads never act. No GPU needed: the plan
comes from heat::make_plan through tests/plan_lists_shim.cpp (helpers.plan_lists), the reference from tests/ideal_loads_ref.py."""
import numpy as np
import pytest

import helpers
import ideal_variants_cases as ivc
from heat_amd import binding, modeldict as mdl
from test_ideal_resident_gpu import hold_to_the_reference

ALL_18 = {(M, v, w) for M in (4, 8, 16) for v in ("nm0", "nm1", "mixed") for w in (4, 8)}


@pytest.mark.parametrize("name", sorted(ivc.CASES))
def test_every_case_plans_as_its_table_entry_says(name):
    md, _ = ivc.model_of(name)
    plan, claimed = ivc.plan_of(name), ivc.CASES[name][2]
    print(name, int(md["n_surfaces"]), "walls:", plan)
    assert plan["lists"] == claimed                          # the (class, list) set, and the workgroups of every list
    assert plan["teams"] == 0 and plan["stream_tiles"] == 0 and plan["reason"] == binding.IDEAL_RESIDENT_OK
    assert int(md["n_surfaces"]) <= 480
    # the shim's answer is the library's own
    assert binding.plan_ideal_resident(md, **ivc.options_of(name)) == (True, binding.IDEAL_RESIDENT_OK)
    assert binding.plan_check(md, **ivc.options_of(name))[5] == md["n_surfaces"]     # every surface resident
    if name in ivc.INSTANTIATIONS:
        M, variant, waves = name.split("-")
        assert (int(M[1:]), variant, int(waves[:-1])) in {helpers.instantiation_of(c, g2) for c, g2 in plan["lists"]}
    if name == "zones32":
        assert plan["most_zones"] == 32                      # kFusedMaxZones: the last element of every per-zone LDS array
    if name.startswith("glazing"):
        assert plan["resident_cavity_tiles"] > 0 and md["cavities"] is not None and len(md["cavities"]) > 0
        assert all(g2 >> 1 for _, g2 in plan["lists"])       # ... in mixed workgroups only
    if name.startswith("queue"):
        assert len(plan["lists"]) == 1 and min(plan["lists"].values()) > 3   # more blocks than HEAT_AMD_FUSED_ROOM=3


def test_the_cases_reach_all_18_instantiations():
    reached = {}
    for name in ivc.INSTANTIATIONS:
        for c, g2 in ivc.plan_of(name)["lists"]:
            reached.setdefault(helpers.instantiation_of(c, g2), []).append(name)
    assert len(ivc.INSTANTIATIONS) == 18 and set(reached) == ALL_18, sorted(ALL_18 - set(reached))
    # the arithmetic of instantiation_of on the classes themselves: six classes per blocking factor, three per nm
    assert [helpers.instantiation_of(c, 0)[:2] for c in (0, 3, 6, 9, 12, 15)] == [(4, "nm0"), (4, "nm1"), (8, "nm0"), (8, "nm1"),
                                                                                  (16, "nm0"), (16, "nm1")]
    assert helpers.instantiation_of(16, 3) == (16, "mixed", 8) and helpers.instantiation_of(16, 1) == (16, "nm1", 8)


def test_the_shim_tells_a_batch_that_is_not_eligible():
    """(the shim is not a constant: teams, streamed tiles and the reason come out where a plan has them)"""
    teams = helpers.plan_lists(mdl.partitioned_buildings(2 * 40 * 12, 32, rooms=40, walls_per_room=12, dt=45.0, seed=64)[0],
                               nodes_per_lane=16, fuse_always=True)
    assert teams["teams"] > 0 and teams["reason"] == binding.IDEAL_RESIDENT_TEAMS
    streamed = helpers.plan_lists(mdl.ragged_mixed(700, Z=20, seed=5)[0], no_fusion=True)
    assert streamed["lists"] == {} and streamed["stream_tiles"] > 0 and streamed["reason"] == binding.IDEAL_RESIDENT_NONE_PLANNED


def test_the_model_of_the_all_terms_call_is_eligible():
    """tests/test_ideal_variants_gpu.py marches tests/test_series_all_terms_gpu.py's fused case with the opt-in."""
    import ambient_cases as ac
    c = ac.case("clustered_massive-fuse_always")
    plan = helpers.plan_lists(c.md, **c.opts)
    print(plan)
    assert plan["reason"] == binding.IDEAL_RESIDENT_OK and plan["teams"] == 0
    # plain workgroups of four wavefronts at 8 and 16 nodes per lane, with and without facings (and a few more)
    assert {(7, 0), (10, 0), (13, 0), (16, 0)} <= set(plan["lists"]) and all(g2 == 0 for _, g2 in plan["lists"])


@pytest.mark.parametrize("n_sub,n_steps", ivc.CALLS)
@pytest.mark.parametrize("name", sorted(n for n in ivc.CASES if not n.startswith("queue")))
def test_the_reference_of_every_case_discriminates(oracle, name, n_sub, n_steps):
    c = ivc.build(oracle, name, n_steps, n_sub)
    ref, ideal = c.ref, c.args[8]
    print("%s n_sub=%d: %d loads; heating %d, cooling %d, floating %d; saturated %d + %d; smallest |need - cap| / S = %.3g" % (
        name, n_sub, len(ideal["zone"]), ref["n_heat"], ref["n_cool"], ref["n_free"], ref["n_sat_heating"].sum(), ref["n_sat_cooling"].sum(),
        ref["margin"]))
    assert sorted(ideal["zone"]) == list(range(int(c.args[0]["n_zones"])))           # a load on every zone
    assert np.isfinite(ideal["heat_cap"]).any() and np.isfinite(ideal["cool_cap"]).any()
    assert np.isinf(ideal["heat_cap"]).any() and np.isinf(ideal["cool_cap"]).any()
    holds = ivc.preconditions(ref)
    assert all(holds.values()), holds
    # ... and these ARE the preconditions of hold_to_the_reference: the reference held to itself passes every assertion
    md, n_sub_ = c.args[0], n_sub
    hold_to_the_reference(name, md, n_sub_, ideal, ref, c.ref_state, dict(ref, ideal=ref), c.ref_state)


@pytest.mark.parametrize("name", ["M4-nm1-4w", "M8-nm1-8w", "M16-nm1-8w", "queue-nm1-8w"])
def test_with_facings_gives_mass_free_end_nodes_and_the_oracle_marches_them(oracle, name):
    md, st = ivc.model_of(name)
    unfaced = ivc.CASES[name.replace("nm1", "nm0")][0] if name in ivc.INSTANTIATIONS else ivc.pb(480, 32, 8)
    plain, _ = unfaced()                                                             # the same walls before the conversion
    off = np.asarray(md["node_offset"], dtype=np.int64)
    first, last = off[:-1], off[1:] - 1
    faced = np.zeros(int(md["n_surfaces"]), bool)
    faced[ivc.faced_walls(md)] = True
    assert faced.sum() == (int(md["n_surfaces"]) + 2) // 3
    mass, u = np.asarray(md["mass"]), np.asarray(md["uvalue"])
    assert np.all(mass[first[faced]] == 0.0) and np.all(mass[last[faced]] == 0.0)
    assert np.all(mass[first[~faced]] > 0.0) and np.all(mass[last[~faced]] > 0.0)
    inner = np.ones(len(mass), bool)
    inner[first[faced]] = inner[last[faced]] = False
    assert np.all(mass[inner] > 0.0)                                                 # one-node facings, nothing else without mass
    # the neighbours hold half an element's mass — what the end node of the all-massive wall held; the facing's segments
    # have U in [0.5, 3]; the emissivities are scaled
    pm = np.asarray(plain["mass"])
    assert np.array_equal(mass[first[faced] + 1], pm[first[faced]]) and np.array_equal(mass[last[faced] - 1], pm[last[faced]])
    for seg in (first[faced], last[faced] - 1):
        assert np.all((u[seg] >= 0.5) & (u[seg] <= 3.0))
    for k in ("front_emissivity", "back_emissivity"):
        assert np.array_equal(np.asarray(md[k])[faced], np.asarray(plain[k])[faced] * (0.2 / 0.9))
        assert np.array_equal(np.asarray(md[k])[~faced], np.asarray(plain[k])[~faced])
    got = st.copy()
    rc, iters = oracle.OracleModel(md).march(got, mdl.weather_series(6, md["dt"]))
    assert rc == 0 and iters > 0 and np.all(np.isfinite(got))
    zs = md["zone_slot"]
    assert not np.array_equal(got[zs], st[zs])
