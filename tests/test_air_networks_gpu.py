"""Air networks of a series on the GPU (include/heat_amd.h, heat_batch_march_series_networks): per step and per network the device
solves the node pressures that balance the mass flows through all links (k_series_networks<W>, one wavefront per workgroup, lane =
node) and writes every link's volume flow into derived channels of the device's copy of the channel table, which the air paths
read as any channel.

The expected result is DEFINED by air_networks_cases.loop_with_rules — heat_amd.controllers.apply, heat_amd.openings.apply and
heat_amd.air_networks.apply (the header's contracts in numpy, one rounded operation per line), then the existing terms' rules
on the row with its derived columns, applied between per-step march calls to the temperatures the call before returned: through
heat_batch_march_ex the series must agree bit for bit, through OracleModel.march (≙ ThermalModel::march, src/model.rs:359-427)
at rtol = atol = 1e-9, the project's parity bound. tests/test_air_networks_host.py runs the same cases through the oracle alone
and asserts the cases' conditions; they are repeated here on the loop each test compares against. The rule is this project's
own: the reference has no counterpart.

20 zones are networks of 1, 2, 8 and 9 nodes: two launches, each less than a wavefront. 500 zones are 70 networks of 1 to 64
nodes: four launches, every class with a full wavefront of networks and — where a workgroup holds more than one — a ragged last
one (five networks in the class of 16 lanes, three in that of 32; air_networks_cases.wave_shapes, asserted by the host test)."""
import numpy as np
import pytest

from heat_amd import HeatBatch, HeatError, air_networks as an, air_species as asp, binding, controllers as ctl, modeldict as mdl, openings as opn
import air_networks_cases as nc
import air_species_cases as asc
import controllers_cases as cc
import openings_cases as oc
from air_handlers_cases import handlers_with
from test_series_gpu import assert_close, owned_slots, series_kwargs, _id

pytestmark = pytest.mark.gpu

OPTIONS = [dict(), dict(use_graph=True), dict(no_fusion=True)]
LARGE = "rooms_with_windows_large"
N_STEPS = nc.N_STEPS
NAMES = ("trace", "failed_step", "applied", "modes", "air", "irradiance", "sum_irradiance", "handlers", "species", "openings", "controllers",
         "networks")
ROWS = ("link_q", "node_p", "net_iters")


def kwargs(c, steps=slice(None)):
    return series_kwargs(c["channel"], c["drives"], c["probes"], c["a0"], c["b0"], steps=steps)


def series(c, opts, networks="case", steps=slice(None), state=None, carry=None, step_base=0, air=None, **more):
    """One series with the case's loads, air paths, radiation, handlers, species, openings, controllers and `networks` on a fresh
    batch, resumed from `carry` (a loop's, or carried() of a series). Returns (the named result, the final state)."""
    got = c["st"].copy() if state is None else state.copy()
    networks = c["networks"] if isinstance(networks, str) else networks
    loads, handlers, species, openings, radiation = c["loads"], c["handlers"], c["species"], c["openings"], c["radiation"]
    air, controllers = c["air"] if air is None else air, c["controllers"]
    if carry:
        loads = dict(loads, thermostats=dict(loads["thermostats"], mode=carry["modes"]))
        air = dict(air, **{k: carry["air"][k] for k in asc.AIR_ACC})
        handlers = handlers_with(handlers, carry["handlers"])
        species = asc.species_with(species, carry["species"], step_base)
        openings = oc.openings_with(openings, carry["openings"], step_base)
        radiation = dict(radiation, sum_irradiance=carry["sum_irradiance"])
        controllers = cc.controllers_with(controllers, carry["controllers"])
        if networks is not None:
            networks = nc.networks_with(networks, carry["networks"])
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(got)
        out = b.march_series(c["w"][steps], c["n_sub"], loads=loads, air=air, radiation=radiation, handlers=handlers, species=species,
                             openings=openings, controllers=controllers, networks=networks, **dict(kwargs(c, steps), **more))
        b.download_state(got)
    names = NAMES if networks is not None else NAMES[:-1]
    assert len(out) == len(names)
    out = dict(zip(names, out))
    assert out["failed_step"] == -1
    return out, got


def carried(got):
    return dict(modes=got["modes"], air={k: got["air"][k] for k in asc.AIR_ACC}, handlers={k: v for k, v in got["handlers"].items() if v.ndim == 1},
                species={k: got["species"][k] for k in ("conc",) + asp.ACC}, openings={k: got["openings"][k] for k in opn.ACC},
                sum_irradiance=got["sum_irradiance"], controllers={k: got["controllers"][k] for k in ctl.STATE + ctl.ACC},
                networks={k: got["networks"][k] for k in an.STATE + an.ACC})


def same(ref, got, what, close=None):
    """A loop's result against a series': the discrete outputs exactly; the rows, sums and state bit for bit, or through close."""
    def value(r, g, name):
        if close is None:
            assert np.array_equal(r, g, equal_nan=True), "%s %s: %d differ, worst %.3e" % (what, name, int((r != g).sum()), np.nanmax(np.abs(r - g)))
        else:
            close(r, g, "%s %s" % (what, name))

    acc = ref["carry"]
    its = got["networks"]["net_iters"]
    if close is None:
        for key in ("iters_sum", "unconverged"):
            assert np.array_equal(acc["networks"][key], got["networks"][key]), "%s %s" % (what, key)
        assert np.array_equal(ref["net_iters"], its), "%s net_iters: %d differ" % (what, int((ref["net_iters"] != its).sum()))
    else:
        # tol = 0.0: a solve runs its max_iter iterations unless a residual is 0.0 EXACTLY, which the last bit of a temperature
        # decides (in the oracle loop about one solve in ten ends so, at an iteration of its own). The counts are therefore
        # held to what does not hang on that bit: every count within [1, max_iter], iters_sum the sum of the rows, and
        # "unconverged" exactly the solves that ran to max_iter; a solve that stopped too early or ran on from other pressures
        # shows in link_q and node_p, which are compared at the bound below. The counts themselves are compared bit for bit
        # against the per-call loop (close is None), where nothing differs by a bit.
        top = nc.MAX_ITER
        print("%s: %d of %d solves stop early in the loop, %d in the series, %d counts differ" % (
            what, int((ref["net_iters"] < top).sum()), its.size, int((its < top).sum()), int((ref["net_iters"] != its).sum())))
        assert ((its >= 1) & (its <= top)).all(), "%s net_iters outside [1, %d]" % (what, top)
        assert np.array_equal(got["networks"]["iters_sum"], its.sum(axis=0)), "%s iters_sum" % what
        assert np.array_equal(got["networks"]["unconverged"], (its == top).sum(axis=0)), "%s unconverged" % what
    for key in ("tripped", "steps_on", "steps_sat", "trips"):
        assert np.array_equal(acc["controllers"][key], got["controllers"][key]), "%s %s" % (what, key)
    for key in asc.DISCRETE:
        assert np.array_equal(acc["species"][key], got["species"][key]), "%s %s" % (what, key)
    assert np.array_equal(acc["modes"], got["modes"]), "%s modes" % what
    for key in ("state", "steps_open", "switches"):
        assert np.array_equal(acc["air"][key], got["air"][key]), "%s air %s" % (what, key)
    value(ref["link_q"], got["networks"]["link_q"], "link_q")
    value(ref["node_p"], got["networks"]["node_p"], "node_p")
    for key in ("pressure", "sum_ab", "sum_ba", "max_res"):
        value(acc["networks"][key], got["networks"][key], key)
    value(ref["control_u"], got["controllers"]["control_u"], "control_u")
    value(ref["opening_v"], got["openings"]["opening_v"], "opening_v")
    value(ref["irradiance"], got["irradiance"], "irradiance")
    value(ref["path_q"], got["air"]["path_q"], "path_q")
    value(ref["applied"], got["applied"], "applied")
    value(ref["branch_q"], got["handlers"]["branch_q"], "branch_q")
    for key in asp.ROWS:
        value(ref[key], got["species"][key], key)
    for key in asc.REAL:
        value(acc["species"][key], got["species"][key], key)
    value(ref["trace"], got["trace"], "trace")


# ---- 1. bit for bit against the per-call loop ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", [("ragged_mixed", 2), ("ragged_mixed", 5), (LARGE, 2), (LARGE, 5)])
def test_series_with_networks_equals_the_per_call_path_bit_for_bit(model, n_sub, opts):
    c = nc.case(model, N_STEPS, n_sub, 2, nc.SEED, floor=False)
    sizes = sorted(c["networks_info"]["sizes"].tolist())
    assert (sizes == [1, 2, 8, 9] and model == "ragged_mixed") or (set(nc.SIZES[500]) <= set(sizes) and sum(sizes) == 500 and model == LARGE)
    own = owned_slots(c["md"])
    ref_state = c["st"].copy()
    with HeatBatch(c["md"], **opts) as b:
        b.upload_state(ref_state)
        ref = nc.loop_with_rules(lambda s, wk, za, zb: b.march(s, wk, za, zb, outputs=b.OUT_ALL), c, ref_state)
    nc.assert_coverage(nc.coverage(c, ref), "%s n_sub=%d (per-call path)" % (model, n_sub))
    got, state = series(c, opts)
    same(ref, got, model)
    assert np.array_equal(ref_state[own], state[own]), "%d state slots differ" % int((ref_state[own] != state[own]).sum())


# ---- 2. the oracle loop ----
_ORACLE_LOOPS = {}


def oracle_loop(oracle, model, n_sub):
    c = nc.case(model, N_STEPS, n_sub, 2, nc.SEED, tol=0.0)
    if (model, n_sub) not in _ORACLE_LOOPS:  # (the same for every option set; left unchanged)
        m = oracle.OracleModel(c["md"])

        def march(s, wk, za, zb):
            assert m.march(s, wk, za, zb, threads=1)[0] == 0

        state = c["st"].copy()
        _ORACLE_LOOPS[(model, n_sub)] = (nc.loop_with_rules(march, c, state), state)
    return (c,) + _ORACLE_LOOPS[(model, n_sub)]


@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("model,n_sub", nc.ORACLE_CASES)
def test_series_with_networks_matches_the_oracle_loop(oracle, model, n_sub, opts):
    """rtol = atol = 1e-9 with tol = 0.0 and max_iter = 24: a solve runs its 24 iterations unless its residual is 0.0 exactly,
    so a last-bit difference in a temperature cannot move an exit by more than that — the discontinuity DESIGN.md §7 describes
    for the no-mass loop — and every p_lin is at least 0.1 Pa: dq/ddp <= c / (2 sqrt(p_lin)) <= 2.4 for the cases' largest c of
    1.5, ddp/dT ~ gh rho / T <= 0.4 Pa/K, so a 1e-12 K difference moves a flow by about 1e-12. The decisions of the controllers
    and of the controlled paths keep 1e-6 K from their thresholds in the oracle loop (asserted here on the loop compared
    against)."""
    c, ref, ref_state = oracle_loop(oracle, model, n_sub)
    assert nc.margin(c, ref) >= nc.MARGIN
    assert float(np.min(c["networks"]["p_lin"])) >= 0.1 and float(np.max(c["networks"]["c"])) <= nc.C_MAX
    nc.assert_coverage(nc.coverage(c, ref), "%s n_sub=%d (oracle loop)" % (model, n_sub), tol=0.0)
    got, state = series(c, opts)
    same(ref, got, model, close=assert_close)
    own = owned_slots(c["md"])
    assert_close(ref_state[own], state[own], "%s final state" % model)


# ---- 3. cut ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
@pytest.mark.parametrize("cut", [7, 15])
def test_series_with_networks_cut_in_two_equals_the_series_in_one(cut, opts):
    c = nc.case("ragged_mixed", N_STEPS, 2, 2, nc.SEED, floor=False)
    one, state1 = series(c, opts)
    first, mid = series(c, opts, steps=slice(0, cut))
    second, state2 = series(c, opts, steps=slice(cut, None), state=mid, carry=carried(first), step_base=cut)
    at_cut = first["networks"]
    assert (at_cut["pressure"] != 0).all() and (at_cut["iters_sum"] < one["networks"]["iters_sum"]).all() and (at_cut["sum_ab"] > 0).any()
    assert np.array_equal(one["trace"], np.concatenate([first["trace"], second["trace"]]))
    for key in ROWS:     # (a solve that started from other pressures, or with dold carried over, would take other iterations)
        assert np.array_equal(one["networks"][key], np.concatenate([first["networks"][key], second["networks"][key]])), key
    for key in an.STATE + an.ACC:
        assert np.array_equal(one["networks"][key], second["networks"][key]), key
    assert np.array_equal(one["air"]["path_q"], np.concatenate([first["air"]["path_q"], second["air"]["path_q"]]))
    assert np.array_equal(state1, state2)


# ---- 4. no networks ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_no_networks_is_the_series_with_controllers_bit_for_bit(opts):
    c = oc.case("rooms_with_windows", 12, 3, 2, 5, floor=False)
    C, dp = binding.C, binding._dp
    results = []
    for how in ("plain", "empty", "controllers_abi", "networks_abi"):
        state = c["st"].copy()
        with HeatBatch(c["md"], **opts) as b:
            b.upload_state(state)
            terms = dict(loads=c["loads"], air=c["air"], handlers=c["handlers"], species=c["species"], openings=c["openings"])
            if how == "plain":
                trace, failed, applied, modes, air, hd, sp, op = b.march_series(c["w"], 3, **terms, **kwargs(c))
            elif how == "empty":
                trace, failed, applied, modes, air, hd, sp, op, nw = b.march_series(c["w"], 3, networks={}, **terms, **kwargs(c))
                assert nw["link_q"].shape == (12, 0) and nw["node_p"].shape == (12, 0) and nw["net_iters"].shape == (12, 0)
                assert nw["net_iters"].dtype == np.int32 and nw["pressure"].size == 0
            else:  # ct == NULL and nw == NULL through the C ABI: the controllers' entry point, and the new one behind it
                s, keep = binding.make_series(c["w"], 3, **kwargs(c))
                l, lkeep = binding.make_zone_loads(**c["loads"])
                a, akeep = binding.make_air_paths(**c["air"])
                h, hkeep = binding.make_air_handlers(**c["handlers"])
                spc, spkeep = binding.make_air_species(**c["species"])
                opc, opkeep = binding.make_openings(**c["openings"])
                Z = int(c["md"]["n_zones"])
                trace, applied, f = np.zeros((12, len(c["probes"]))), np.zeros((12, l.n_thermostats)), C.c_int32(7)
                path_q, branch_q, conc_rows = np.zeros((12, a.n_paths)), np.zeros((12, h.n_branches)), np.zeros((12, spc.n_species, Z))
                opening_v = np.zeros((12, opc.n_openings))
                call = binding.SeriesCall(size=C.sizeof(binding.SeriesCall), s=C.pointer(s), l=C.pointer(l), air=C.pointer(a), failed_step=C.pointer(f),
                                          trace=trace.ctypes.data_as(dp), applied=applied.ctypes.data_as(dp), path_q=path_q.ctypes.data_as(dp))
                args = (b._h, C.byref(call), None, None, None, C.byref(h), None, None, None, branch_q.ctypes.data_as(dp), C.byref(spc),
                        conc_rows.ctypes.data_as(dp), None, None, C.byref(opc), opening_v.ctypes.data_as(dp), None, None, None)
                if how == "controllers_abi":
                    assert b._L.heat_batch_march_series_controllers(*args) == 0
                else:
                    assert b._L.heat_batch_march_series_networks(*args, None, None, None, None) == 0
                failed, modes = f.value, lkeep["th_mode"]
                air = dict(path_q=path_q, **{k: akeep[k] for k in asc.AIR_ACC})
                hd = dict(branch_q=branch_q, bypass=hkeep["bypass"])
                sp = dict(conc_rows=conc_rows, **{k: spkeep[k] for k in ("conc",) + asp.ACC})
                op = dict(opening_v=opening_v, **{k: opkeep[k] for k in opn.ACC})
            b.download_state(state)
        assert failed == -1
        results.append((trace, applied, modes, state, hd["branch_q"], hd["bypass"], sp["conc_rows"], op["opening_v"]) +
                       tuple(sp[k] for k in ("conc",) + asp.ACC) + tuple(op[k] for k in opn.ACC) + tuple(air[k] for k in ("path_q",) + asc.AIR_ACC))
    for other in results[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(results[0], other))


# ---- 5. nullable outputs ----
@pytest.mark.parametrize("opts", OPTIONS, ids=_id)
def test_an_array_that_is_not_asked_for_changes_no_bit_of_the_others(opts):
    c = nc.case("ragged_mixed", N_STEPS, 2, 2, nc.SEED, floor=False)
    full, state = series(c, opts)
    n = an.counts(c["networks"])
    every = binding.NETWORK_STATS
    for state_names, stats, rows in (((), (), ()), (("pressure",), ("sum_ab",), ("link_q",)), ((), ("sum_ba", "max_res"), ("node_p",)),
                                     (("pressure",), ("iters_sum", "unconverged"), ("net_iters",)), (binding.NETWORK_STATE, every, ()),
                                     ((), (), ROWS)):
        got, st = series(c, opts, networks=dict(c["networks"], state=state_names, stats=stats), **{k: k in rows for k in ROWS})
        assert set(got["networks"]) == set(ROWS) | set(state_names) | set(stats)
        for key, width in zip(ROWS, (n["link"], n["node"], n["net"])):
            assert got["networks"][key].shape == ((N_STEPS if key in rows else 0), width)
        for key, v in got["networks"].items():
            if v.size:
                assert np.array_equal(v, full["networks"][key]), (state_names, stats, key)
        assert np.array_equal(got["trace"], full["trace"]) and np.array_equal(got["applied"], full["applied"]) and np.array_equal(st, state)
        assert np.array_equal(got["air"]["path_q"], full["air"]["path_q"]) and np.array_equal(got["species"]["conc"], full["species"]["conc"])


# ---- 6. refusals ----
def test_bad_networks_and_sharded_batches_are_refused_and_leave_the_device_untouched():
    md, st = mdl.clustered_massive(200, Z=8, seed=3)
    w, channel = np.zeros((2, 1, 3)), np.zeros((2, 10))
    channel[:, 0] = 5.0
    ok = dict(net_offset=[0, 2, 3], tol=[1e-7, 1e-7], max_iter=[24, 24], g_min=[1e-9, 1e-9], node_zone=[1, 4, 6], zone_a=[1, 1, 4, 6],
              zone_b=[4, -1, -1, -1], temp_chan=[-1, 0, 0, 0], frac_chan=[-1, 9, -1, -1], out_ab=[5, -1, -1, -1], out_ba=[6, 7, -1, 8],
              c=[0.5, 0.02, 0.03, 0.02], gh=[9.81, 4.0, 20.0, 9.81], p_lin=[0.1] * 4)
    op = dict(zone_a=[2], zone_b=[-1], temp_chan=[0], out_chan=[4], area=[0.5], cs=[9.0], c0=[0.01])
    ct = dict(sense_index=[1], set_chan=[1], out_chan=[9], kp=[0.5], out_hi=[1.0])
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        for bad, code, needle in ((dict(ok, node_zone=[1, 4, 8]), -4, "node 2:"),
                                  (dict(ok, node_zone=[1, 4, 4]), -4, "node 2:"),
                                  (dict(ok, net_offset=[0, 3, 3]), -4, "network 1:"),
                                  (dict(ok, max_iter=[24, 65]), -1, "network 1:"),
                                  (dict(ok, g_min=[0.0, 1e-9]), -1, "network 0:"),
                                  (dict(ok, tol=[1e-7, -1.0]), -1, "network 1:"),
                                  (dict(ok, zone_b=[6, -1, -1, -1]), -4, "link 0:"),             # another network's zone
                                  (dict(ok, zone_a=[1, 1, 4, 2]), -4, "link 3:"),                # a zone of no network
                                  (dict(ok, zone_b=[1, -1, -1, -1]), -1, "link 0:"),             # zone_a == zone_b
                                  (dict(ok, temp_chan=[-1, -1, 0, 0]), -4, "link 1:"),
                                  (dict(ok, temp_chan=[0, 0, 0, 0]), -4, "link 0:"),
                                  (dict(ok, zone_b=[4, -1, -1, 0]), -4, "link 3:"),              # into a zone of no network
                                  (dict(ok, out_ba=[6, 6, -1, 8]), -4, "link 1:"),               # two writers
                                  (dict(ok, out_ba=[6, 4, -1, 8]), -4, "link 1:"),               # the opening's
                                  (dict(ok, out_ab=[9, -1, -1, -1]), -4, "link 0:"),             # the controller's
                                  (dict(ok, frac_chan=[-1, 4, -1, -1]), -4, "link 1:"),          # reads an opening's
                                  (dict(ok, frac_chan=[-1, 8, -1, -1]), -4, "link 1:"),          # reads a network's
                                  (dict(ok, c=[0.5, -0.02, 0.03, 0.02]), -1, "link 1:"),
                                  (dict(ok, p_lin=[0.1, 0.1, 0.0, 0.1]), -1, "link 2:"),
                                  (dict(ok, gh=[9.81, 4.0, np.inf, 9.81]), -1, "link 2:"),
                                  (dict(ok, resume=dict(an.fresh(ok), pressure=[0.0, np.nan, 0.0])), -1, "node 1:")):
            with pytest.raises(HeatError) as e:
                b.march_series(w, 1, channel=channel, openings=op, controllers=ct, networks=bad)
            assert e.value.code == code and needle in str(e.value), (str(e.value), needle)
        # an opening or a controller that reads a network's derived channel: the networks run behind both
        for kw in (dict(openings=dict(op, frac_chan=[7])), dict(controllers=dict(ct, en_chan=[5]))):
            with pytest.raises(HeatError) as e:
                b.march_series(w, 1, channel=channel, **dict(dict(openings=op, controllers=ct, networks=ok), **kw))
            assert e.value.code == -4 and "link" in str(e.value) and "run behind" in str(e.value), str(e.value)
        got = st.copy()
        own = owned_slots(md)
        got[own] = np.nan                                             # (a download writes the slots the device owns, and only those)
        b.download_state(got)
        assert np.array_equal(got, st)
        # the batch marches on: a good term afterwards
        trace, failed, o, cr, nw = b.march_series(w, 1, channel=channel, openings=op, controllers=ct, networks=ok, probes=md["zone_slot"])
        assert failed == -1 and np.isfinite(nw["link_q"]).all() and (nw["net_iters"] > 0).all() and (nw["unconverged"] == 0).all()
    ranks, _ = binding.partition(md, 2)
    with HeatBatch(md, n_ranks=2, rank=0, rank_of_surface=ranks) as b:
        with pytest.raises(HeatError) as e:
            b.march_series(w, 1, channel=channel, networks=ok)
        assert e.value.code == -1 and "sharded" in str(e.value)


# ---- 7. unread channels ----
def test_derived_channels_that_nothing_reads_change_no_bit_of_the_march():
    c = nc.case("ragged_mixed", N_STEPS, 2, 2, nc.SEED, floor=False)
    info = c["networks_info"]
    air = {k: (np.asarray(v)[:info["paths"][0]] if k != "state" else v) for k, v in c["air"].items()}      # without the networks' paths
    air = {k: v for k, v in air.items() if k in ("target", "source", "temp_chan", "volume_chan", "volume_gain", "open_chan", "sense", "band", "min_delta")}
    with_nw, s1 = series(c, {}, air=air)
    without, s0 = series(c, {}, networks=None, air=air)
    assert np.isfinite(with_nw["networks"]["link_q"]).all() and (with_nw["networks"]["link_q"] != 0).any()
    assert np.array_equal(with_nw["trace"], without["trace"]) and np.array_equal(s1, s0)
    assert np.array_equal(with_nw["air"]["path_q"], without["air"]["path_q"]) and np.array_equal(with_nw["species"]["conc"], without["species"]["conc"])


# ---- 8. edge steps ----
def test_a_series_of_no_sub_timestep_still_solves_every_step():
    c = nc.case("ragged_mixed", 6, 0, 2, 21, floor=False)
    ref = nc.loop_with_rules(lambda s, wk, za, zb: None, c, c["st"].copy())          # nothing marches: every step sees the start
    state = c["st"].copy()
    with HeatBatch(c["md"]) as b:
        b.upload_state(state)
        got = dict(zip(NAMES, b.march_series(None, 0, n_steps=6, loads=c["loads"], air=c["air"], radiation=c["radiation"], handlers=c["handlers"],
                                             species=c["species"], openings=c["openings"], controllers=c["controllers"], networks=c["networks"],
                                             **kwargs(c))))
        b.download_state(state)
    own = owned_slots(c["md"])
    assert got["failed_step"] == -1 and np.array_equal(state[own], c["st"][own]) and (ref["net_iters"] > 0).all()
    for key in ROWS:
        assert np.array_equal(ref[key], got["networks"][key]), key
    assert np.array_equal(ref["path_q"], got["air"]["path_q"])
    for key in an.STATE + an.ACC:
        assert np.array_equal(ref["carry"]["networks"][key], got["networks"][key]), key


def test_a_nan_outside_temperature_is_data_in_its_network_until_a_path_reads_it():
    """Two networks of one zone each with two links to outside at two heights. A NaN outside temperature of the first makes
    both of its flows NaN — every residual of the network is NaN, which never raises res, so the solve stops at once — and its
    pressure stays as it was; the second network knows nothing of it. Read by nothing the NaNs stay in their rows; read by an
    air path they make the zone's a0 NaN, which is HEAT_N_NAN_ZONE at that step."""
    md, st = mdl.clustered_massive(700, Z=28, dt=45.0, seed=3)
    n_steps, j = 6, 3
    channel = np.tile([5.0, 8.0, np.nan, np.nan], (n_steps, 1))           # two outside temperatures, two derived channels
    channel[j, 0] = np.nan
    nw = dict(net_offset=[0, 1, 2], tol=[1e-7, 1e-7], max_iter=[24, 24], g_min=[1e-9, 1e-9], node_zone=[13, 5], zone_a=[13, 13, 5, 5],
              zone_b=[-1, -1, -1, -1], temp_chan=[0, 0, 1, 1], out_ba=[2, -1, 3, -1], c=[0.02, 0.02, 0.03, 0.03], gh=[5.0, 25.0, 5.0, 25.0],
              p_lin=[0.01] * 4)
    w = mdl.weather_series(n_steps * 2, 45.0).reshape(n_steps, 2, 3)
    with HeatBatch(md) as b:
        b.upload_state(st.copy())
        trace, failed, got = b.march_series(w, 2, networks=nw, channel=channel, probes=md["zone_slot"])
        assert failed == -1 and np.isfinite(trace).all()
        q, it = got["link_q"], got["net_iters"]
        assert np.isnan(q[j, :2]).all() and np.isfinite(np.delete(q[:, :2], j, axis=0)).all() and np.isfinite(q[:, 2:]).all()
        assert it[j, 0] == 0 and (np.delete(it[:, 0], j) > 0).all() and np.array_equal(got["node_p"][j, 0], got["node_p"][j - 1, 0])
        assert (q[:, 0] * q[:, 1] < 0)[np.arange(n_steps) != j].all()       # the stack: in below, out above
        assert np.isnan(got["sum_ba"][0]) and np.isfinite(got["sum_ba"][2]) and (got["unconverged"] == 0).all()
        for n_sub in (0, 1):
            b.upload_state(st.copy())
            with pytest.raises(HeatError) as e:
                b.march_series(w[:, :n_sub] if n_sub else None, n_sub, networks=nw, air=dict(an_paths(nw)), channel=channel, probes=md["zone_slot"],
                               **(dict(n_steps=n_steps) if n_sub == 0 else {}))
            assert e.value.failed_step == j and e.value.code == 3 and b.failed_surface() == (13, 3), (n_sub, str(e.value))


def an_paths(nw):
    return {k: v for k, v in an.paths(nw).items() if k != "link"}


# ---- 9. the two ends of the launch geometry ----
def chain(zones, rng, c0):
    """One network over `zones`: a chain of doorways, a link to outside at each end and at every fifth node; channels c0 (the
    outside temperature) and c0 + 1 (a wind pressure)."""
    n = len(zones)
    za = list(zones[1:]) + [zones[i] for i in range(0, n, 5)] + [zones[-1]]
    zb = list(zones[:-1]) + [-1] * (len(za) - (n - 1))
    zb = np.asarray(zb)
    L = len(za)
    return dict(net_offset=[0, n], tol=[1e-7], max_iter=[24], g_min=[1e-9], node_zone=zones, zone_a=za, zone_b=zb, temp_chan=np.where(zb < 0, c0, -1),
                wp_chan=np.where((zb < 0) & (np.arange(L) % 2 == 0), c0 + 1, -1), c=np.where(zb < 0, 0.02, 0.3) * rng.uniform(0.5, 1.5, L),
                gh=rng.uniform(0.0, 60.0, L), p_lin=np.full(L, 0.05))


@pytest.mark.parametrize("shape", ["one_of_64", "65_of_1"])
def test_a_single_network_of_64_nodes_and_65_networks_of_one_node(shape):
    md, st = mdl.clustered_massive(1300, Z=65, dt=45.0, seed=7)
    rng = np.random.default_rng(11)
    n_steps = 4
    T = st[md["zone_slot"]] + rng.uniform(-3.0, 3.0, 65)
    st = st.copy()
    st[md["zone_slot"]] = T
    channel = np.concatenate([rng.uniform(0.0, 12.0, (n_steps, 1)), rng.uniform(-5.0, 5.0, (n_steps, 1))], axis=1)
    if shape == "one_of_64":
        nw = chain(rng.permutation(65)[:64], rng, 0)
    else:
        nw = an.concat(*[chain(np.array([z]), rng, 0) for z in rng.permutation(65)])
    sizes = np.diff(nw["net_offset"])
    assert (sizes.tolist() == [64]) if shape == "one_of_64" else (sizes.tolist() == [1] * 65)
    acc = an.fresh(nw)
    plan = an.structure(nw)
    want = []
    for k in range(n_steps):
        _, r = an.apply(T, channel[k], nw, acc, plan)
        an.accumulate(r, acc)
        want.append(r)
    with HeatBatch(md) as b:
        b.upload_state(st)
        trace, failed, got = b.march_series(None, 0, n_steps=n_steps, networks=nw, channel=channel)
    assert failed == -1 and all(r["converged"].all() for r in want) and max(int(r["net_iters"].max()) for r in want) >= 3
    for key in ROWS:
        assert np.array_equal(np.stack([r[key] for r in want]), got[key]), key
    for key in an.STATE + an.ACC:
        assert np.array_equal(acc[key], got[key]), key
