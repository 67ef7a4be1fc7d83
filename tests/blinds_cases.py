"""The cases of the blind tests (include/heat_amd.h, heat_blinds), shared by tests/test_blinds_host.py — which builds them on the
CPU alone and asserts their coverage on synthetic zone temperatures — and tests/test_blinds_gpu.py.

A case starts from shades_cases.shades_case (channels, sky-driven inputs, apertures, receivers, 150 shades). Blinds of every kind
are added by pattern, in shuffled shade order; their thresholds come from the quantiles of the pattern's own irradiance on the
shade's plane (which does not depend on any zone: it is known before a march), their setpoints lie around the model's zone
temperatures. The reference is a LOOP WITH FEEDBACK (`loop`): before march call k it reads the zone temperatures the state
holds, applies heat_amd.blinds.apply — the rule in numpy —, forms the shaded inputs of that step with sky.incident(..., shade=)
and solar_gains.transmitted(..., shade=) / received from the effective factors, writes them into the state and marches. No
device is needed to build a case."""
from types import SimpleNamespace

import numpy as np

import shades_cases as sc
from heat_amd import blinds as bl, sky, solar_gains
from test_series_gpu import INPUTS, term_row, write_inputs
from test_solar_gains_gpu import EN, SOLAR

N_STEPS = sc.N_SUNS
N_BLINDS = 97          # of sc.N_SHADES = 150 shades: some keep no blind; neither is a multiple of 64
SHARED_AT = 4          # the blind on sc.SHARED (a shade that serves two sides and an aperture): controlled, gated by a zone
KINDS = ("scheduled in [0, 1]", "scheduled beyond [0, 1]", "controlled", "controlled, enable channel", "controlled, zone",
         "controlled, zone, enable channel", "controlled, zone, band 0")
ACC = ("steps_closed", "switches", "sum_position")


def blinds_case(md, st, rng, n_steps=N_STEPS, channel=None, drives=None, sunny=False):
    """Returns a namespace: md, state, channel (the shades case's table plus the blinds' columns), call / ref_drives, args,
    gains, shades, blinds (a dict of binding.make_blinds' arguments), kind [n_blinds], f [n_steps, n_shades] (geometric) and
    I [n_steps, n_shades] (blinds.incident_on). sunny: no record holds a negative diffuse or ground value (the skies of
    test_sky_gpu have some, for the clamps): whatever a blind does then lowers what its consumers receive."""
    Z = int(md["n_zones"])
    channel, call, ref, args, gains, shades = sc.shades_case(md, rng, n_steps, channel, drives)
    NS, NB = sc.N_SHADES, N_BLINDS
    if sunny:
        args["record"][..., sky.DIFFUSE:sky.GROUND + 1] = np.abs(args["record"][..., sky.DIFFUSE:sky.GROUND + 1])
    f = sc.sunlit_of(shades, args["record"])
    I = bl.incident_on(shades, args["record"], f)
    assert not np.isnan(I).any()
    # ---- the blinds' channels, behind the case's own ----
    C0 = channel.shape[1]
    T0 = np.asarray(st)[md["zone_slot"]]
    steps = np.arange(n_steps)
    pos_in = rng.uniform(0.0, 1.0, n_steps)
    pos_in[::6] = np.resize((0.0, 1.0, 0.25, 0.5), len(pos_in[::6]))
    pos_out = rng.uniform(-0.5, 1.5, n_steps)
    pos_out[1::5] = np.resize((-0.25, 1.75, -0.0, 2.0), len(pos_out[1::5]))
    enable_a = np.where((steps // 5) % 2 == 0, 1.0, np.where(steps % 2 == 0, 0.0, -1.0))      # on for five steps, off for five
    enable_b = np.where((steps + 3) % 7 < 5, rng.uniform(0.1, 2.0, n_steps), 0.0)
    centre = float(np.median(T0))
    # (off the centre itself: the zones of some models all start at one temperature, and a setpoint on it would be a tie)
    setpoints = np.stack([centre + rng.uniform(-1.5, 1.5, n_steps), centre + 0.21 + 10.0 * steps / n_steps + np.sin(steps * 0.9),
                          np.full(n_steps, centre + 0.37)], axis=1)       # (the second one rises as the zones of these models do)
    channel = np.concatenate([channel, np.stack([pos_in, pos_out, enable_a, enable_b], axis=1), setpoints], axis=1)
    POS_IN, POS_OUT, EN_A, EN_B, SET = C0, C0 + 1, C0 + 2, C0 + 3, C0 + 4
    # ---- the blinds, in shuffled shade order ----
    shade = rng.permutation(NS)[:NB].astype(np.int32)
    if sc.SHARED in shade:
        shade[np.flatnonzero(shade == sc.SHARED)[0]] = shade[SHARED_AT]
    shade[SHARED_AT] = sc.SHARED
    i = np.arange(NB)
    kind = i % len(KINDS)
    assert kind[SHARED_AT] == 4
    scheduled, gated = kind < 2, kind >= 4
    pos_chan = np.where(kind == 0, POS_IN, np.where(kind == 1, POS_OUT, -1)).astype(np.int32)
    enable_chan = np.where(kind == 3, EN_A, np.where(kind == 5, EN_B, -1)).astype(np.int32)
    zone = np.where(gated, rng.integers(0, Z, NB), -1).astype(np.int32)
    set_chan = np.where(gated, SET + i % 3, -1).astype(np.int32)
    band = np.where(kind == 6, 0.0, rng.uniform(0.1, 1.0, NB))
    closed = {}
    for a, name in enumerate(("beam_closed", "diffuse_closed", "ground_closed")):
        v = rng.uniform(0.02, 0.6, NB)
        v[(i + a) % 5 == 0] = 0.0
        v[(i + a) % 11 == 3] = 1.0
        closed[name] = v
    # thresholds between two neighbouring values of the pattern's own I on the blind's shade: no comparison is near a tie
    irr_close, irr_open = np.zeros(NB), np.zeros(NB)
    for n in range(NB):
        v = np.unique(I[:, shade[n]])
        assert len(v) >= 8
        hi = int(rng.integers(len(v) // 2, len(v) - 2))
        lo = int(rng.integers(1, max(2, hi - 1)))
        irr_close[n], irr_open[n] = 0.5 * (v[hi] + v[hi + 1]), 0.5 * (v[lo] + v[lo - 1])
    assert np.all(irr_open <= irr_close)
    blinds = dict(shade=shade, pos_chan=pos_chan, irr_close=irr_close, irr_open=irr_open, zone=zone, set_chan=set_chan, band=band,
                  enable_chan=enable_chan, **closed)
    # ---- the pattern ----
    assert NB % 64 != 0 and NS % 64 != 0 and len(set(shade)) == NB < NS and not np.array_equal(shade, np.sort(shade))
    assert all((kind == q).sum() >= 10 for q in range(len(KINDS)))
    assert ((pos_in > 0) & (pos_in < 1)).any() and (pos_out < 0).any() and (pos_out > 1).any()
    for v in closed.values():
        assert (v == 0.0).any() and (v == 1.0).any() and ((v > 0) & (v < 1)).any()
    front, back, ap = shades["front_shade"], shades["back_shade"], shades["aperture_shade"]
    assert (front == sc.SHARED).sum() >= 1 and (back == sc.SHARED).sum() >= 1 and (ap == sc.SHARED).sum() >= 1
    blinded = np.zeros(NS, bool)
    blinded[shade] = True
    used = np.concatenate([front[front >= 0], back[back >= 0], ap[ap >= 0]])
    assert blinded[used].any() and (~blinded[used]).any()                    # consumers with and without a blind on their shade
    return SimpleNamespace(md=md, state=np.asarray(st), channel=channel, call=call, ref_drives=ref, args=args, gains=gains,
                           shades=shades, blinds=blinds, kind=kind, f=f, I=I, n_steps=n_steps)


def fresh(n):
    """The in/out arrays of n blinds at the start of a run: state and the three accumulators."""
    return dict(state=np.zeros(n, np.uint8), steps_closed=np.zeros(n, np.int64), switches=np.zeros(n, np.int64), sum_position=np.zeros(n))


def reference_rows(c, eff, steps):
    """The shaded sky and the shaded gains of the steps `steps` as channel rows, as shades_cases.reference forms them for a
    whole series — with the EFFECTIVE factors eff = (f', fd', fg'), [len(steps), n_shades] each, in place of the shades' own.
    Returns the widened rows, the drives that read them and the transmitted powers [len(steps), n_apertures]."""
    md, args, gains, shades = c.md, c.args, c.gains, c.shades
    S = int(md["n_surfaces"])
    rec, mode, normals = args["record"][steps], args["mode"], args["normals"]
    rec = rec[:, np.zeros(S, np.int64), :]                                   # (one site: the sites test loops per site)
    pick = lambda j: tuple(e[:, j] for e in eff)
    side_shade = dict(solar_front=shades.get("front_shade"), solar_back=shades.get("back_shade"))
    cols, base, out = [c.channel[steps]], c.channel.shape[1], {}
    for bit, (name, _) in enumerate(INPUTS):
        chan, gain = c.ref_drives[name]
        on = np.flatnonzero(mode >> bit & 1)
        v = sky.incident(rec[:, on, :], tuple(n[on] for n in normals), name)
        if side_shade.get(name) is not None:
            j = np.asarray(side_shade[name])[on]
            sel = np.flatnonzero(j >= 0)
            at = on[sel]
            v[:, sel] = sky.incident(rec[:, at, :], tuple(n[at] for n in normals), name, shade=pick(j[sel]))
        chan = chan.copy()
        chan[on] = base + np.arange(len(on))
        base += len(on)
        cols.append(v)
        out[name] = (chan, gain)
    ap_rec = rec[:, gains["ap_surface"], :]
    ap = (gains["ap_normal"], gains["ap_tau_coef"], gains["ap_tau_diffuse"], gains["ap_scale"])
    pb, pd = solar_gains.transmitted(ap_rec, *ap)
    j = np.asarray(shades["aperture_shade"])
    sel = np.flatnonzero(j >= 0)
    one = (tuple(n[sel] for n in ap[0]), ap[1][sel], ap[2][sel], ap[3][sel])
    pb[:, sel], pd[:, sel] = solar_gains.transmitted(ap_rec[:, sel, :], *one, shade=pick(j[sel]))
    v, has = solar_gains.received(pb, pd, n_surfaces=S, **{k: gains[k] for k in EN})
    for side, name in enumerate(SOLAR):
        chan, gain = out[name]
        on = np.flatnonzero(has[side])
        assert np.all(chan[on] < 0)
        chan = chan.copy()
        chan[on] = base + np.arange(len(on))
        base += len(on)
        cols.append(v[:, side, on])
        out[name] = (chan, gain)
    return np.concatenate(cols, axis=1), out, pb + pd


def loop(c, state, march, probes, carry=None, steps=None, blinds=None, ap_sum=None):
    """The loop with feedback a blinded series replaces. march(state, k): one march call of step k on `state`, in place (the
    library's per-call path, the oracle, or a stand-in that only moves the zone temperatures). carry: fresh() or what an
    earlier loop returned under "carry" (it is copied). Returns a dict: trace, position, incident, transmitted (rows of the
    steps run), ap_sum, carry (state and accumulators afterwards), margin (blinds.apply's) and the (f', fd', fg') rows."""
    md = c.md
    blinds = c.blinds if blinds is None else blinds
    NB = len(blinds["shade"])
    steps = range(c.n_steps) if steps is None else steps
    carry = {k: v.copy() for k, v in (fresh(NB) if carry is None else carry).items()}
    out = dict(trace=np.zeros((len(steps), len(probes))), position=np.zeros((len(steps), NB)), incident=np.zeros((len(steps), NB)),
               transmitted=np.zeros((len(steps), len(c.gains["ap_surface"]))), eff=[], margin={})
    total = np.zeros(len(c.gains["ap_surface"])) if ap_sum is None else np.array(ap_sum, dtype=np.float64)
    for n, k in enumerate(steps):
        T = state[md["zone_slot"]].copy()
        before = carry["state"].copy()
        p, fe, fde, fge = bl.apply(c.I[k], T, c.channel[k], blinds, carry["state"], c.f[k], c.shades, margin=out["margin"])
        bl.accumulate(p, carry["state"], before, carry["sum_position"], carry["steps_closed"], carry["switches"])
        rows, drives, tp = reference_rows(c, (fe[None], fde[None], fge[None]), [k])
        write_inputs(md, state, 0, rows, drives)
        march(state, k)
        out["trace"][n], out["position"][n], out["incident"][n], out["transmitted"][n] = state[probes], p, c.I[k][blinds["shade"]], tp[0]
        out["eff"].append((fe, fde, fge))
        total = total + tp[0]
    out["ap_sum"], out["carry"] = total, carry
    return out


def marcher(b, c, w, a0=None, b0=None):
    """march(state, k) through the library's per-call path."""
    return lambda state, k: b.march(state, w[k], term_row(a0, k), term_row(b0, k), outputs=b.OUT_ALL)


def oracle_marcher(m, w, a0=None, b0=None, count=None):
    """march(state, k) through the oracle; count (a list) collects the no-mass passes."""
    def march(state, k):
        rc, it = m.march(state, w[k], term_row(a0, k), term_row(b0, k))
        assert rc == 0
        if count is not None:
            count.append(it)
    return march


def blinded_kwargs(c, probes, a0=None, b0=None, steps=slice(None), ap_sum=None, blinds=None, carry=None, **more):
    """The arguments of HeatBatch.march_series for the case: shades_cases.shaded_kwargs plus blinds (with `carry` as their
    state and accumulators)."""
    kw = sc.shaded_kwargs(c.channel, c.call, probes, a0, b0, c.args, c.gains, c.shades, steps, ap_sum)
    blinds = dict(c.blinds if blinds is None else blinds)
    if carry is not None:
        blinds.update({k: carry[k] for k in ("state",) + ACC if k in carry})
    return dict(kw, blinds=blinds, **more)


def same_blinds(ref, got, what=""):
    """Asserts that a loop's result (`loop`) and the "blinds" dict of a series hold the same bits."""
    for key in ("position", "incident"):
        bad = ~((ref[key] == got[key]) | (np.isnan(ref[key]) & np.isnan(got[key])))
        assert not bad.any(), "%s%s: %d values differ" % (what, key, int(bad.sum()))
    for key in ("state",) + ACC:
        assert np.array_equal(ref["carry"][key], got[key]), "%s%s: %d values differ" % (what, key, int((ref["carry"][key] != got[key]).sum()))


def coverage(c, ref):
    """What a loop's result took of the rule, as a dict of counts (asserted by the tests on their own results)."""
    p, kind = ref["position"], c.kind
    ctl = kind >= 2
    s = p[:, ctl]
    d = np.diff(np.concatenate([np.zeros((1, s.shape[1])), s]), axis=0)
    I = ref["incident"][:, ctl]
    between = (I > c.blinds["irr_open"][ctl]) & (I <= c.blinds["irr_close"][ctl])
    return dict(closed=int((d > 0).sum()), reopened=int((d < 0).sum()), both=int(((d > 0).any(axis=0) & (d < 0).any(axis=0)).sum()),
                held=int(((s == 1) & (d == 0) & between).sum()),
                fractional=int(((p[:, kind == 0] > 0) & (p[:, kind == 0] < 1)).sum()),
                clamped=int(((p[:, kind == 1] == 0) | (p[:, kind == 1] == 1)).sum()))
