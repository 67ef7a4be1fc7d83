"""The cases of the anisotropic-sky tests (include/heat_amd.h, heat_sky_aniso), shared by tests/test_sky_aniso_host.py — which
builds them on the CPU alone and asserts their coverage on synthetic zone temperatures — and tests/test_sky_aniso_gpu.py.

A case starts from blinds_cases.blinds_case (channels, sky-driven inputs, apertures, receivers, 150 shades, 97 blinds whose
thresholds lie between the values of the ISOTROPIC irradiance on their shades). Added by pattern: one coefficient pair per step
— significant circumsolar fractions, horizon coefficients of both signs, one step of two zeros — and random bands per side,
aperture and shade, some of them zero. The suns are the shade pattern's own: above cos 85 deg, between it and the horizon, below
the horizon, behind planes, one NaN. The reference is blinds_cases' LOOP WITH FEEDBACK with the anisotropic rule of
heat_amd/sky.py, solar_gains.py and blinds.py (each with aniso=) in place of the isotropic one. No device is needed to build a
case."""
from types import SimpleNamespace

import numpy as np

import blinds_cases as bc
import shades_cases as sc
from heat_amd import blinds as bl, sky, solar_gains
from test_series_gpu import INPUTS, write_inputs
from test_solar_gains_gpu import EN, SOLAR

N_STEPS = bc.N_STEPS
ZERO_STEP = 3          # the step whose pair is (0, 0): the isotropic bits
BANDS = ("front_band", "back_band", "aperture_band", "shade_band")


def aniso_case(md, st, rng, **more):
    """blinds_case plus coef [n_steps, 1, 2], bands (a dict of the four arrays), I (the ANISOTROPIC irradiance on the shades'
    planes, [n_steps, n_shades]) and I_iso (the isotropic one the thresholds were drawn from)."""
    return widen(bc.blinds_case(md, st, rng, **more), rng)


def widen(c, rng):
    """Adds the anisotropic sky to a blinds case, in place. Returns it."""
    md = c.md
    S, NA, NS = int(md["n_surfaces"]), len(c.gains["ap_surface"]), sc.N_SHADES
    n = c.n_steps
    coef = np.stack([rng.uniform(0.15, 0.7, n), rng.uniform(-0.1, 0.35, n)], axis=1)
    coef[ZERO_STEP] = 0.0
    coef[ZERO_STEP + 7] = (0.4, 0.0)                                       # Hay-Davies: no horizon term
    bands = {}
    for key, count in zip(BANDS, (S, S, NA, NS)):
        v = rng.uniform(0.0, 1.0, count)
        v[::5] = 0.0
        bands[key] = v
    c.coef, c.bands, c.I_iso = coef[:, None, :], bands, c.I
    c.I = bl.incident_on(c.shades, c.args["record"], c.f, aniso=(coef[:, None, 0], coef[:, None, 1], bands["shade_band"]))
    assert not np.isnan(c.I).any() and not np.array_equal(c.I, c.I_iso) and np.array_equal(c.I[ZERO_STEP], c.I_iso[ZERO_STEP])
    return c


def aniso_kwargs(c, steps=slice(None)):
    return dict(coef=c.coef[steps], **c.bands)


def reference_rows(c, eff, steps):
    """blinds_cases.reference_rows with the anisotropic rule: the sky-driven solar sides and the apertures of the steps `steps`
    take the steps' pairs and their own bands; the long-wave sides are as they were."""
    md, args, gains, shades = c.md, c.args, c.gains, c.shades
    S = int(md["n_surfaces"])
    rec, mode, normals = args["record"][steps], args["mode"], args["normals"]
    rec = rec[:, np.zeros(S, np.int64), :]                                   # (one site: the sites test loops per site)
    circ, horiz = c.coef[steps][:, 0, :1], c.coef[steps][:, 0, 1:]           # [len(steps), 1]: one pair per step
    pick = lambda j: tuple(e[:, j] for e in eff)
    side_shade = dict(solar_front=shades.get("front_shade"), solar_back=shades.get("back_shade"))
    side_band = dict(solar_front=c.bands["front_band"], solar_back=c.bands["back_band"])
    cols, base, out = [c.channel[steps]], c.channel.shape[1], {}
    for bit, (name, _) in enumerate(INPUTS):
        chan, gain = c.ref_drives[name]
        on = np.flatnonzero(mode >> bit & 1)
        band = side_band.get(name)
        an = (lambda at: None) if band is None else (lambda at: (circ, horiz, band[at]))
        v = sky.incident(rec[:, on, :], tuple(n[on] for n in normals), name, aniso=an(on))
        if side_shade.get(name) is not None:
            j = np.asarray(side_shade[name])[on]
            sel = np.flatnonzero(j >= 0)
            at = on[sel]
            v[:, sel] = sky.incident(rec[:, at, :], tuple(n[at] for n in normals), name, shade=pick(j[sel]), aniso=an(at))
        chan = chan.copy()
        chan[on] = base + np.arange(len(on))
        base += len(on)
        cols.append(v)
        out[name] = (chan, gain)
    ap_rec = rec[:, gains["ap_surface"], :]
    ap = (gains["ap_normal"], gains["ap_tau_coef"], gains["ap_tau_diffuse"], gains["ap_scale"])
    ab = c.bands["aperture_band"]
    pb, pd = solar_gains.transmitted(ap_rec, *ap, aniso=(circ, horiz, ab))
    j = np.asarray(shades["aperture_shade"])
    sel = np.flatnonzero(j >= 0)
    one = (tuple(n[sel] for n in ap[0]), ap[1][sel], ap[2][sel], ap[3][sel])
    pb[:, sel], pd[:, sel] = solar_gains.transmitted(ap_rec[:, sel, :], *one, shade=pick(j[sel]), aniso=(circ, horiz, ab[sel]))
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


def loop(c, state, march, probes, carry=None, steps=None, ap_sum=None):
    """blinds_cases.loop with the anisotropic rule (c.I is the anisotropic irradiance). Returns what it returns."""
    md, blinds = c.md, c.blinds
    NB = len(blinds["shade"])
    steps = range(c.n_steps) if steps is None else steps
    carry = {k: v.copy() for k, v in (bc.fresh(NB) if carry is None else carry).items()}
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


def positions_without_a_zone(c, I):
    """The positions [n_steps, n_blinds] the blinds take under the irradiance I with every zone at NaN: those of the blinds
    that no zone gates (kinds 0-3) are what any march gives — they do not depend on a temperature."""
    state = np.zeros(len(c.blinds["shade"]), np.uint8)
    T = np.full(int(c.md["n_zones"]), np.nan)
    return np.stack([bl.apply(I[k], T, c.channel[k], c.blinds, state, c.f[k], c.shades)[0] for k in range(c.n_steps)])


def coverage(c, ref=None):
    """What the case takes of the rule, as a dict of counts over (step, consumer) pairs; with a loop's result `ref`, the blinds
    no zone gates must have moved as the case says."""
    rec, mode, normals, shades = c.args["record"][:, 0, :], c.args["mode"], c.args["normals"], c.shades
    sz = rec[:, sky.SUN_Z]
    cos = lambda n: (n[0][None, :] * rec[:, None, 0] + n[1][None, :] * rec[:, None, 1]) + n[2][None, :] * rec[:, None, 2]
    f_on, b_on = np.flatnonzero(mode & 1), np.flatnonzero(mode & 2)
    planes = [cos(tuple(n[f_on] for n in normals)), cos(tuple(-n[b_on] for n in normals)), cos(c.gains["ap_normal"]), cos(shades["normal"])]
    c_all = np.concatenate(planes, axis=1)
    front, back, ap = shades["front_shade"], shades["back_shade"], shades["aperture_shade"]
    free = c.kind == 2                                                       # controlled, no zone, no enable channel: I alone decides
    p_iso, p_an = positions_without_a_zone(c, c.I_iso), positions_without_a_zone(c, c.I)
    if ref is not None:
        assert np.array_equal(ref["position"][:, c.kind < 4], p_an[:, c.kind < 4], equal_nan=True)
    return dict(sun_high=int((sz > sky.Z0).sum()), sun_grazing=int(((sz > 0.0) & (sz <= sky.Z0)).sum()),
                below_horizon_facing=int(((sz <= 0.0)[:, None] & (c_all > 0.0)).sum()), behind=int((c_all <= 0.0).sum()),
                circumsolar=int(((sz > 0.0)[:, None] & (c_all > 0.0) & (c.coef[:, 0, :1] > 0.0)).sum()),
                zero_steps=int((~c.coef[:, 0, :].any(axis=1)).sum()), hay_davies_steps=int(((c.coef[:, 0, 0] > 0) & (c.coef[:, 0, 1] == 0)).sum()),
                front_shaded=int((front[f_on] >= 0).sum()), front_unshaded=int((front[f_on] < 0).sum()),
                back_shaded=int((back[b_on] >= 0).sum()), back_unshaded=int((back[b_on] < 0).sum()),
                apertures_shaded=int((ap >= 0).sum()), apertures_unshaded=int((ap < 0).sum()),
                zero_bands=int(sum((c.bands[k] == 0.0).sum() for k in BANDS)),
                decisions_moved=int((p_iso[:, free] != p_an[:, free]).sum()), blinds_moved=int((p_iso[:, free] != p_an[:, free]).any(axis=0).sum()))


def covered(cov):
    """Every item the issue lists appears in the case."""
    return all(cov[k] > 0 for k in ("sun_high", "sun_grazing", "below_horizon_facing", "behind", "circumsolar", "zero_steps", "front_shaded",
                                    "front_unshaded", "back_shaded", "back_unshaded", "apertures_shaded", "apertures_unshaded", "zero_bands",
                                    "decisions_moved", "blinds_moved"))


def namespace_copy(c, **changes):
    return SimpleNamespace(**dict(vars(c), **changes))
