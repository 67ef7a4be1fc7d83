"""The cases of the shade tests (include/heat_amd.h, heat_shades), shared by tests/test_shades_host.py — which builds them on the
CPU alone and so runs the assertions below — and tests/test_shades_gpu.py.

A case starts from test_solar_gains_gpu.gains_case (itself test_sky_gpu.sky_case plus windows): channels, sky-driven inputs,
apertures and receivers. Then the suns of the records are laid out BY PATTERN, shades are added by pattern, and the pattern
is asserted with heat_amd.shading.sunlit — the rule in numpy. The expected inputs of the reference loops are one channel
column per sky-driven input and per receiver, filled by sky.incident(..., shade=) and solar_gains.received of the shaded
solar_gains.transmitted(..., shade=) (`reference`): those loops run unchanged. No device is needed to build a case."""
import numpy as np

from heat_amd import shading, sky, solar_gains
from test_series_gpu import INPUTS
from test_sky_gpu import call_kwargs
from test_solar_gains_gpu import EN, SOLAR, gains_case

N_SUNS = 24            # the length of the sun pattern: a case has at least as many steps
N_SHADES = 150         # not a multiple of 64: the last wavefront of k_series_shading is ragged
N_HORIZONS = 3
GEOMETRY = ("width", "height") + shading.GEOMETRY
SOUTH = 0              # shade 0: a south window with an overhang and both fins, no horizon — the exact cases are asserted on it
SHARED = 1             # shade 1 serves two surface sides and an aperture


def sun_pattern(rng):
    """[N_SUNS, 3] sun vectors and the slot of the NaN. Slots 0-15: one sun inside every 22.5 degree sector, at five kinds of
    elevation (grazing, low, middle, high, below the horizon); 16-21 exactly on sector boundaries — |sx| == |sy| in all four
    quadrants, sy == 0 (which is c == 0 exactly on a south-facing plane) and sx == 0 (us == 0 exactly on it); 22: sy == 0 with
    the sun in the west; 23: a NaN component."""
    sun = np.zeros((N_SUNS, 3))
    sz = np.array([0.05, 0.3, 0.7, 0.95, -0.3])
    for q in range(16):
        z = sz[q % 5] * rng.uniform(0.9, 1.0)
        az = np.radians(22.5 * (q + rng.uniform(0.2, 0.8)))
        h = np.sqrt(1.0 - z * z)
        sun[q] = (h * np.cos(az), h * np.sin(az), z)
    sun[16:20] = [(0.5, 0.5, 0.7), (-0.5, 0.5, 0.7), (-0.5, -0.5, 0.7), (0.5, -0.5, 0.7)]
    sun[20] = (0.6, 0.0, 0.8)
    sun[21] = (0.0, -0.6, 0.8)
    sun[22] = (-0.8, 0.0, 0.6)
    sun[23] = (np.nan, -0.6, 0.8)
    return sun, 23


def shades_case(md, rng, n_steps, channel=None, drives=None):
    """Returns (channel, drives of the call, drives of the reference, sky arguments, gains arguments, shades arguments — a dict
    of binding.make_shades' arguments)."""
    assert n_steps >= N_SUNS, "the sun pattern needs %d steps" % N_SUNS
    S = int(md["n_surfaces"])
    channel, call, ref, args, gains = gains_case(md, rng, n_steps, channel, drives)
    sun, nan_slot = sun_pattern(rng)
    shift = int(rng.integers(0, N_SUNS))                                   # (a case of its own per site: a wrong record shows)
    slot = (np.arange(n_steps) + shift) % N_SUNS
    args["record"][:, 0, :3] = sun[slot]
    NS, NH, NA = N_SHADES, N_HORIZONS, len(gains["ap_surface"])
    j = np.arange(NS)
    # planes: exactly south-facing walls, walls of any azimuth, planes tilted towards the sky
    az = rng.uniform(0.0, 2 * np.pi, NS)
    south = j % 15 == 0
    nz = np.where((j % 3 != 1) & ~south, 0.8, 0.0)
    nh = np.sqrt(1.0 - nz * nz)
    normal = (np.where(south, 0.0, nh * np.cos(az)), np.where(south, -1.0, nh * np.sin(az)), nz)
    right, up = shading.frame_of(normal)
    geometry = dict(width=rng.uniform(0.8, 3.0, NS), height=rng.uniform(1.0, 2.5, NS),
                    overhang_depth=np.where(j % 5 == 4, 0.0, rng.uniform(0.3, 1.2, NS)), overhang_gap=rng.uniform(0.0, 0.4, NS),
                    fin_pos_depth=np.where(j % 4 == 3, 0.0, rng.uniform(0.2, 1.0, NS)), fin_pos_gap=rng.uniform(0.0, 0.2, NS),
                    fin_neg_depth=np.where(j % 4 == 2, 0.0, rng.uniform(0.2, 1.0, NS)), fin_neg_gap=rng.uniform(0.0, 0.2, NS))
    for key, v in dict(width=1.2, height=1.5, overhang_depth=0.6, overhang_gap=0.2, fin_pos_depth=0.4, fin_pos_gap=0.05,
                       fin_neg_depth=0.3, fin_neg_gap=0.05).items():
        geometry[key][SOUTH] = v
    horizon = np.where(j % 2 == 0, j % NH, -1).astype(np.int32)
    horizon[SOUTH] = -1
    elevations = rng.uniform(0.0, 25.0, (NH, 16))
    elevations[1, ::2] = 0.0                                               # a flat horizon in every other sector: tan2 == 0
    front = np.full(S, -1, np.int32)
    back = np.full(S, -1, np.int32)
    mode = args["mode"]
    f_on, b_on = np.flatnonzero(mode & 1), np.flatnonzero(mode & 2)
    front[f_on] = np.where(np.arange(len(f_on)) % 3 == 2, -1, f_on % NS)
    back[b_on] = np.where(np.arange(len(b_on)) % 2 == 1, -1, (3 * b_on + 1) % NS)
    both = np.flatnonzero((mode & 3) == 3)
    assert len(both) >= 2 and len(f_on) >= 3 and len(b_on) >= 3
    front[both[0]], back[both[0]] = 5, -1                                  # one side shaded, the other not
    front[f_on[0] if f_on[0] != both[0] else f_on[1]] = SHARED
    back[b_on[-1] if b_on[-1] != both[0] else b_on[-2]] = SHARED
    aperture = np.where(np.arange(NA) % 3 == 2, -1, (7 * np.arange(NA)) % NS).astype(np.int32)
    aperture[1] = SHARED
    shades = dict(surface=rng.integers(0, S, NS), normal=normal, right=right, up=up, diffuse_factor=rng.uniform(0.5, 1.0, NS),
                  ground_factor=rng.uniform(0.3, 1.0, NS), horizon=horizon, horizon_tan2=shading.horizon_tan2(elevations),
                  front_shade=front, back_shade=back, aperture_shade=aperture, **geometry)
    # ---- the pattern, asserted with the rule in numpy ----
    d = sunlit_of(shades, args["record"], details=True)
    f = d["f"]
    partial = (f > 0.0) & (f < 1.0)
    assert partial.mean() >= 0.25, "only %.0f %% of the (step, shade) pairs are partly sunlit" % (100 * partial.mean())
    assert (f == 0.0).any() and (f == 1.0).any() and not np.isnan(f).any()
    s0 = {k: v[:, SOUTH] for k, v in d.items()}
    H, gap = geometry["height"][SOUTH], geometry["overhang_gap"][SOUTH]
    lit0 = s0["c"] > 0.0
    assert (lit0 & (s0["sh"] == H)).any() and (lit0 & (s0["drop"] < gap) & (s0["vs"] > 0.0)).any() and (lit0 & (s0["vs"] <= 0.0)).any()
    assert (lit0 & (s0["us"] > 0.0) & (s0["wp"] > 0.0)).any() and (lit0 & (s0["us"] < 0.0) & (s0["wn"] > 0.0)).any()
    assert (lit0 & (s0["us"] == 0.0)).any() and (s0["c"] == 0.0).any() and np.isnan(s0["c"]).sum() == (slot == nan_slot).sum() > 0
    for key in ("fin_pos_depth", "fin_neg_depth", "overhang_depth"):       # every device acts somewhere, and is absent somewhere
        assert (geometry[key] == 0.0).any() and (geometry[key] > 0.0).any()
    sx, sy = args["record"][:, 0, 0], args["record"][:, 0, 1]
    assert set(d["sector"][:, 0]) == set(range(16))
    assert (sy == 0.0).any() and (sx == 0.0).any() and len(set(d["sector"][np.abs(sx) == np.abs(sy), 0])) == 4
    with_profile = horizon >= 0
    assert with_profile.any() and (~with_profile).any()
    in_front = d["c"][:, with_profile] > 0.0
    assert (d["lit"][:, with_profile] & in_front).any() and (~d["lit"][:, with_profile] & in_front).any()
    assert (front == SHARED).sum() >= 1 and (back == SHARED).sum() >= 1 and aperture[1] == SHARED
    assert (back >= 0).any() and front[both[0]] >= 0 and back[both[0]] < 0 and (mode[both[0]] & 3) == 3
    assert (front[f_on] < 0).any() and (back[b_on] < 0).any() and (aperture < 0).any() and (aperture >= 0).any()
    assert NS % 64 != 0
    return channel, call, ref, args, gains, shades


def sunlit_of(shades, record, site=None, details=False):
    """[n_steps, n_shades]: shading.sunlit of every shade under the sun of ITS surface's site."""
    surface = np.asarray(shades["surface"], dtype=np.int64)
    site = np.zeros(len(surface), np.int64) if site is None else np.asarray(site, dtype=np.int64)[surface]
    return shading.sunlit(record[:, site, :], shades["normal"], shades["right"], shades["up"], horizon=shades.get("horizon"),
                          horizon_tan2=shades.get("horizon_tan2"), details=details, **{k: shades[k] for k in GEOMETRY})


def factors(shades, j, f):
    """(f, fd, fg) of the consumers whose shades are j (all >= 0), for sky.incident / solar_gains.transmitted."""
    n = len(shades["surface"])
    fd = np.ones(n) if shades.get("diffuse_factor") is None else np.asarray(shades["diffuse_factor"], dtype=np.float64)
    fg = np.ones(n) if shades.get("ground_factor") is None else np.asarray(shades["ground_factor"], dtype=np.float64)
    return f[:, j], fd[j], fg[j]


def reference(md, channel, ref_drives, args, gains, shades, site=None):
    """The shaded sky and the shaded gains as channels, for the reference loops (test_sky_gpu.expanded and
    test_solar_gains_gpu.with_gains, with the shades). Returns the widened table and drives, sunlit [n_steps, n_shades],
    transmitted [n_steps, n_apertures] and ap_sum [n_apertures] as the rules give them."""
    S = int(md["n_surfaces"])
    site = np.zeros(S, np.int64) if site is None else np.asarray(site, dtype=np.int64)
    rec, mode, normals = args["record"], args["mode"], args["normals"]
    f = sunlit_of(shades, rec, site)
    side_shade = dict(solar_front=shades.get("front_shade"), solar_back=shades.get("back_shade"))
    cols, base, out = [channel], channel.shape[1], {}
    for bit, (name, _) in enumerate(INPUTS):
        chan, gain = ref_drives[name]
        on = np.flatnonzero(mode >> bit & 1)
        v = sky.incident(rec[:, site[on], :], tuple(n[on] for n in normals), name)            # [n_steps, len(on)]
        if side_shade.get(name) is not None:
            j = np.asarray(side_shade[name])[on]
            sel = np.flatnonzero(j >= 0)
            at = on[sel]
            v[:, sel] = sky.incident(rec[:, site[at], :], tuple(n[at] for n in normals), name, shade=factors(shades, j[sel], f))
        chan = chan.copy()
        chan[on] = base + np.arange(len(on))
        base += len(on)
        cols.append(v)
        out[name] = (chan, gain)
    ap_rec = rec[:, site[gains["ap_surface"]], :]
    ap = (gains["ap_normal"], gains["ap_tau_coef"], gains["ap_tau_diffuse"], gains["ap_scale"])
    pb, pd = solar_gains.transmitted(ap_rec, *ap)
    if shades.get("aperture_shade") is not None:
        j = np.asarray(shades["aperture_shade"])
        sel = np.flatnonzero(j >= 0)
        one = (tuple(n[sel] for n in ap[0]), ap[1][sel], ap[2][sel], ap[3][sel])
        pb[:, sel], pd[:, sel] = solar_gains.transmitted(ap_rec[:, sel, :], *one, shade=factors(shades, j[sel], f))
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
    p = pb + pd
    ap_sum = np.zeros(p.shape[1])
    for k in range(len(p)):
        ap_sum = ap_sum + p[k]
    return np.concatenate(cols, axis=1), out, f, p, ap_sum


def shaded_kwargs(channel, call, probes, a0, b0, args, gains, shades, steps=slice(None), ap_sum=None):
    return dict(call_kwargs(channel, call, probes, a0, b0, steps, args), gains=dict(gains, ap_sum=ap_sum), shades=shades)


def transparent_shades(md, args, gains):
    """Shades that shade nothing: one per sky-driven solar side and per aperture, in the consumer's own plane, with zero depths,
    no horizon and the factors NULL. Such a shade has f == 1 exactly where its consumer's cosine is positive (the same
    expression on the same values), and f only ever multiplies a beam that is 0.0 elsewhere: the bits of the call without
    shades."""
    S = int(md["n_surfaces"])
    mode = args["mode"]
    f_on, b_on = np.flatnonzero(mode & 1), np.flatnonzero(mode & 2)
    NA = len(gains["ap_surface"])
    normal = tuple(np.concatenate([n[f_on], -n[b_on], a]) for n, a in zip(args["normals"], gains["ap_normal"]))
    right, up = shading.frame_of(normal)
    n = len(normal[0])
    front, back = np.full(S, -1, np.int32), np.full(S, -1, np.int32)
    front[f_on] = np.arange(len(f_on))
    back[b_on] = len(f_on) + np.arange(len(b_on))
    return dict(surface=np.concatenate([f_on, b_on, gains["ap_surface"]]), normal=normal, right=right, up=up, width=np.ones(n),
                height=np.ones(n), front_shade=front, back_shade=back, **{key: np.zeros(n) for key in shading.GEOMETRY},
                aperture_shade=(len(f_on) + len(b_on) + np.arange(NA)).astype(np.int32))
