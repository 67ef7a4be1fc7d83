"""Air networks of a series on the host (include/heat_amd.h, heat_air_networks): the rule the device applies to every network
behind the openings of every step, in numpy, and conveniences that give link coefficients, join lists and name the air paths
that read the derived channels. No device, no library.

apply() IS the contract's rule, line for line — every sum, product, quotient and root one rounded f64 operation in the header's
order (numpy never fuses a multiply-add, numpy.sqrt is correctly rounded, and an array expression rounds every element as the
scalar one does) — and so the reference of the tests: a host that applies it to the step's channel row behind the controllers'
and the openings' rules and before the other terms', between heat_batch_march_ex calls, gets the bits of
heat_batch_march_series_networks. The reference has no counterpart (model.rs:546,592-593 take the volumes as given numbers).

The networks of one size are solved side by side, [networks, n, n]: the order of the operations within a network is the
header's, and networks do not meet."""
import numpy as np

G = 9.81
NET_KEYS = ("net_offset", "tol", "max_iter", "g_min")
NODE_INT_KEYS = ("node_zone", "src_chan")
NODE_REAL_KEYS = ("src_gain",)
LINK_INT_KEYS = ("zone_a", "zone_b", "temp_chan", "wp_chan", "frac_chan", "out_ab", "out_ba")
LINK_REAL_KEYS = ("c", "gh", "p_lin", "wp_gain")
INT_KEYS = ("net_offset", "max_iter") + NODE_INT_KEYS + LINK_INT_KEYS
KEYS = NET_KEYS + NODE_INT_KEYS + NODE_REAL_KEYS + LINK_INT_KEYS + LINK_REAL_KEYS
STATE = ("pressure",)
ACC = ("sum_ab", "sum_ba", "iters_sum", "unconverged", "max_res")
_NEUTRAL = dict(src_chan=-1, src_gain=1.0, temp_chan=-1, wp_chan=-1, frac_chan=-1, out_ab=-1, out_ba=-1, gh=0.0, wp_gain=1.0)
_DTYPE = dict(pressure=np.float64, sum_ab=np.float64, sum_ba=np.float64, iters_sum=np.int64, unconverged=np.int64, max_res=np.float64)
_OVER = dict(pressure="node", sum_ab="link", sum_ba="link", iters_sum="net", unconverged="net", max_res="net")
MAX_NODES = 64


def n_networks(nw):
    return 0 if not nw or nw.get("net_offset") is None else max(len(np.atleast_1d(nw["net_offset"])) - 1, 0)


def n_nodes(nw):
    return 0 if not nw or nw.get("node_zone") is None else len(np.atleast_1d(nw["node_zone"]))


def n_links(nw):
    return 0 if not nw or nw.get("zone_a") is None else len(np.atleast_1d(nw["zone_a"]))


def counts(nw):
    return dict(net=n_networks(nw), node=n_nodes(nw), link=n_links(nw))


def _given(nw, key, n):
    dtype = np.int64 if key in INT_KEYS else np.float64
    return np.full(n, _NEUTRAL[key], dtype) if nw.get(key) is None else np.asarray(nw[key], dtype=dtype).reshape(-1)


def fresh(nw):
    """The state and the accumulators as resume == 0 leaves them on the device: all zero."""
    n = counts(nw)
    return {k: np.zeros(n[_OVER[k]], _DTYPE[k]) for k in STATE + ACC}


def structure(nw):
    """What apply() needs of a term besides its numbers, formed once: the node of every zone, the links' nodes and network, the
    incidence list (every link at its first node with sign -1 and, between zones, at its second with +1, in ascending link
    number — the order in which a node's balance is summed) and the networks grouped by their size."""
    W, N, L = n_networks(nw), n_nodes(nw), n_links(nw)
    off = np.asarray(nw["net_offset"], dtype=np.int64).reshape(-1) if W else np.zeros(1, np.int64)
    node_zone = _given(nw, "node_zone", N)
    size = np.diff(off)
    node_net = np.repeat(np.arange(W), size)
    node_local = np.arange(N) - off[:-1][node_net]
    node_of_zone = np.full(int(node_zone.max()) + 2 if N else 1, -1, np.int64)
    node_of_zone[node_zone] = np.arange(N)
    za, zb = _given(nw, "zone_a", L), _given(nw, "zone_b", L)
    la = node_of_zone[za]
    lb = np.where(zb >= 0, node_of_zone[np.maximum(zb, 0)], -1)
    inner = np.flatnonzero(lb >= 0)
    # the incidence entries in ascending link number, a link's first node ahead of its second
    e_link = np.concatenate([np.arange(L), inner])
    e_node = np.concatenate([la, lb[inner]])
    e_sign = np.concatenate([-np.ones(L), np.ones(len(inner))])
    order = np.lexsort((e_sign, e_link))
    groups = []
    for n in np.unique(size):
        nets = np.flatnonzero(size == n)
        slot = np.full(W, -1, np.int64)
        slot[nets] = np.arange(len(nets))
        mine = inner[size[node_net[la[inner]]] == n]
        # the off-diagonal entries, A[a][b] and A[b][a] of every link between zones, in ascending link number: three links of the
        # same two zones, whichever way round each is given, are subtracted from an entry in the header's order
        twice = np.repeat(mine, 2)
        rows = np.stack([node_local[la[mine]], node_local[lb[mine]]], axis=1).reshape(-1)
        cols = np.stack([node_local[lb[mine]], node_local[la[mine]]], axis=1).reshape(-1)
        groups.append(dict(n=int(n), nets=nets, nodes=off[:-1][nets][:, None] + np.arange(n)[None, :], link=twice,
                           slot=slot[node_net[la[twice]]], row=rows, col=cols))
    return dict(W=W, N=N, L=L, off=off, node_net=node_net, la=la, lb=lb, link_net=node_net[la], e_link=e_link[order], e_node=e_node[order],
                e_sign=e_sign[order], groups=groups)


def rho(t):
    """The density of dry air at t C as heat_air_paths forms it: the same expression and grouping."""
    tk = t + 273.15
    return 101325. * 28.97 / (8314.46261815324 * tk)


def apply(T, row, nw, state, plan=None):
    """One step of the rule. Returns (row_with_derived_columns, rec): a copy of `row` with every link's flows stored at out_ab and
    out_ba, and rec = dict(link_q [n_links], node_p [n_nodes], net_iters [n_networks] — the step's rows —, ab, ba [n_links],
    res [n_networks], converged [n_networks], fired [n_networks]: whether the acceleration took a w < 1 in some node-iteration,
    root [n_links]: whether the link ended in the root regime). state["pressure"] is updated in place.
    T      the zone AIR temperatures at the start of the step
    row    the step's channel row (not written)
    nw     a dict of arrays (make_air_networks names them)
    state  fresh(nw), or what a series returned
    plan   structure(nw), where the caller keeps it over the steps"""
    T = np.asarray(T, dtype=np.float64)
    new = np.array(row, dtype=np.float64)
    row = np.asarray(row, dtype=np.float64)
    p = plan if plan is not None else structure(nw)
    W, N, L = p["W"], p["N"], p["L"]
    if W == 0:
        return new, dict(link_q=np.zeros(0), node_p=np.zeros(0), net_iters=np.zeros(0, np.int32), ab=np.zeros(0), ba=np.zeros(0), res=np.zeros(0),
                         converged=np.zeros(0, bool), fired=np.zeros(0, bool), root=np.zeros(0, bool))
    g = {k: _given(nw, k, L) for k in LINK_INT_KEYS + LINK_REAL_KEYS}
    tol, max_iter, g_min = _given(nw, "tol", W), _given(nw, "max_iter", W), _given(nw, "g_min", W)
    src_chan, src_gain, node_zone = _given(nw, "src_chan", N), _given(nw, "src_gain", N), _given(nw, "node_zone", N)
    la, lb, za, zb = p["la"], p["lb"], g["zone_a"], g["zone_b"]
    at = lambda chan: row[np.maximum(chan, 0)] if len(row) else np.full(len(chan), np.nan)
    P = state["pressure"]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s_lin = np.sqrt(g["p_lin"])
        f = np.where(g["frac_chan"] >= 0, at(g["frac_chan"]), 1.0)
        f = np.where(f < 0.0, 0.0, f)
        f = np.where(f > 1.0, 1.0, f)
        C = g["c"] * f
        ra = rho(T[za])
        rb = np.where(zb >= 0, rho(T[np.maximum(zb, 0)]), rho(at(g["temp_chan"])))
        p_out = np.where(g["wp_chan"] >= 0, g["wp_gain"] * at(g["wp_chan"]), 0.0)
        dr = ra - rb
        sh = g["gh"] * dr
        src = np.where(src_chan >= 0, src_gain * at(src_chan), 0.0)
        dold = np.zeros(N)
        active = np.ones(W, bool)
        converged, fired = np.zeros(W, bool), np.zeros(W, bool)
        iters, res = np.zeros(W, np.int32), np.zeros(W)
        q_end, fwd_end, root_end = np.zeros(L), np.zeros(L, bool), np.zeros(L, bool)
        for it in range(MAX_NODES + 1):
            # ---- assemble ----
            pb = np.where(lb >= 0, P[np.maximum(lb, 0)], p_out)
            d0 = P[la] - pb
            dp = d0 - sh
            ad = np.abs(dp)
            root = ad >= g["p_lin"]
            s = np.sqrt(ad)
            q_root = C * s
            hq = 0.5 * q_root
            ca = C * ad
            q = np.where(root, q_root, ca / s_lin)
            gq = np.where(root, hq / ad, C / s_lin)
            fwd = dp >= 0.0
            ru = np.where(fwd, ra, rb)
            m = ru * q
            gm = ru * gq
            ms = np.where(fwd, m, -m)
            F = src.copy()
            np.add.at(F, p["e_node"], p["e_sign"] * ms[p["e_link"]])      # F[a] - ms and F[b] + ms, a node's links ascending
            diag = g_min[p["node_net"]].copy()
            np.add.at(diag, p["e_node"], gm[p["e_link"]])
            af = np.abs(F)
            res_now = np.maximum.reduceat(np.where(af > 0.0, af, 0.0), p["off"][:-1])
            mine = active[p["link_net"]]
            q_end[mine], fwd_end[mine], root_end[mine] = q[mine], fwd[mine], root[mine]
            res[active] = res_now[active]
            spent = active & (it >= max_iter)
            done = active & ~spent & (res <= tol)
            iters[spent | done] = it
            converged[done] = True
            active &= ~(spent | done)
            if not active.any():
                break
            # ---- eliminate, back-substitute, accelerate: the networks of one size side by side ----
            for grp in p["groups"]:
                sel = active[grp["nets"]]
                if not sel.any():
                    continue
                n, nodes = grp["n"], grp["nodes"][sel]
                A = np.zeros((len(grp["nets"]), n, n))
                i = np.arange(n)
                A[:, i, i] = diag[grp["nodes"]]
                np.subtract.at(A, (grp["slot"], grp["row"], grp["col"]), gm[grp["link"]])
                A = A[sel]
                Fg = F[nodes]
                for kk in range(n - 1):
                    fac = A[:, kk + 1:, kk] / A[:, kk, kk][:, None]
                    t = fac[:, :, None] * A[:, kk, kk + 1:][:, None, :]
                    A[:, kk + 1:, kk + 1:] -= t
                    t = fac * Fg[:, kk][:, None]
                    Fg[:, kk + 1:] -= t
                d = np.zeros_like(Fg)
                for j in range(n - 1, -1, -1):
                    d[:, j] = Fg[:, j] / A[:, j, j]
                    t = A[:, :j, j] * d[:, j][:, None]
                    Fg[:, :j] -= t
                do = dold[nodes]
                r = d / do
                relax = (do != 0.0) & (r < -0.5)
                o = 1.0 - r
                w = np.where(relax, 1.0 / o, 1.0)
                dn = w * d
                P[nodes] = P[nodes] + dn
                dold[nodes] = dn
                fired[grp["nets"][sel]] |= relax.any(axis=1)
    ab, ba = np.where(fwd_end, q_end, 0.0), np.where(fwd_end, 0.0, q_end)
    oab, oba = g["out_ab"], g["out_ba"]
    new[oab[oab >= 0]] = ab[oab >= 0]
    new[oba[oba >= 0]] = ba[oba >= 0]
    return new, dict(link_q=np.where(fwd_end, q_end, -q_end), node_p=P.copy(), net_iters=iters, ab=ab, ba=ba, res=res, converged=converged,
                     fired=fired, root=root_end)


def accumulate(rec, acc):
    """The accumulators of one step, in place, from the rec apply() returned."""
    with np.errstate(invalid="ignore"):
        if "sum_ab" in acc:
            acc["sum_ab"][:] = acc["sum_ab"] + rec["ab"]
        if "sum_ba" in acc:
            acc["sum_ba"][:] = acc["sum_ba"] + rec["ba"]
        if "iters_sum" in acc:
            acc["iters_sum"][:] = acc["iters_sum"] + rec["net_iters"]
        if "unconverged" in acc:
            acc["unconverged"][~rec["converged"]] += 1
        if "max_res" in acc:
            higher = rec["res"] > acc["max_res"]
            acc["max_res"][higher] = rec["res"][higher]


def mass_in(T, row, nw, rec, plan=None):
    """The signed mass flow into every node, kg/s, of the flows apply() returned with their step's T and row: the links' ru q
    and the nodes' sources. At a converged step its magnitude is at most tol."""
    p = plan if plan is not None else structure(nw)
    L, N = p["L"], p["N"]
    g = {k: _given(nw, k, L) for k in ("zone_a", "zone_b", "temp_chan")}
    row = np.asarray(row, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    ra = rho(T[g["zone_a"]])
    rb = np.where(g["zone_b"] >= 0, rho(T[np.maximum(g["zone_b"], 0)]), rho(row[np.maximum(g["temp_chan"], 0)]))
    ms = ra * rec["ab"] - rb * rec["ba"]
    src_chan, src_gain = _given(nw, "src_chan", N), _given(nw, "src_gain", N)
    F = np.where(src_chan >= 0, src_gain * row[np.maximum(src_chan, 0)], 0.0)
    np.add.at(F, p["e_node"], p["e_sign"] * ms[p["e_link"]])
    return F


def concat(*parts):
    """Joins network dicts (as apply() takes them) into one: the networks, their nodes and their links behind one another, a
    list that a part leaves out filled with its neutral value (a channel -1, a gain 1, gh 0)."""
    parts = [q for q in parts if n_networks(q)]
    out = {}
    base = np.cumsum([0] + [n_nodes(q) for q in parts])
    offs = [np.asarray(q["net_offset"], dtype=np.int64).reshape(-1)[(1 if j else 0):] + base[j] for j, q in enumerate(parts)]
    out["net_offset"] = (np.concatenate(offs) if offs else np.zeros(1)).astype(np.int32)
    for key in KEYS[1:]:
        if key not in _NEUTRAL and all(q.get(key) is None for q in parts):
            continue
        n_of = n_networks if key in NET_KEYS else n_nodes if key in NODE_INT_KEYS + NODE_REAL_KEYS else n_links
        dtype = np.int32 if key in INT_KEYS else np.float64
        cols = [np.full(n_of(q), _NEUTRAL[key], dtype) if q.get(key) is None else np.asarray(q[key], dtype=dtype).reshape(-1) for q in parts]
        out[key] = np.concatenate(cols) if cols else np.zeros(0, dtype)
    return out


def orifice(area, cd):
    """The flow coefficient of a sharp-edged orifice, q = cd A sqrt(2 dp / rho) at the standard density 1.2 kg/m3: c = cd A
    sqrt(2 / 1.2), m3/s per sqrt(Pa). area: m2; cd: the discharge coefficient (0.6 - 0.65). The rule carries the step's own
    densities in the mass flow; the volume law takes the standard one, as the crack and opening data of the multizone tools do."""
    area, cd = np.asarray(area, dtype=np.float64), np.asarray(cd, dtype=np.float64)
    return cd * area * np.sqrt(2.0 / 1.2)


def tall_opening(width, height, cd, sill=0.0):
    """A tall doorway or window as TWO links, at a quarter and at three quarters of its height, each with half of its area:
    with a temperature difference the lower carries air one way and the upper the other, and the two-way flow falls out of the
    network's balance. width, height: m; cd: the discharge coefficient; sill: the height of its lower edge above the network's
    datum, m. Returns dict(c, gh) with arrays of shape [2, ...]: the lower link first."""
    width, height, cd, sill = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (width, height, cd, sill)))
    c = orifice(width * height / 2.0, cd)
    return dict(c=np.stack([c, c]), gh=np.stack([G * (sill + 0.25 * height), G * (sill + 0.75 * height)]))


def paths(nw):
    """The air paths (heat_air_paths; air_paths.concat joins them to others) that read every derived channel of the networks:
    for a link between zones a -> b with volume out_ab and b -> a with volume out_ba, for a link to outside one supply path
    into its zone (source -1, the link's temp_chan) with volume out_ba, and where it names one an exhaust-side path is none:
    what leaves a zone enters no balance. The path's m = rho(Ts) V is the network's ru q. Returns the dict and, as its key
    "link", the link of every path."""
    L = n_links(nw)
    g = {k: _given(nw, k, L) for k in LINK_INT_KEYS}
    za, zb, oab, oba = g["zone_a"], g["zone_b"], g["out_ab"], g["out_ba"]
    fw = np.flatnonzero((zb >= 0) & (oab >= 0))
    bw = np.flatnonzero((zb >= 0) & (oba >= 0))
    su = np.flatnonzero((zb < 0) & (oba >= 0))
    i32 = lambda *cols: np.concatenate(cols).astype(np.int32)
    return dict(target=i32(zb[fw], za[bw], za[su]), source=i32(za[fw], zb[bw], np.full(len(su), -1)),
                temp_chan=i32(np.full(len(fw) + len(bw), -1), g["temp_chan"][su]), volume_chan=i32(oab[fw], oba[bw], oba[su]),
                link=np.concatenate([fw, bw, su]))
