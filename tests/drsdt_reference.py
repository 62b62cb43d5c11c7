"""DRSDT / DRVDT restated from the rule written in include/opmgpu.h at opmgpu_set_dissolution_limits -- NOT from the device code.

The capped cell.  cell() is cell_reference.cell() with two more inputs, the cell's caps: the same 50-digit arithmetic, the same frozen
branches and central differences (cell_reference's own helpers and its branch record), and on top of them the rule's three sentences:
    capped_s = rs_cap < RsSat (after the VAPPARS factor; strict), and then the effective saturated ratio is the constant rs_cap;
    rs is the primary variable in an OIL_ONLY cell, else the effective saturated ratio;
    the oil PVT is saturated iff !has_disgas || (free gas && !capped_s), else the 2-D table at (rs, p);
and the same for Rv with rv_cap, RvSat, free oil and the table at (p_g, rv).  capped_s / capped_v are discrete choices of the base point
like every other branch: decided once there, in float64 from the 50-digit RsSat / RvSat rounded once (a tie is a float64 notion), and frozen.
With both caps +inf every line below is cell_reference's: test_drsdt_reference.py holds the two to exact equality.

The caps of a time step: caps().  The state update: update_state(), BlackoilModelBase::updateState as include/opmgpu.h and the comments
of csrc/blackoil.hip describe it (pressure and saturation chopping, the rs / rv chopping, the phase switching against the saturated
ratios at the old and at the new pressure), in NumPy float64 over all cells at once, for a context WITHOUT end-point scaling, with the
rule's two changes: each of the four saturated ratios becomes min(itself, the cell's cap), and a cell that the switching decision
(taken with the unlimited value) leaves OIL_ONLY / GAS_ONLY takes min(new rs, rs_cap) / min(new rv, rv_cap); with_margins: the smallest relative distance
of a cell's comparisons against a saturated ratio from a tie.
"""
import numpy as np

import cell_reference as R
from cell_reference import GAS_AND_OIL, GAS_ONLY, OIL_ONLY, mpf

INF = float("inf")


def _sat_ratios(tab, F, br, p, pg, so, so_max):
    """(RsSat, RvSat) after the VAPPARS factor at 50 digits, branches frozen (the lines of cell_reference.evaluate)"""
    O, G = F.O, F.G

    def vapf(k, vap):
        active, floor = br["vap"][k]
        if not active:
            return mpf(1)
        so_i = so + (mpf(R.SO_FLOOR) - mpf(br["so"])) if floor else so
        return (so_i / mpf(float(so_max))) ** mpf(float(vap))
    rs_sat = R._lin(O["psat"], O["rs"], br["psat"].seg, p) * vapf(1, tab.vap2) if tab.has_disgas else mpf(0)
    rv_sat = R._lin(G["pg"], G["rv"], br["pg"].seg, pg) * vapf(0, tab.vap1) if tab.has_vapoil else mpf(0)
    return rs_sat, rv_sat


def branches(tab, preg, sreg, p, sw, sg, rs, rv, hc, so_max, rs_cap, rv_cap):
    """cell_reference's branch record plus capped_s / capped_v and, for a capped cell, the searches of the 2-D table it now evaluates"""
    br = R.branches(tab, preg, sreg, p, sw, sg, rs, rv, hc, so_max)
    F = R._Frozen.of(tab, preg, sreg)
    T = R.Tables(tab)
    O, G = T.oil(preg), T.gas(preg)
    pm = mpf(float(p))
    sgm = mpf(br["sg"])
    pg = pm + R._satc(F.S["sg"], F.S["pcgo"], br["sgof"], sgm)
    rs_sat, rv_sat = _sat_ratios(tab, F, br, pm, pg, mpf(br["so"]), so_max)
    # (compared in float64, where a tie exists: the 50-digit ratio rounded once)
    br["capped_s"] = bool(float(rs_cap) < float(rs_sat))
    br["capped_v"] = bool(float(rv_cap) < float(rv_sat))
    free_gas, free_oil = hc != OIL_ONLY, hc != GAS_ONLY
    if tab.has_disgas and free_gas and br["capped_s"]:
        br["oil"] = "under"
        n = br["rs_node"] = R.pvt_search(O["rs"], float(rs_cap))
        br["oil_col"] = (R.pvt_search(O["col_y"][n.seg], float(p)), R.pvt_search(O["col_y"][n.seg + 1], float(p)))
    if tab.has_vapoil and free_oil and br["capped_v"]:
        br["gas"] = "under"
        n = br["pg"]
        br["gas_col"] = (R.pvt_search(G["col_y"][n.seg], float(rv_cap)), R.pvt_search(G["col_y"][n.seg + 1], float(rv_cap)))
    return br


def evaluate(tab, preg, sreg, br, p, sw, x, so_max, rs_cap, rv_cap):
    """cell_reference.evaluate with the caps: the 26 properties (cell_reference.NAMES) at (p, sw, x), the choices of `br` frozen;
    rsSat / rvSat are the EFFECTIVE saturated ratios"""
    F = R._Frozen.of(tab, preg, sreg)
    S, O, G = F.S, F.O, F.G
    hc = br["hc"]
    sg = x if hc == GAS_AND_OIL else ((1 - sw) if hc == GAS_ONLY else mpf(0))
    so = 1 - sw - sg
    pw = p - R._satc(S["sw"], S["pcow"], br["swof"], sw)
    pg = p + R._satc(S["sg"], S["pcgo"], br["sgof"], sg)
    krw = R._satc(S["sw"], S["krw"], br["swof"], sw)
    krg = R._satc(S["sg"], S["krg"], br["sgof"], sg)
    swco = S["sw"][0]
    swp = sw if br["above_swco"] else swco
    swow = mpf(br["swow"]) + (sg - mpf(br["sg"])) + (swp - (mpf(br["sw"]) if br["above_swco"] else swco))
    d = mpf(br["d"]) + (swow - mpf(br["swow"]))
    kow = R._satc(S["sw"], S["krow"], br["krow"], swow)
    kgo = R._satc(S["sg"], S["krog"], br["krog"], d)
    eps = mpf(R.EPS_BLEND)
    if br["blend"] == "k2":
        kro = (kow + kgo) / 2
    else:
        k1 = (sg * kgo + (swp - swco) * kow) / d
        if br["blend"] == "full":
            kro = k1
        else:
            al = (eps - d) / (eps / 2)
            kro = (kow + kgo) / 2 * al + k1 * (1 - al)
    rs_sat, rv_sat = _sat_ratios(tab, F, br, p, pg, so, so_max)
    # THE RULE: a capped saturated ratio is the constant cap
    if br["capped_s"]:
        rs_sat = mpf(float(rs_cap))
    if br["capped_v"]:
        rv_sat = mpf(float(rv_cap))
    rs = x if (tab.has_disgas and hc == OIL_ONLY) else rs_sat
    rv = x if (tab.has_vapoil and hc == GAS_ONLY) else rv_sat
    w = F.w
    X = w[2] * (pw - w[0])
    bw = (1 + X * (1 + X / 2)) / w[1]
    Y = (w[2] - w[4]) * (pw - w[0])
    muw = w[3] * w[1] * bw / (1 + Y * (1 + Y / 2))
    if br["oil"] == "sat":
        i = br["psat"].seg
        bo, bmo = R._lin(O["psat"], O["ib"], i, p), R._lin(O["psat"], O["ibm"], i, p)
    else:
        i, (c0, c1) = br["rs_node"].seg, br["oil_col"]
        bo = R._lin2(O["rs"], i, O["col_y"], O["col_ib"], c0.seg, c1.seg, rs, p)
        bmo = R._lin2(O["rs"], i, O["col_y"], O["col_ibm"], c0.seg, c1.seg, rs, p)
    i = br["pg"].seg
    if br["gas"] == "sat":
        bg, bmg = R._lin(G["pg"], G["ib"], i, pg), R._lin(G["pg"], G["ibm"], i, pg)
    else:
        c0, c1 = br["gas_col"]
        bg = R._lin2(G["pg"], i, G["col_y"], G["col_ib"], c0.seg, c1.seg, pg, rv)
        bmg = R._lin2(G["pg"], i, G["col_y"], G["col_ibm"], c0.seg, c1.seg, pg, rv)
    muo, mug = bo / bmo, bg / bmg
    rhos = F.rhos
    rho = (rhos[0] * bw, rhos[1] * bo + rhos[2] * rs * bo, rhos[2] * bg + rhos[1] * rv * bg)
    pvm, trm = mpf(1), mpf(1)
    if br["rocktab"] is not None:
        k = br["rocktab"].seg
        pvm, trm = R._lin(F.rt[0], F.rt[1], k, p), R._lin(F.rt[0], F.rt[2], k, p)
    elif tab.rock_comp != 0.0:
        cp = mpf(float(tab.rock_comp)) * (p - mpf(float(tab.rock_pref)))
        pvm = 1 + cp + cp * cp / 2
    mob = (trm * krw / muw, trm * kro / muo, trm * krg / mug)
    aw, ao, ag = pvm * bw * sw, pvm * bo * so, pvm * bg * sg
    return [pw, p, pg, bw, bo, bg, muw, muo, mug, krw, kro, krg, rho[0], rho[1], rho[2], mob[0], mob[1], mob[2], rs, rv,
            aw, ao + rv * ag, ag + rs * ao, rs_sat, rv_sat, pvm]


def cell(tab, preg, sreg, p, sw, sg, rs, rv, hc, so_max=0.0, rs_cap=INF, rv_cap=INF):
    """(out[26][4] float64: value, d/dp, d/dSw, d/dX of cell_reference.NAMES; the branch record) of a cell with caps"""
    with R._digits():
        step = mpf(10) ** -25
        br = branches(tab, preg, sreg, p, sw, sg, rs, rv, hc, so_max, rs_cap, rv_cap)
        xv = rs if hc == OIL_ONLY else (rv if hc == GAS_ONLY else sg)
        base = [mpf(float(p)), mpf(float(sw)), mpf(float(xv))]
        out = np.zeros((len(R.NAMES), 4))
        out[:, 0] = [float(v) for v in evaluate(tab, preg, sreg, br, base[0], base[1], base[2], so_max, rs_cap, rv_cap)]
        for k in range(3):
            h = step * max(abs(base[k]), mpf("1e-3"))
            up, dn = list(base), list(base)
            up[k] += h; dn[k] -= h
            fu = evaluate(tab, preg, sreg, br, up[0], up[1], up[2], so_max, rs_cap, rv_cap)
            fd = evaluate(tab, preg, sreg, br, dn[0], dn[1], dn[2], so_max, rs_cap, rv_cap)
            out[:, 1 + k] = [float((a - b) / (2 * h)) for a, b in zip(fu, fd)]
        return out, br


def cells(tab, pvtnum, satnum, st, so_max, rs_cap, rv_cap):
    """every cell of a decks.State with its caps: (out[nc][26][4], list of branch records)"""
    n = st.p.size
    out, recs = np.zeros((n, len(R.NAMES), 4)), []
    for c in range(n):
        o, br = cell(tab, int(pvtnum[c]), int(satnum[c]), st.p[c], st.sat[c, 0], st.sat[c, 2], st.rs[c], st.rv[c], int(st.hc[c]),
                     0.0 if so_max is None else so_max[c], float(rs_cap[c]), float(rv_cap[c]))
        out[c] = o
        recs.append(br)
    return out, recs


# ---- the caps of a time step -----------------------------------------------------------------------------------------------------
def caps(st, dt, drsdt=None, free_only=False, drvdt=None):
    """(rs_cap, rv_cap) at the begin of a time step of length dt from the state st: d = rate * dt once, then ONE addition per cell;
    +inf where the rate is off (None) and, with free_only, where the cell holds no free gas (sg == 0)"""
    n = st.p.size
    rs_cap, rv_cap = np.full(n, INF), np.full(n, INF)
    if drsdt is not None:
        d_s = np.float64(drsdt) * np.float64(dt)
        rs_cap = st.rs + d_s
        if free_only:
            rs_cap = np.where(st.sat[:, 2] == 0.0, INF, rs_cap)
    if drvdt is not None:
        rv_cap = st.rv + np.float64(drvdt) * np.float64(dt)
    return rs_cap, rv_cap


# ---- updateState in NumPy float64 ---------------------------------------------------------------------------------------------
def _pvt_lin(x, y, v):
    """piecewise-linear table with linear extrapolation, one table, v an array: the segment rule of the PVT tables (cell_reference)"""
    x, y = np.asarray(x, float), np.asarray(y, float)
    n = x.size
    i = np.zeros(v.shape, int)
    if n > 2:
        i = (x[1] < v).astype(int)
        for k in range(2, n - 1):
            i = i + (x[k] <= v)
    slope = (y[i + 1] - y[i]) / (x[i + 1] - x[i])
    return y[i] + slope * (v - x[i])


def _sat_right(x, y, v):
    """SGOF curve by a gas saturation: the RIGHT segment at a node, constant at and beyond the end nodes"""
    x, y = np.asarray(x, float), np.asarray(y, float)
    n = x.size
    i = np.zeros(v.shape, int)
    for k in range(1, n - 1):
        i = i + (x[k] <= v)
    f = y[i] + (y[i + 1] - y[i]) / (x[i + 1] - x[i]) * (v - x[i])
    return np.where(v <= x[0], y[0], np.where(v >= x[-1], y[-1], f))


def _by_region(fn, reg, *args):
    out = np.zeros(reg.shape)
    for r in np.unique(reg):
        k = reg == r
        out[k] = fn(int(r), *[a[k] for a in args])
    return out


def _vap(vap, so, so_max):
    f = np.ones_like(so)
    if vap > 0.0:
        k = (so_max > 0.01) & (so < so_max)
        f[k] = (np.maximum(so[k], R.SO_FLOOR) / so_max[k]) ** vap
    return f


def update_state(tab, pvtnum, satnum, prm, dx, st, rs_cap=None, rv_cap=None, so_max=None, relax=1.0, with_margins=False):
    """BlackoilModelBase::updateState with the dissolution caps (None = +inf): the new decks.State; with_margins also the smallest
    relative distance from a tie among each cell's comparisons against a saturated ratio"""
    from opmgpu import decks
    T = R.Tables(tab)
    nc = st.p.size
    eps = R.SO_FLOOR                     # sqrt(DBL_EPSILON)
    rs_cap = np.full(nc, INF) if rs_cap is None else np.asarray(rs_cap, float)
    rv_cap = np.full(nc, INF) if rv_cap is None else np.asarray(rv_cap, float)
    so_max = np.zeros(nc) if so_max is None else np.asarray(so_max, float)
    pvtnum, satnum = np.asarray(pvtnum), np.asarray(satnum)
    hc = np.asarray(st.hc)
    isSg, isRs, isRv = hc == GAS_AND_OIL, hc == OIL_ONLY, hc == GAS_ONLY
    dx = np.asarray(dx, float)
    dp, dsw, dxv = relax * dx[:nc], relax * dx[nc:2 * nc], relax * dx[2 * nc:]
    p_old = st.p
    pn = np.maximum(p_old - np.sign(dp) * np.minimum(np.abs(dp), prm.dp_max_rel * np.abs(p_old)), 0.0)
    sw_old, so_old, sg_old = st.sat[:, 0], st.sat[:, 1], st.sat[:, 2]
    dsg = np.where(isSg, dxv, 0.0) - np.where(isRv, dsw, 0.0)
    dso = -dsw - dsg
    max_val = np.maximum(np.abs(dso), np.maximum(np.abs(dsg), np.abs(dsw)))
    with np.errstate(divide="ignore"):
        step = np.minimum(prm.ds_max / max_val, 1.0)
    w, g, o = sw_old - step * dsw, sg_old - step * dsg, so_old - step * dso
    with np.errstate(divide="ignore", invalid="ignore"):          # (the quotients are taken only where their guard holds)
        k = g < 0
        w, o, g = np.where(k, w / (1 - g), w), np.where(k, o / (1 - g), o), np.where(k, 0.0, g)
        k = o < 0
        w, g, o = np.where(k, w / (1 - o), w), np.where(k, g / (1 - o), g), np.where(k, 0.0, o)
        k = w < 0
        o, g, w = np.where(k, o / (1 - w), o), np.where(k, g / (1 - w), g), np.where(k, 0.0, w)
    rs_old, rv_old = st.rs, st.rv
    rsn, rvn = rs_old.copy(), rv_old.copy()
    if tab.has_disgas:
        d = np.where(isRs, dxv, 0.0)
        rsn = np.maximum(rs_old - np.sign(d) * np.minimum(np.abs(d), np.maximum(np.abs(rs_old) * prm.dr_max_rel, 1.0)), 0.0)
    if tab.has_vapoil:
        d = np.where(isRv, dxv, 0.0)
        rvn = np.maximum(rv_old - np.sign(d) * np.minimum(np.abs(d), np.maximum(np.abs(rv_old) * prm.dr_max_rel, 1e-3)), 0.0)
    wat_only = w > (1 - eps)
    hn = np.full(nc, GAS_AND_OIL, np.int8)
    margin = np.full(nc, INF)

    def rel_gap(a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(np.isfinite(a) & np.isfinite(b) & (np.maximum(np.abs(a), np.abs(b)) > 0), np.abs(a - b) / np.maximum(np.abs(a), np.abs(b)), INF)
    if tab.has_disgas:
        rs_curve = lambda r, pv: _pvt_lin(T.oil(r)["psat"], T.oil(r)["rs"], pv)
        sat0 = _vap(tab.vap2, so_old, so_max) * _by_region(rs_curve, pvtnum, p_old)
        sat1 = _vap(tab.vap2, o, so_max) * _by_region(rs_curve, pvtnum, pn)
        sat0, sat1 = np.minimum(sat0, rs_cap), np.minimum(sat1, rs_cap)           # THE RULE
        has_gas = (g > 0) & ~isRs
        vaporized = (rsn > sat1 * (1 + eps)) & isRs & (rs_old > sat0 * (1 - eps))
        margin = np.minimum(margin, np.where(isRs, np.minimum(rel_gap(rsn, sat1 * (1 + eps)), rel_gap(rs_old, sat0 * (1 - eps))), INF))
        sw_ = wat_only | has_gas | vaporized
        rsn = np.where(sw_, sat1, np.minimum(rsn, rs_cap))                        # THE RULE: a cell left OIL_ONLY does not pass its cap
        hn = np.where(sw_, hn, OIL_ONLY).astype(np.int8)
        o, g, rsn = np.where(wat_only, 0.0, o), np.where(wat_only, 0.0, g), np.where(wat_only, 0.0, rsn)
    if tab.has_vapoil:
        pcgo = lambda r, s: _sat_right(T.sat(r)["sg"], T.sat(r)["pcgo"], s)
        pg_old, pg_new = p_old + _by_region(pcgo, satnum, sg_old), pn + _by_region(pcgo, satnum, g)
        rv_curve = lambda r, pv: _pvt_lin(T.gas(r)["pg"], T.gas(r)["rv"], pv)
        sat0 = _vap(tab.vap1, so_old, so_max) * _by_region(rv_curve, pvtnum, pg_old)
        sat1 = _vap(tab.vap1, o, so_max) * _by_region(rv_curve, pvtnum, pg_new)
        sat0, sat1 = np.minimum(sat0, rv_cap), np.minimum(sat1, rv_cap)           # THE RULE
        has_oil = (o > 0) & ~isRv
        condensed = (rvn > sat1 * (1 + eps)) & isRv & (rv_old > sat0 * (1 - eps))
        margin = np.minimum(margin, np.where(isRv, np.minimum(rel_gap(rvn, sat1 * (1 + eps)), rel_gap(rv_old, sat0 * (1 - eps))), INF))
        sw_ = wat_only | has_oil | condensed
        rvn = np.where(sw_, sat1, np.minimum(rvn, rv_cap))                        # THE RULE: a cell left GAS_ONLY does not pass its cap
        hn = np.where(sw_, hn, GAS_ONLY).astype(np.int8)
        o, g, rvn = np.where(wat_only, 0.0, o), np.where(wat_only, 0.0, g), np.where(wat_only, 0.0, rvn)
    new = decks.State(pn, np.stack([w, o, g], 1), rsn if tab.has_disgas else rs_old.copy(), rvn if tab.has_vapoil else rv_old.copy(), hn)
    return (new, margin) if with_margins else new


CAP_SEED = 17            # chosen on the CPU (test_drsdt_reference.py): with it the restatement leaves out at most 1 % of the cells of every case


def update_cases():
    """the grid, the three states and the increments of test_gpu_assembly.py::test_update_state_parity, each with caps at the state's
    rs / rv times U(0.5, 1.5): (tab, grid, prm, st, dx, rs_cap, rv_cap) per state"""
    from opmgpu import capi, decks
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(9, 8, 6)
    prm = capi.default_params()
    rng, crng = np.random.default_rng(4), np.random.default_rng(CAP_SEED)
    nc = grid.nc
    for seed in (1, 2, 3):
        st = decks.random_state(grid, tab, seed=seed)
        dx = np.concatenate([rng.standard_normal(nc) * 30 * decks.BAR, rng.standard_normal(nc) * 0.25,
                             rng.standard_normal(nc) * np.where(st.hc == capi.HC_OIL_ONLY, 30.0, np.where(st.hc == capi.HC_GAS_ONLY, 1e-4, 0.25))])
        dx[rng.random(3 * nc) < 0.1] = 0.0
        yield tab, grid, prm, st, dx, st.rs * crng.uniform(0.5, 1.5, nc), st.rv * crng.uniform(0.5, 1.5, nc)
