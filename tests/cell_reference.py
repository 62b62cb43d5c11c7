"""One cell of the default three-phase black-oil model (no ENDSCALE, no hysteresis) at 50 digits, restated from the rules written in the
comments of csrc/fluid_eval.hpp, include/opmgpu.h and oracle/oracle.cpp -- NOT from the device code, and value-only: there is no chain rule
here that could share a mistake with the kernel's or the oracle's.

Two steps.  branches() decides every discrete choice at the base point, in float64 and by the stated rules, and returns them as a record:
    table searches  PVT tables (Tabulated1DFunction): linear extrapolation; at a node x[k] the segment is k, except that at x[1] it is 0
                    (segment 0 reaches up to and INCLUDING x[1]) and from x[n-2] on it is n-2.
                    SWOF curves by a water saturation: the LEFT segment at a node (x[i] < s <= x[i+1]); SGOF curves by a gas saturation: the
                    RIGHT one (x[i] <= s < x[i+1]); both constant at and beyond the end nodes (the clamp flag).
                    ROCKTAB: the LEFT segment at a breakpoint, linear extrapolation.
    sw > swco       Sw' = max(Sw, Swco) with derivative 0 at and below Swco (Swco = the first SWOF node)
    blend           d = (Sg + Sw') - Swco against eps = 1e-5:  d >= eps the saturation-weighted kro; d <= eps/2 the plain mean k2;
                    between, k2 * al + k1 * (1 - al) with al = (eps - d) / (eps / 2)
    oil / gas PVT   the saturated curve when the other hydrocarbon phase is free (or without DISGAS / VAPOIL), else the 2-D table
    VAPPARS         the factor (max(so, 1.49e-8) / so_max)^vap applies iff vap > 0, so_max > 0.01 and so < so_max
                    (the factor and its so-derivative are those of (s / so_max)^vap at s = max(so, 1.49e-8): the derivative is NOT zeroed on
                    the floor -- BlackoilPropsAdFromDeck.cpp:1065-1067 --, so the frozen floor is the shift s = so + (1.49e-8 - so_base))
The derived arguments of a search (Sg + Sw', that minus Swco, p_g = p + pcgo) are formed in float64 in the stated order, as every
implementation forms them, so that "on a node" means the same here as there.  For the blend the float64 values of Sg + Sw' and of
d = (Sg + Sw') - Swco are also what evaluate() starts from (plus the exact change of Sg and Sw' from the base point): the law divides by d,
which is ~1e-5 in the blend zone, so the 1.4e-17 rounding of Sg + Sw' next to Swco = 0.1 is worth 1e-12 of kro and 1e-7 of its
derivatives.  That is the conditioning of the stated rule in float64, common to every implementation, and not what this file measures.

evaluate() is then the smooth function of (p, Sw, X) with those choices frozen, at 50 digits (mpmath; the standard library's decimal where that is missing); the derivatives are its central
differences with a relative step of 1e-25 (of max(|x|, 1e-3): a saturation of 0 or 5e-324 still gets a step the 50 digits resolve;
truncation ~1e-50, rounding ~1e-25: exact for a float64 comparison).  At a node the frozen
branch makes the derivative the chosen segment's.  X is the cell's third primary variable: Sg, rs or rv by its hydrocarbon state.
"""
import contextlib
import decimal
from collections import namedtuple

import numpy as np

try:
    import mpmath
except ImportError:          # the standard library's decimal does the same arithmetic at the same digits (test_cell_reference.py compares the two)
    mpmath = None
BACKEND = "mpmath" if mpmath is not None else "decimal"
DPS = 50


def mpf(v):
    """v (a float, exactly; an int; a string) as a number of the backend"""
    return mpmath.mpf(v) if BACKEND == "mpmath" else decimal.Decimal(v)


@contextlib.contextmanager
def _digits():
    if BACKEND == "mpmath":
        with mpmath.workdps(DPS):
            yield
    else:
        with decimal.localcontext() as c:
            c.prec = DPS
            yield


GAS_ONLY, GAS_AND_OIL, OIL_ONLY = 0, 1, 2          # include/opmgpu.h: OPMGPU_HC_*
EPS_BLEND = 1e-5
SO_FLOOR = 1.4901161193847656e-08                  # sqrt(DBL_EPSILON)
NAMES = ["p_w", "p_o", "p_g", "b_w", "b_o", "b_g", "mu_w", "mu_o", "mu_g", "kr_w", "kr_o", "kr_g", "rho_w", "rho_o", "rho_g",
         "mob_w", "mob_o", "mob_g", "rs", "rv", "accum_w", "accum_o", "accum_g", "rsSat", "rvSat", "pvm"]
SLOTS = ("value", "d/dp", "d/dSw", "d/dX")

# seg: the segment evaluated; at: the node index the argument is exactly on (-1: none); side: -1 / +1 = at or beyond the first / last node
# (saturation tables: the clamp flag), below / above the table (PVT, ROCKTAB: extrapolated); n: the table's length
Seg = namedtuple("Seg", "seg at side n")


def _at(x, v):
    k = np.flatnonzero(x == v)
    return int(k[0]) if k.size else -1


def pvt_search(x, v):
    n = len(x)
    if n == 2 or v <= x[1]:
        i = 0
    elif v >= x[n - 2]:
        i = n - 2
    else:
        i = max(k for k in range(1, n - 1) if x[k] <= v)
    return Seg(i, _at(x, v), -1 if v < x[0] else (1 if v > x[-1] else 0), n)


def sat_search(x, v, right):
    n = len(x)
    side = -1 if v <= x[0] else (1 if v >= x[-1] else 0)
    inner = [k for k in range(1, n - 1) if (x[k] <= v if right else x[k] < v)]
    return Seg(max(inner) if inner else 0, _at(x, v), side, n)


def rocktab_search(x, v):
    n = len(x)
    inner = [k for k in range(1, n - 1) if x[k] < v]
    return Seg(max(inner) if inner else 0, _at(x, v), -1 if v < x[0] else (1 if v > x[-1] else 0), n)


class Tables:
    """the arrays of a decks.FluidTables, cut into regions"""

    def __init__(self, tab):
        self.tab = tab

    def sat(self, r):
        t = self.tab
        a, b = t.swof_ptr[r], t.swof_ptr[r + 1]
        c, d = t.sgof_ptr[r], t.sgof_ptr[r + 1]
        return dict(sw=t.swof_sw[a:b], krw=t.swof_krw[a:b], krow=t.swof_krow[a:b], pcow=t.swof_pcow[a:b],
                    sg=t.sgof_sg[c:d], krg=t.sgof_krg[c:d], krog=t.sgof_krog[c:d], pcgo=t.sgof_pcgo[c:d])

    def oil(self, r):
        t = self.tab
        a, b = t.oil_node_ptr[r], t.oil_node_ptr[r + 1]
        cols = [slice(t.oil_col_ptr[k], t.oil_col_ptr[k + 1]) for k in range(a, b)]
        return dict(rs=t.oil_rs[a:b], psat=t.oil_psat[a:b], ib=t.oil_invb_sat[a:b], ibm=t.oil_invbmu_sat[a:b],
                    col_y=[t.oil_col_p[s] for s in cols], col_ib=[t.oil_col_invb[s] for s in cols], col_ibm=[t.oil_col_invbmu[s] for s in cols])

    def gas(self, r):
        t = self.tab
        a, b = t.gas_node_ptr[r], t.gas_node_ptr[r + 1]
        cols = [slice(t.gas_col_ptr[k], t.gas_col_ptr[k + 1]) for k in range(a, b)]
        return dict(pg=t.gas_pg[a:b], rv=t.gas_rvsat[a:b], ib=t.gas_invb_sat[a:b], ibm=t.gas_invbmu_sat[a:b],
                    col_y=[t.gas_col_rv[s] for s in cols], col_ib=[t.gas_col_invb[s] for s in cols], col_ibm=[t.gas_col_invbmu[s] for s in cols])


def _lin64(x, y, i, v):
    return float(y[i]) + (float(y[i + 1]) - float(y[i])) / (float(x[i + 1]) - float(x[i])) * (v - float(x[i]))


def branches(tab, preg, sreg, p, sw, sg, rs, rv, hc, so_max=0.0):
    """the record of every discrete choice of the cell at its base point (see the module docstring)"""
    T = Tables(tab)
    S, O, G = T.sat(sreg), T.oil(preg), T.gas(preg)
    p, sw = float(p), float(sw)
    is_sg, is_rs, is_rv = hc == GAS_AND_OIL, hc == OIL_ONLY, hc == GAS_ONLY
    sgv = float(sg) if is_sg else ((1.0 - sw) if is_rv else 0.0)
    so = (1.0 - sw) - sgv
    br = dict(hc=int(hc), sw=sw, sg=sgv, so=so)
    br["swof"] = sat_search(S["sw"], sw, False)
    br["sgof"] = sat_search(S["sg"], sgv, True)
    swco = float(S["sw"][0])
    br["above_swco"] = sw > swco
    swow = sgv + (sw if sw > swco else swco)
    d = swow - swco
    br["swow"], br["d"] = swow, d
    br["krow"] = sat_search(S["sw"], swow, False)
    br["krog"] = sat_search(S["sg"], d, True)
    br["blend"] = ("interp" if d > EPS_BLEND / 2 else "k2") if d < EPS_BLEND else "full"
    g = br["sgof"]
    pcgo = float(S["pcgo"][0]) if g.side < 0 else (float(S["pcgo"][-1]) if g.side > 0 else _lin64(S["sg"], S["pcgo"], g.seg, sgv))
    pg = p + pcgo
    br["pg_value"] = pg
    br["psat"] = pvt_search(O["psat"], p)
    br["pg"] = pvt_search(G["pg"], pg)
    free_oil, free_gas = is_sg or is_rs, is_sg or is_rv
    br["oil"] = "sat" if (free_gas or not tab.has_disgas) else "under"
    if br["oil"] == "under":
        n = br["rs_node"] = pvt_search(O["rs"], float(rs))
        br["oil_col"] = (pvt_search(O["col_y"][n.seg], p), pvt_search(O["col_y"][n.seg + 1], p))
    br["gas"] = "sat" if (free_oil or not tab.has_vapoil) else "under"
    if br["gas"] == "under":
        n = br["pg"]
        br["gas_col"] = (pvt_search(G["col_y"][n.seg], float(rv)), pvt_search(G["col_y"][n.seg + 1], float(rv)))
    so_max = float(so_max)
    br["vap"] = tuple((vap > 0.0 and so_max > 0.01 and so < so_max, so < SO_FLOOR) for vap in (tab.vap1, tab.vap2))
    br["rocktab"] = rocktab_search(tab.rocktab_p, p) if tab.rocktab_n > 0 else None
    return br


def _m(a):
    return [mpf(float(v)) for v in a]


class _Frozen:
    """the tables of one (preg, sreg) as mpf lists, built once per region pair"""
    _cache = {}

    def __init__(self, tab, preg, sreg):
        T = Tables(tab)
        conv = lambda d: {k: ([_m(c) for c in v] if isinstance(v, list) else _m(v)) for k, v in d.items()}
        self.S, self.O, self.G = conv(T.sat(sreg)), conv(T.oil(preg)), conv(T.gas(preg))
        self.w = _m(tab.pvtw[preg])
        self.rhos = _m(tab.surface_density[preg])
        if tab.rocktab_n > 0:
            self.rt = (_m(tab.rocktab_p), _m(tab.rocktab_pvmult), _m(tab.rocktab_transmult))

    @classmethod
    def of(cls, tab, preg, sreg):
        key = (id(tab), preg, sreg, BACKEND)
        if key not in cls._cache:
            cls._cache[key] = (tab, cls(tab, preg, sreg))       # (tab kept alive so that its id stays its own)
        return cls._cache[key][1]


def _lin(x, y, i, v):
    return y[i] + (y[i + 1] - y[i]) / (x[i + 1] - x[i]) * (v - x[i])


def _satc(x, y, s, v):
    return y[0] if s.side < 0 else (y[-1] if s.side > 0 else _lin(x, y, s.seg, v))


def _lin2(xs, i, cy, cv, j0, j1, xv, yv):
    """UniformXTabulated2DFunction: each bracketing column at the same y, then linearly in x"""
    al = (xv - xs[i]) / (xs[i + 1] - xs[i])
    return _lin(cy[i], cv[i], j0, yv) * (1 - al) + _lin(cy[i + 1], cv[i + 1], j1, yv) * al


def evaluate(tab, preg, sreg, br, p, sw, x, so_max):
    """the 26 properties (NAMES) as mpf at (p, sw, x) with the choices of `br` frozen"""
    F = _Frozen.of(tab, preg, sreg)
    S, O, G = F.S, F.O, F.G
    hc = br["hc"]
    sg = x if hc == GAS_AND_OIL else ((1 - sw) if hc == GAS_ONLY else mpf(0))
    so = 1 - sw - sg
    # capillary pressures, two-phase curves
    pw = p - _satc(S["sw"], S["pcow"], br["swof"], sw)
    pg = p + _satc(S["sg"], S["pcgo"], br["sgof"], sg)
    krw = _satc(S["sw"], S["krw"], br["swof"], sw)
    krg = _satc(S["sg"], S["krg"], br["sgof"], sg)
    # three-phase kro (EclDefaultMaterial)
    swco = S["sw"][0]
    swp = sw if br["above_swco"] else swco
    # (the float64 sums of the base point plus the exact change from it: see the module docstring)
    swow = mpf(br["swow"]) + (sg - mpf(br["sg"])) + (swp - (mpf(br["sw"]) if br["above_swco"] else swco))
    d = mpf(br["d"]) + (swow - mpf(br["swow"]))
    kow = _satc(S["sw"], S["krow"], br["krow"], swow)
    kgo = _satc(S["sg"], S["krog"], br["krog"], d)
    eps = mpf(EPS_BLEND)
    if br["blend"] == "k2":
        kro = (kow + kgo) / 2
    else:
        k1 = (sg * kgo + (swp - swco) * kow) / d
        if br["blend"] == "full":
            kro = k1
        else:
            al = (eps - d) / (eps / 2)
            kro = (kow + kgo) / 2 * al + k1 * (1 - al)
    # saturated ratios with VAPPARS
    def vapf(k, vap):
        active, floor = br["vap"][k]
        if not active:
            return mpf(1)
        so_i = so + (mpf(SO_FLOOR) - mpf(br["so"])) if floor else so          # d so_i / d so = 1 on the floor too, as the rule is written
        return (so_i / mpf(float(so_max))) ** mpf(float(vap))
    rs_sat = _lin(O["psat"], O["rs"], br["psat"].seg, p) * vapf(1, tab.vap2) if tab.has_disgas else mpf(0)
    rv_sat = _lin(G["pg"], G["rv"], br["pg"].seg, pg) * vapf(0, tab.vap1) if tab.has_vapoil else mpf(0)
    rs = x if (tab.has_disgas and hc == OIL_ONLY) else rs_sat
    rv = x if (tab.has_vapoil and hc == GAS_ONLY) else rv_sat
    # water
    w = F.w
    X = w[2] * (pw - w[0])
    bw = (1 + X * (1 + X / 2)) / w[1]
    Y = (w[2] - w[4]) * (pw - w[0])
    muw = w[3] * w[1] * bw / (1 + Y * (1 + Y / 2))
    # oil
    if br["oil"] == "sat":
        i = br["psat"].seg
        bo, bmo = _lin(O["psat"], O["ib"], i, p), _lin(O["psat"], O["ibm"], i, p)
    else:
        i, (c0, c1) = br["rs_node"].seg, br["oil_col"]
        bo = _lin2(O["rs"], i, O["col_y"], O["col_ib"], c0.seg, c1.seg, rs, p)
        bmo = _lin2(O["rs"], i, O["col_y"], O["col_ibm"], c0.seg, c1.seg, rs, p)
    # gas
    i = br["pg"].seg
    if br["gas"] == "sat":
        bg, bmg = _lin(G["pg"], G["ib"], i, pg), _lin(G["pg"], G["ibm"], i, pg)
    else:
        c0, c1 = br["gas_col"]
        bg = _lin2(G["pg"], i, G["col_y"], G["col_ib"], c0.seg, c1.seg, pg, rv)
        bmg = _lin2(G["pg"], i, G["col_y"], G["col_ibm"], c0.seg, c1.seg, pg, rv)
    muo, mug = bo / bmo, bg / bmg
    rhos = F.rhos
    rho = (rhos[0] * bw, rhos[1] * bo + rhos[2] * rs * bo, rhos[2] * bg + rhos[1] * rv * bg)
    # rock
    pvm, trm = mpf(1), mpf(1)
    if br["rocktab"] is not None:
        k = br["rocktab"].seg
        pvm, trm = _lin(F.rt[0], F.rt[1], k, p), _lin(F.rt[0], F.rt[2], k, p)
    elif tab.rock_comp != 0.0:
        cp = mpf(float(tab.rock_comp)) * (p - mpf(float(tab.rock_pref)))
        pvm = 1 + cp + cp * cp / 2
    mob = (trm * krw / muw, trm * kro / muo, trm * krg / mug)
    aw, ao, ag = pvm * bw * sw, pvm * bo * so, pvm * bg * sg
    return [pw, p, pg, bw, bo, bg, muw, muo, mug, krw, kro, krg, rho[0], rho[1], rho[2], mob[0], mob[1], mob[2], rs, rv,
            aw, ao + rv * ag, ag + rs * ao, rs_sat, rv_sat, pvm]


def cell(tab, preg, sreg, p, sw, sg, rs, rv, hc, so_max=0.0):
    """(out[26][4] float64: value, d/dp, d/dSw, d/dX of NAMES; the branch record)"""
    with _digits():
        step = mpf(10) ** -25
        br = branches(tab, preg, sreg, p, sw, sg, rs, rv, hc, so_max)
        xv = rs if hc == OIL_ONLY else (rv if hc == GAS_ONLY else sg)
        base = [mpf(float(p)), mpf(float(sw)), mpf(float(xv))]
        out = np.zeros((len(NAMES), 4))
        out[:, 0] = [float(v) for v in evaluate(tab, preg, sreg, br, base[0], base[1], base[2], so_max)]
        for k in range(3):
            h = step * max(abs(base[k]), mpf("1e-3"))
            up, dn = list(base), list(base)
            up[k] += h; dn[k] -= h
            fu = evaluate(tab, preg, sreg, br, up[0], up[1], up[2], so_max)
            fd = evaluate(tab, preg, sreg, br, dn[0], dn[1], dn[2], so_max)
            out[:, 1 + k] = [float((a - b) / (2 * h)) for a, b in zip(fu, fd)]
        return out, br


def cells(tab, pvtnum, satnum, st, so_max=None):
    """every cell of a decks.State: (out[nc][26][4], list of branch records)"""
    n = st.p.size
    out, recs = np.zeros((n, len(NAMES), 4)), []
    for c in range(n):
        o, br = cell(tab, int(pvtnum[c]), int(satnum[c]), st.p[c], st.sat[c, 0], st.sat[c, 2], st.rs[c], st.rv[c], int(st.hc[c]),
                     0.0 if so_max is None else so_max[c])
        out[c] = o
        recs.append(br)
    return out, recs
