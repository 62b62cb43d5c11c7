"""Rock regions and irreversible compaction, restated from the rule written in include/opmgpu.h at opmgpu_set_rock_regions -- from that
text alone, not from the device code.

The rule, per cell c with region r = rocknum[c], pressure p and history p_min[c]:
    table region   on_curve = (mode == REVERSIBLE) or (p <= p_min)     (a tie is on the curve)
                   x = p if on_curve else p_min
                   pv_mult = L(pv table of r, x), trans_mult = L(trans table of r, x); L: piecewise linear, the LEFT segment at a
                   breakpoint, the end segments extrapolated beyond both ends; d/dp = the segment's slope on the curve, exactly 0 off it
    ROCK form      (0 rows) always at p: pv_mult = 1 + X + X^2 / 2, X = rock_comp (p - rock_pref); trans_mult = 1
    history        p_min = min(p_min, p), starting at +inf
pv_mult multiplies every accumulation term, trans_mult the three mobilities; nothing else of the cell changes.

Three restatements:
    history()      NumPy, exact: the device must match bit for bit
    multipliers()  float64, y_i + slope_i (x - x_i) with slope_i = (y_(i+1) - y_i) / (x_(i+1) - x_i) rounded once, as the rule says the
                   slopes are formed; with the magnitude |y_i| + |slope_i (x - x_i)| that the tolerance of a comparison is stated in
    cell()         all 26 properties of tests/cell_reference.py with their derivatives at 50 digits.  That module's evaluator is used as it
                   is: a cell on its curve, and a ROCK-form cell, is the cell of a table set whose ONE rock is the region's (a view of the
                   tables with the rock fields replaced); a cell off its curve is the cell without any rock, its accumulation terms times
                   the constant L(pv table, p_min), its mobilities times L(trans table, p_min), both formed at 50 digits.
`regions` is any object with the fields of opmgpu.decks.RockRegions (SI)."""
import numpy as np

import cell_reference as R

REVERSIBLE, IRREVERSIBLE = 0, 1             # include/opmgpu.h: OPMGPU_ROCK_*
INF = float("inf")
I_MOB, I_ACCUM, I_PVM = R.NAMES.index("mob_w"), R.NAMES.index("accum_w"), R.NAMES.index("pvm")


def table_of(regions, r):
    """(p, pv_mult, trans_mult) of region r's table, or None for the ROCK form"""
    a, b = int(regions.tab_ptr[r]), int(regions.tab_ptr[r + 1])
    return None if a == b else (regions.tab_p[a:b], regions.tab_pvmult[a:b], regions.tab_transmult[a:b])


def branch(regions, r, p, p_min):
    """the discrete choices of one cell: form ('table' / 'rock'), on_curve, tie (p == p_min), the argument x of the look-ups and its
    search record (cell_reference.Seg: seg, at = the node x is exactly on or -1, side = -1 / +1 below / above the table, n)"""
    t = table_of(regions, r)
    p, p_min = float(p), float(p_min)
    if t is None:
        return dict(form="rock", on_curve=True, tie=p == p_min, x=p, search=None, region=int(r), fresh=p_min == INF)
    on = int(regions.mode) == REVERSIBLE or p <= p_min
    x = p if on else p_min
    return dict(form="table", on_curve=bool(on), tie=p == p_min, x=x, search=R.rocktab_search(t[0], x), region=int(r), fresh=p_min == INF)


def history(p_min, p):
    return np.minimum(p_min, p)


def multipliers(regions, rocknum, p, p_min):
    """float64: (pv_mult, trans_mult, d pv_mult / dp, d trans_mult / dp, |y_i| + |slope (x - x_i)| of the pv look-up, of the trans
    look-up) per cell; the last two are 0 for a ROCK-form cell, whose bound the caller states itself"""
    n = len(p)
    out = [np.zeros(n) for _ in range(6)]
    for c in range(n):
        r = int(rocknum[c])
        b = branch(regions, r, p[c], p_min[c])
        if b["form"] == "rock":
            X = float(regions.rock_comp[r]) * (float(p[c]) - float(regions.rock_pref[r]))
            out[0][c], out[1][c] = 1.0 + X + 0.5 * X * X, 1.0
            out[2][c] = float(regions.rock_comp[r]) * (1.0 + X)
            continue
        x, ypv, ytr = table_of(regions, r)
        i, h = b["search"].seg, b["x"] - float(x[b["search"].seg])
        for k, y in ((0, ypv), (1, ytr)):
            s = (float(y[i + 1]) - float(y[i])) / (float(x[i + 1]) - float(x[i]))
            out[k][c] = float(y[i]) + s * h
            out[2 + k][c] = s if b["on_curve"] else 0.0
            out[4 + k][c] = abs(float(y[i])) + abs(s * h)
    return tuple(out)


class _View:
    """a table set with some fields replaced (the rock of ONE region, or none)"""

    def __init__(self, tab, **over):
        self._tab = tab
        self.__dict__.update(over)

    def __getattr__(self, k):
        return getattr(self._tab, k)


_views = {}


def _view(tab, regions, r, plain):
    key = (id(tab), id(regions), int(r), bool(plain))
    if key not in _views:
        t = None if plain else table_of(regions, r)
        if plain:
            v = _View(tab, rocktab_n=0, rock_pref=0.0, rock_comp=0.0)
        elif t is None:
            v = _View(tab, rocktab_n=0, rock_pref=float(regions.rock_pref[r]), rock_comp=float(regions.rock_comp[r]))
        else:
            v = _View(tab, rocktab_n=len(t[0]), rocktab_p=t[0], rocktab_pvmult=t[1], rocktab_transmult=t[2], rock_pref=0.0, rock_comp=0.0)
        _views[key] = (tab, regions, v)          # (both kept alive so that their ids stay their own)
    return _views[key][2]


def cell(tab, regions, r, preg, sreg, p, sw, sg, rs, rv, hc, p_min, so_max=0.0):
    """(out[26][4] float64: value, d/dp, d/dSw, d/dX of cell_reference.NAMES; the rock branch record with the fluid's under 'fluid')"""
    with R._digits():
        rec = branch(regions, r, p, p_min)
        frozen = rec["form"] == "table" and not rec["on_curve"]
        view = _view(tab, regions, r, plain=frozen)
        cpv = ctr = None
        if frozen:
            x, ypv, ytr = table_of(regions, r)
            i, xv = rec["search"].seg, R.mpf(rec["x"])
            lin = lambda y: R.mpf(float(y[i])) + (R.mpf(float(y[i + 1])) - R.mpf(float(y[i]))) / (R.mpf(float(x[i + 1])) - R.mpf(float(x[i]))) * (xv - R.mpf(float(x[i])))   # noqa: E731
            cpv, ctr = lin(ypv), lin(ytr)
        br = R.branches(view, preg, sreg, p, sw, sg, rs, rv, hc, so_max)
        rec["fluid"] = br

        def ev(a, b, c):
            v = R.evaluate(view, preg, sreg, br, a, b, c, so_max)
            if frozen:
                for k in range(3):
                    v[I_MOB + k] = ctr * v[I_MOB + k]
                    v[I_ACCUM + k] = cpv * v[I_ACCUM + k]
                v[I_PVM] = cpv
            return v
        step = R.mpf(10) ** -25
        xv = rs if hc == R.OIL_ONLY else (rv if hc == R.GAS_ONLY else sg)
        base = [R.mpf(float(p)), R.mpf(float(sw)), R.mpf(float(xv))]
        out = np.zeros((len(R.NAMES), 4))
        out[:, 0] = [float(v) for v in ev(*base)]
        for k in range(3):
            h = step * max(abs(base[k]), R.mpf("1e-3"))
            up, dn = list(base), list(base)
            up[k] += h; dn[k] -= h
            out[:, 1 + k] = [float((a - b) / (2 * h)) for a, b in zip(ev(*up), ev(*dn))]
        return out, rec


def cells(tab, regions, rocknum, pvtnum, satnum, st, p_min, so_max=None):
    """every cell of a decks.State: (out[nc][26][4], list of branch records)"""
    n = st.p.size
    out, recs = np.zeros((n, len(R.NAMES), 4)), []
    for c in range(n):
        o, rec = cell(tab, regions, int(rocknum[c]), int(pvtnum[c]), int(satnum[c]), st.p[c], st.sat[c, 0], st.sat[c, 2], st.rs[c], st.rv[c],
                      int(st.hc[c]), p_min[c], 0.0 if so_max is None else so_max[c])
        out[c] = o
        recs.append(rec)
    return out, recs
