"""Killough's relative-permeability hysteresis of the non-wetting phases, restated in numpy from the text of include/opmgpu.h alone
(opmgpu_set_hysteresis_model for the rule, opmgpu_grid for the fixed points of the end-point scaling, opmgpu_tables::threephase_model
for the default three-phase law).  No device code and no oracle code was consulted for the rule: it is what tests/test_killough_*.py and
tests/test_gpu_killough*.py pin the device to.  Plain float64, one cell at a time: clarity over speed, the grids of the tests are small.

    curves = cell_systems(tab, grid, c)              # {"go": System, "ow": System} of cell c: krnd, krni, Sncrd, Sncri, Snmax
    sncrt, m, R = scan(system, mdc, a)               # the scanning parameters at a history value (mdc = 2: none)
    krn(system, mdc, a, sn)                          # the non-wetting relative permeability at Sn (drainage or scanning side)
    kr_cell(tab, grid, c, mdc_ow, mdc_go, a, sw, sg) # (krg, kro) of the default three-phase law with both systems' scanning curves
    twin_tables(...)                                 # "Carlson with zero shift on a twin imbibition table", one region per cell
"""
import numpy as np

NO_HISTORY = 2.0


class Scaled:
    """A tabulated curve y(x) seen through one cell's scaling: S -> x by the piecewise-linear map through the fixed points
    (s_pts[j] <-> u_pts[j], two or three of them, extrapolated along the end pieces), the table value times vfac."""

    def __init__(self, x, y, s_pts=None, u_pts=None, vfac=1.0):
        self.x, self.y = np.asarray(x, float), np.asarray(y, float)
        self.s_pts = None if s_pts is None else [float(v) for v in s_pts]
        self.u_pts = None if u_pts is None else [float(v) for v in u_pts]
        self.vfac = float(vfac)

    def to_table(self, s):
        if self.s_pts is None:
            return s
        sp, up = self.s_pts, self.u_pts
        if len(sp) == 3 and s >= sp[1]:
            return up[1] + (s - sp[1]) * ((up[2] - up[1]) / (sp[2] - sp[1]))
        return up[0] + (s - sp[0]) * ((up[1] - up[0]) / (sp[1] - sp[0]))

    def from_table(self, u):
        if self.s_pts is None:
            return u
        sp, up = self.s_pts, self.u_pts
        if len(sp) == 3 and u >= up[1]:
            return sp[1] + (u - up[1]) / ((up[2] - up[1]) / (sp[2] - sp[1]))
        return sp[0] + (u - up[0]) / ((up[1] - up[0]) / (sp[1] - sp[0]))

    def __call__(self, s):
        return self.vfac * float(np.interp(self.to_table(s), self.x, self.y))       # (constant beyond the table's ends)


class System:
    """One two-phase system of a cell in its non-wetting saturation Sn"""

    def __init__(self, krnd, krni, sncrd, sncri, snmax):
        self.krnd, self.krni, self.sncrd, self.sncri, self.snmax = krnd, krni, sncrd, sncri, snmax


def _zero_run_low(x, y):
    i = 0
    while i + 1 < len(y) and y[i + 1] <= 0.0:
        i += 1
    return x[i]


def _zero_run_high(x, y):
    i = len(y) - 1
    while i > 0 and y[i - 1] <= 0.0:
        i -= 1
    return x[i]


def table_points(tab, reg):
    """unscaled end points read off a region's tables: SWL SWCR SWU SOWCR SGL SGCR SGU SOGCR"""
    a, b = tab.swof_ptr[reg], tab.swof_ptr[reg + 1]
    sw, krw, krow = tab.swof_sw[a:b], tab.swof_krw[a:b], tab.swof_krow[a:b]
    a, b = tab.sgof_ptr[reg], tab.sgof_ptr[reg + 1]
    sg, krg, krog = tab.sgof_sg[a:b], tab.sgof_krg[a:b], tab.sgof_krog[a:b]
    first_zero = lambda x, y: x[np.flatnonzero(y == 0.0)[0]] if np.any(y == 0.0) else x[-1]       # noqa: E731
    return {"SWL": sw[0], "SWCR": _zero_run_low(sw, krw), "SWU": sw[-1], "SOWCR": 1.0 - first_zero(sw, krow),
            "SGL": sg[0], "SGCR": _zero_run_low(sg, krg), "SGU": sg[-1], "SOGCR": 1.0 - first_zero(sg, krog)}


_NAMES = ("SWL", "SWCR", "SWU", "SOWCR", "SGL", "SGCR", "SGU", "SOGCR")


def _points(e, curve, three):
    """fixed points of a curve (opmgpu_grid: eps / scalecrs) for the end points e"""
    if curve == "krg":
        p = [e["SGCR"], 1.0 - e["SOGCR"] - e["SWL"], e["SGU"]]
    elif curve == "krow":
        p = [e["SWL"] + e["SGL"], e["SWCR"] + e["SGL"], 1.0 - e["SOWCR"] - e["SGL"]]
    elif curve == "krog":       # in oil saturation
        p = [e["SOGCR"], 1.0 - e["SGCR"] - e["SWL"], 1.0 - e["SWL"] - e["SGL"]]
    else:
        raise KeyError(curve)
    return p if three else [p[0], p[2]]


def scaled_curve(tab, grid, c, reg, curve, ends):
    """curve "krg" / "krow" / "krog" of table region reg as cell c sees it through the end points `ends` (list of eight arrays or None)"""
    if curve == "krow":
        a, b = tab.swof_ptr[reg], tab.swof_ptr[reg + 1]
        x, y, vname, ymax = tab.swof_sw[a:b], tab.swof_krow[a:b], "KRO", tab.swof_krow[a]
    else:
        a, b = tab.sgof_ptr[reg], tab.sgof_ptr[reg + 1]
        x = tab.sgof_sg[a:b]
        y, vname, ymax = (tab.sgof_krg[a:b], "KRG", tab.sgof_krg[b - 1]) if curve == "krg" else (tab.sgof_krog[a:b], "KRO", tab.sgof_krog[a])
    v = 1.0
    if grid.eps_v is not None and vname in grid.eps_v and ymax != 0.0:
        v = grid.eps_v[vname][c] / ymax
    if ends is None:
        return Scaled(x, y, vfac=v)
    e = {k: ends[i][c] for i, k in enumerate(_NAMES)}
    return Scaled(x, y, _points(e, curve, grid.scalecrs), _points(table_points(tab, reg), curve, grid.scalecrs), v)


def cell_systems(tab, grid, c):
    sreg = 0 if grid.satnum is None else int(grid.satnum[c])
    ireg = int(grid.imbnum[c])
    iends = grid.ieps if grid.ieps is not None else grid.eps
    gd, gi = scaled_curve(tab, grid, c, sreg, "krg", grid.eps), scaled_curve(tab, grid, c, ireg, "krg", iends)
    go = System(gd, gi, gd.from_table(_zero_run_low(gd.x, gd.y)), gi.from_table(_zero_run_low(gi.x, gi.y)), gd.from_table(gd.x[-1]))
    wd, wi = scaled_curve(tab, grid, c, sreg, "krow", grid.eps), scaled_curve(tab, grid, c, ireg, "krow", iends)
    ow = System(lambda s: wd(1.0 - s), lambda s: wi(1.0 - s), 1.0 - wd.from_table(_zero_run_high(wd.x, wd.y)),
                1.0 - wi.from_table(_zero_run_high(wi.x, wi.y)), 1.0 - wd.from_table(wd.x[0]))
    ow.table_d, ow.table_i, go.table_d, go.table_i = wd, wi, gd, gi
    return {"go": go, "ow": ow}


def scan(s, mdc, a):
    """(Sncrt, m, R) of system s at the history value mdc; without a history m = R = 1 and Sncrt = 0"""
    if not mdc < NO_HISTORY:
        return 0.0, 1.0, 1.0
    shy = min(1.0 - mdc, s.snmax)
    kd, ki, D = s.krnd(shy), s.krni(s.snmax), shy - s.sncrd
    sncrt = s.sncrd
    if s.sncri > s.sncrd and s.snmax > s.sncrd:
        C = 1.0 / (s.sncri - s.sncrd) - 1.0 / (s.snmax - s.sncrd)
        sncrt = s.sncrd + D / (1.0 + a * (s.snmax - shy) + C * D)
    if kd <= 0.0 or ki <= 0.0 or s.snmax <= s.sncri:
        return sncrt, 0.0, 0.0
    return sncrt, (s.snmax - s.sncri) / (shy - sncrt), kd / ki


def in_guard(s, mdc):
    """a cell with a history whose scanning side is the zero curve (R = m = 0)"""
    return mdc < NO_HISTORY and scan(s, mdc, 0.1)[1] == 0.0


def krn(s, mdc, a, sn):
    if mdc < NO_HISTORY and 1.0 - sn > mdc:             # the scanning side (the switch is Carlson's)
        sncrt, m, R = scan(s, mdc, a)
        return R * s.krni(s.sncri + m * (sn - sncrt))
    return s.krnd(sn)


def kr_cell(tab, grid, c, mdc_ow, mdc_go, a, sw, sg):
    """(krg, kro) of cell c: the default three-phase law (opmgpu_tables::threephase_model) over the two systems' non-wetting curves"""
    sy = cell_systems(tab, grid, c)
    sreg = 0 if grid.satnum is None else int(grid.satnum[c])
    krg = krn(sy["go"], mdc_go, a, sg)
    swco = grid.eps[0][c] if grid.eps is not None else tab.swof_sw[tab.swof_ptr[sreg]]
    swp = max(sw, swco)
    swow = sg + swp
    kow = krn(sy["ow"], mdc_ow, a, 1.0 - swow)
    og = scaled_curve(tab, grid, c, sreg, "krog", grid.eps)
    if grid.eps is not None:        # krog is tabulated against the oil saturation 1 - Swco_table - Sg: the scaling acts on that axis
        kgo = og.vfac * float(np.interp(1.0 - tab.swof_sw[tab.swof_ptr[sreg]] - og.to_table(1.0 - swow), og.x, og.y))
    else:
        kgo = og.vfac * float(np.interp(swow - swco, og.x, og.y))
    den, eps = swow - swco, 1e-5
    num = sg * kgo + (swp - swco) * kow
    if den < eps:
        k2 = 0.5 * (kow + kgo)
        if den > eps / 2:
            al = (eps - den) / (eps / 2)
            return krg, k2 * al + (num / den) * (1.0 - al)
        return krg, k2
    return krg, num / den


def scanning_planes(tab, grid, mdc_ow, mdc_go, a):
    """dict of [nc] arrays: sncrt / m / r / sncrd / sncri / snmax / guard, each suffixed _ow / _go"""
    out = {k + "_" + s: np.zeros(grid.nc) for k in ("sncrt", "m", "r", "sncrd", "sncri", "snmax", "shy") for s in ("ow", "go")}
    out["guard_ow"], out["guard_go"] = np.zeros(grid.nc, bool), np.zeros(grid.nc, bool)
    for c in range(grid.nc):
        sy = cell_systems(tab, grid, c)
        for name, mdc in (("ow", mdc_ow[c]), ("go", mdc_go[c])):
            s = sy[name]
            out["sncrt_" + name][c], out["m_" + name][c], out["r_" + name][c] = scan(s, mdc, a)
            out["sncrd_" + name][c], out["sncri_" + name][c], out["snmax_" + name][c] = s.sncrd, s.sncri, s.snmax
            out["shy_" + name][c] = min(1.0 - mdc, s.snmax)
            out["guard_" + name][c] = in_guard(s, mdc)
    return out


def twin_table(x, y, a0, m, R):
    """The twin of an imbibition table for R y(a0 + m S): abscissae (x - a0) / m, ordinates R y; all-zero ordinates (abscissae kept)
    where R = 0.  Carlson with ZERO shift on it is Killough's scanning curve."""
    x, y = np.asarray(x, float), np.asarray(y, float)
    if R == 0.0 or m == 0.0:
        return x.copy(), np.zeros_like(y)
    return (x - a0) / m, R * y
