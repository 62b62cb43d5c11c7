"""Stone I / Stone II three-phase oil relative permeability, restated in numpy from the rule in include/opmgpu.h
(opmgpu_tables::threephase_model) -- NOT from the kernel.  The rule is this project's own (opm-material, which holds the reference's, is not
part of its tree).

Everything here is complex-safe: table segments and switches are chosen by the real part, the arithmetic carries the imaginary part, so
derivatives come from the complex step, d f / d x = Im f(x + i h) / h with h = 1e-30 (as in oracle/wells.py).

Tables are piecewise linear with constant extrapolation.  Two-point end-point scaling (include/opmgpu.h, opmgpu_grid::eps / eps_v): a curve is
looked up at  u0 + (S - s0) (u1 - u0) / (s1 - s0)  where [s0, s1] are the cell's scaled end points of that curve and [u0, u1] the same points
read off the table:
    krw           [SWCR, SWU]                    krg                 [SGCR, SGU]
    krow (in Sw)  [SWL + SGL, 1 - SOWCR - SGL]   krog (in So)        [SOGCR, 1 - SWL - SGL]
krog is tabulated against Sg; its oil saturation is So = 1 - Swl_table - Sg.  Vertical scaling: the value times (cell maximum / table
maximum); the KRO maximum refers to krow at the first Sw node and to krog at the first Sg node.
"""
import numpy as np

DEFAULT, STONE1, STONE2 = 0, 1, 2
EPS_NAMES = ("SWL", "SWCR", "SWU", "SOWCR", "SGL", "SGCR", "SGU", "SOGCR")
H = 1e-30


def lookup(x, y, xv):
    """piecewise linear y(x) at xv (complex allowed), constant beyond the end nodes"""
    xr = np.real(xv)
    if xr <= x[0]:
        return y[0] + 0 * xv
    if xr >= x[-1]:
        return y[-1] + 0 * xv
    i = int(np.searchsorted(x, xr, side="right")) - 1
    return y[i] + (y[i + 1] - y[i]) / (x[i + 1] - x[i]) * (xv - x[i])


class Region:
    """SWOF / SGOF of one saturation region and the end points read off them"""

    def __init__(self, tab, r):
        a, b = tab.swof_ptr[r], tab.swof_ptr[r + 1]
        self.sw, self.krw, self.krow = tab.swof_sw[a:b], tab.swof_krw[a:b], tab.swof_krow[a:b]
        a, b = tab.sgof_ptr[r], tab.sgof_ptr[r + 1]
        self.sg, self.krg, self.krog = tab.sgof_sg[a:b], tab.sgof_krg[a:b], tab.sgof_krog[a:b]

        def last_zero(x, y):
            i = 0
            while i + 1 < len(x) and y[i + 1] == 0.0:
                i += 1
            return x[i]

        def first_zero(x, y):
            i = 0
            while i < len(x) - 1 and y[i] != 0.0:
                i += 1
            return x[i]
        self.unscaled = {"SWL": self.sw[0], "SWCR": last_zero(self.sw, self.krw), "SWU": self.sw[-1], "SOWCR": 1.0 - first_zero(self.sw, self.krow),
                         "SGL": self.sg[0], "SGCR": last_zero(self.sg, self.krg), "SGU": self.sg[-1], "SOGCR": 1.0 - first_zero(self.sg, self.krog)}


def _ends(e):
    """the two fixed points of every curve from a set of eight end points"""
    return {"krw": (e["SWCR"], e["SWU"]), "krg": (e["SGCR"], e["SGU"]),
            "krow": (e["SWL"] + e["SGL"], 1.0 - e["SOWCR"] - e["SGL"]), "krog": (e["SOGCR"], 1.0 - e["SWL"] - e["SGL"])}


class Cell:
    """The saturation functions of one cell: region tables, optionally the cell's eight scaled end points (dict) and its KRO maximum."""

    def __init__(self, region, eps=None, kro_max=None):
        self.R, self.eps, self.kro_max = region, eps, kro_max
        self.u = _ends(region.unscaled)
        self.s = _ends(eps) if eps is not None else None

    def _map(self, curve, s):
        if self.s is None:
            return s
        (s0, s1), (u0, u1) = self.s[curve], self.u[curve]
        return u0 + (s - s0) * ((u1 - u0) / (s1 - s0))

    def _unmap(self, curve, u):
        if self.s is None:
            return u
        (s0, s1), (u0, u1) = self.s[curve], self.u[curve]
        return s0 + (u - u0) * ((s1 - s0) / (u1 - u0))

    def v_krow(self):
        return 1.0 if self.kro_max is None or self.R.krow[0] == 0.0 else self.kro_max / self.R.krow[0]

    def v_krog(self):
        return 1.0 if self.kro_max is None or self.R.krog[0] == 0.0 else self.kro_max / self.R.krog[0]

    def krw(self, sw):
        return lookup(self.R.sw, self.R.krw, self._map("krw", sw))

    def krg(self, sg):
        return lookup(self.R.sg, self.R.krg, self._map("krg", sg))

    def krow(self, sw):
        return lookup(self.R.sw, self.R.krow, self._map("krow", sw)) * self.v_krow()

    def krog_of_so(self, so):
        return lookup(self.R.sg, self.R.krog, 1.0 - self.R.sw[0] - self._map("krog", so)) * self.v_krog()

    @property
    def swco(self):
        return self.eps["SWL"] if self.eps is not None else self.R.sw[0]

    @property
    def krocw(self):
        return self.R.krow[0] * self.v_krow()

    @property
    def som(self):
        e = self.eps if self.eps is not None else self.R.unscaled
        return min(e["SOWCR"], e["SOGCR"])

    # ---- where the functions of (Sw, Sg) have kinks: table nodes in the cell's own saturations, and the law's switches
    def sw_kinks(self):
        return np.concatenate([self._unmap("krw", self.R.sw), self._unmap("krow", self.R.sw), [self.swco]])

    def sg_kinks(self):
        so_nodes = self._unmap("krog", 1.0 - self.R.sw[0] - self.R.sg)           # krog nodes as oil saturations of the cell
        return np.concatenate([self._unmap("krg", self.R.sg), 1.0 - self.swco - so_nodes])


def kro(model, cell, sw, sg, eta=1.0):
    """kro of `cell` at (sw, sg) by the rule of include/opmgpu.h; sw, sg may be complex"""
    swco, krocw = cell.swco, cell.krocw
    zero = 0.0 * (sw + sg)
    if not krocw > 0.0:
        return zero
    sws = sw if np.real(sw) > swco else swco + 0.0 * sw          # Sw* = max(Sw, Swco), derivative 0 below Swco
    krw, krg = cell.krw(sw), cell.krg(sg)
    krow = cell.krow(sws)
    krog = cell.krog_of_so(1.0 - swco - sg)
    if model == STONE2:
        k = krocw * ((krow / krocw + krw) * (krog / krocw + krg) - krw - krg)
    elif model == STONE1:
        som = cell.som
        D = 1.0 - swco - som
        sos = 1.0 - sws - sg
        if D <= 0.0 or np.real(sos) <= som:
            return zero
        sso, ssw, ssg = (sos - som) / D, (sws - swco) / D, sg / D
        beta = (sso / ((1.0 - ssw) * (1.0 - ssg))) ** eta
        k = beta * krow * krog / krocw
    else:
        raise ValueError("not a Stone model: %r" % (model,))
    return k if np.real(k) > 0.0 else zero


def kro_and_derivatives(model, cell, sw, sg, eta=1.0):
    """(kro, d kro / d Sw, d kro / d Sg) by the complex step"""
    v = kro(model, cell, sw, sg, eta)
    dw = np.imag(kro(model, cell, sw + 1j * H, sg, eta)) / H
    dg = np.imag(kro(model, cell, sw, sg + 1j * H, eta)) / H
    return float(np.real(v)), float(dw), float(dg)


def cells_of(tab, satnum, eps=None, kro_max=None):
    """one Cell per grid cell; eps: dict name -> [nc] array, kro_max: [nc] array"""
    regions = [Region(tab, r) for r in range(tab.n_sat)]
    out = []
    for c, r in enumerate(satnum):
        e = None if eps is None else {k: float(np.asarray(eps[k])[c]) for k in EPS_NAMES}
        out.append(Cell(regions[r], e, None if kro_max is None else float(kro_max[c])))
    return out
