"""numpy restatement of the capillary-pressure curves of a set of cells and of the SWATINIT rule, the checker of
tests/test_gpu_swatinit.py.  Written from the statement of the rule (include/opmgpu.h, opmgpu_set_swatinit_scaling), not from
opmgpu/equil.py or the device code:

  table look-up     piecewise linear between the table's nodes, constant beyond its first and last node
  horizontal map    two-point: S_table = u0 + (S - s0) * (u2 - u0) / (s2 - s0), with (s0, s2) the cell's scaled end points (SWL, SWU for
                    pcow; SGL, SGU for pcgo) and (u0, u2) the first and last saturation node of the cell's table; without end points
                    the saturation goes to the table as it is
  vertical factor   cell maximum / table maximum (PCW against the first pcow node, PCG against the last pcgo node); 1 without an array
                    or where the table maximum is zero
  the rule          pcow < 0: sw_out = Swu, PCW unchanged; else Sw = min(max(sw, Swl), Swu) = sw_out, pc_at = pcow(Sw) on the current
                    curve and, where pc_at > 0, PCW *= pcow / pc_at
"""
import numpy as np


def _table(x, y, xv):
    xv = np.asarray(xv, float)
    i = np.clip(np.searchsorted(x, xv, side="left") - 1, 0, len(x) - 2)
    f = y[i] + (y[i + 1] - y[i]) / (x[i + 1] - x[i]) * (xv - x[i])
    return np.where(xv <= x[0], y[0], np.where(xv >= x[-1], y[-1], f))


class Curves:
    """pcow(Sw) and pcgo(Sg) of the nc cells of `grid` (an opmgpu.decks.GridData: satnum, eps, eps_v) on `tables` (FluidTables)"""

    def __init__(self, grid, tables):
        t, n = tables, grid.nc
        self.n = n
        self.sat = np.zeros(n, int) if grid.satnum is None else np.asarray(grid.satnum, int)
        self.gas = getattr(t, "phases", "wog") != "wo"
        self.w, self.g = {}, {}
        for r in range(t.n_sat):
            a, b = t.swof_ptr[r], t.swof_ptr[r + 1]
            self.w[r] = (np.array(t.swof_sw[a:b]), np.array(t.swof_pcow[a:b]))
            if self.gas:
                a, b = t.sgof_ptr[r], t.sgof_ptr[r + 1]
                self.g[r] = (np.array(t.sgof_sg[a:b]), np.array(t.sgof_pcgo[a:b]))
        self.pcw_tab = np.array([self.w[r][1][0] for r in self.sat])
        self.swl_tab = np.array([self.w[r][0][0] for r in self.sat])
        self.swu_tab = np.array([self.w[r][0][-1] for r in self.sat])
        names = list(grid.EPS_NAMES)
        self.scaled = grid.eps is not None
        if self.scaled:
            self.swl, self.swu = np.array(grid.eps[names.index("SWL")]), np.array(grid.eps[names.index("SWU")])
            self.sgl, self.sgu = np.array(grid.eps[names.index("SGL")]), np.array(grid.eps[names.index("SGU")])
        else:
            self.swl, self.swu = self.swl_tab.copy(), self.swu_tab.copy()
        ev = grid.eps_v or {}
        self.pcw = np.where(self.pcw_tab != 0.0, ev["PCW"], self.pcw_tab) if "PCW" in ev else self.pcw_tab.copy()
        self.pcg = ev.get("PCG")

    def pcow(self, sw):
        sw = np.asarray(sw, float)
        out = np.zeros(self.n)
        for r, (x, y) in self.w.items():
            m = self.sat == r
            s = sw[m]
            if self.scaled:
                s = x[0] + (s - self.swl[m]) * ((x[-1] - x[0]) / (self.swu[m] - self.swl[m]))
            v = self.pcw[m] / y[0] if y[0] != 0.0 else 1.0
            out[m] = _table(x, y, s) * v
        return out

    def pcgo(self, sg):
        out = np.zeros(self.n)
        if not self.gas:
            return out
        sg = np.asarray(sg, float)
        for r, (x, y) in self.g.items():
            m = self.sat == r
            s = sg[m]
            if self.scaled:
                s = x[0] + (s - self.sgl[m]) * ((x[-1] - x[0]) / (self.sgu[m] - self.sgl[m]))
            v = self.pcg[m] / y[-1] if (self.pcg is not None and y[-1] != 0.0) else 1.0
            out[m] = _table(x, y, s) * v
        return out

    def apply_swatinit(self, sw, pcow):
        """the rule for all cells; returns (sw_out, the cells whose PCW was rescaled)"""
        sw, pcow = np.asarray(sw, float), np.asarray(pcow, float)
        s = np.minimum(np.maximum(sw, self.swl), self.swu)
        pc_at = self.pcow(s)
        scaled = ~(pcow < 0.0) & (pc_at > 0.0)
        self.pcw = np.where(scaled, self.pcw * (pcow / np.where(scaled, pc_at, 1.0)), self.pcw)
        return np.where(pcow < 0.0, self.swu, s), scaled
