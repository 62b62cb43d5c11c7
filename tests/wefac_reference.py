"""Reference for the well efficiency factors (WEFAC): oracle.wells.CoupledOracleModel -- complex-step derivatives, ONE sparse system with
the well unknowns as extra rows and columns, a direct solve -- with the factors applied where the reference applies them
(addWellContributionToMassBalanceEq, BlackoilModelBase_impl.hpp:953-975, subtracts efficiency_factors * cq_s; StandardWells_impl.hpp:1405-1434
builds that vector, one value per well copied to its perforations):

    reservoir rows     R_a[cell_j] -= e_w cq_s[a][j];   blocks  -e_w d cq_s / dx  and  -e_w d cq_s / dy
    well rows          unchanged: E, dE/dx, dE/dy

Only `assemble` and `solveJacobianSystem` are overridden, each a restatement of the parent's with e_w at those three places; everything else
-- the well equations, the pre-solve, the control logic, the connection pressures, the well state update -- is the parent's, which knows
nothing of a factor.  No Schur complement in either form (explicit or factored) is involved.  With every factor 1 the products are exact
and the subclass computes bit for bit what its parent computes (tests/test_wefac.py)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import oracle as orc
from oracle.wells import CoupledOracleModel, NumericalIssue, WellStateArrays


def arrays(ws):
    """a WellState of opmgpu/wells.py as the plain arrays the oracle model takes"""
    return WellStateArrays(ws.bhp, ws.qs, ws.perf_press, ws.perf_rates, ws.current)


class WefacOracleModel(CoupledOracleModel):
    def __init__(self, grid, tables, params, wells, well_state, efficiency, dbhp_max_rel=1.0):
        super().__init__(grid, tables, params, wells, well_state, dbhp_max_rel=dbhp_max_rel)
        e = np.asarray(efficiency, float)
        assert e.shape == (self.nw,) and np.isfinite(e).all() and (e > 0).all() and (e <= 1).all()
        self.eff = e
        self.eff_perf = e[self.perf_well]

    def assemble(self, initial):
        self.update_well_controls()
        if initial:
            self.acc0 = None
        self.r, self.val, self.acc0, self.binv = orc.assemble(self.grid, self.tab, self.dt, self.st, self.rowptr, self.col, scale=(1.0, 1.0, 1.0), accum0=self.acc0)
        if initial:
            self.compute_connection_pressures()
        vals, ders = self.perf_props(self.st)
        self.B_avg = self.binv.reshape(3, self.nc).mean(1)
        if initial and self.prm.solve_welleq_initially:
            self.presolve_converged = self.solve_well_eq(vals, self.B_avg)
        self.E, cq_s, self.alive, self.dE_dy, self.dcq_dy, self.dE_dx, self.dcq_dx = self.linearise(vals, ders, self.ws.bhp, self.ws.qs)
        self._store_perf(cq_s)                                # perfPhaseRates: the well's own rates, unweighted
        for a in range(3):                                    # material_balance_eq[phase] -= efficiency_factors * cq_s[phase]
            np.add.at(self.r, a * self.nc + self.cells, -(self.eff_perf * cq_s[:, a].real))

    def solveJacobianSystem(self):
        nc, nw = self.nc, self.nw
        n = 3 * nc + 4 * nw
        A = sp.bsr_matrix((self.val.reshape(-1, 3, 3), self.col, self.rowptr), shape=(3 * nc, 3 * nc)).tocoo()
        rr, cc, dd = [], [], []

        def block(r0, c0, m):
            m = np.asarray(m)
            for a in range(m.shape[0]):
                for v in range(m.shape[1]):
                    rr.append(r0 + a); cc.append(c0 + v); dd.append(m[a, v])

        for (i, j), m in self.dcq_dx.items():                 # reservoir rows of cell i, variables of cell j: -e_w d cq_s / dx
            block(3 * self.cells[i], 3 * self.cells[j], -(self.eff_perf[i] * m))
        for j in range(self.nperf):
            w = self.perf_well[j]
            block(3 * self.cells[j], 3 * nc + 4 * w, -(self.eff_perf[j] * self.dcq_dy[j]))      # reservoir rows, well columns: weighted
            block(3 * nc + 4 * w, 3 * self.cells[j], self.dE_dx[j])                             # well rows: as they are
        for w in range(nw):
            block(3 * nc + 4 * w, 3 * nc + 4 * w, self.dE_dy[w])
        rows = np.concatenate([A.row, np.asarray(rr)])
        cols = np.concatenate([A.col, np.asarray(cc)])
        data = np.concatenate([A.data, np.asarray(dd, float)])
        J = sp.coo_matrix((data, (rows, cols)), shape=(n, n)).tocsc()
        rhs = np.concatenate([np.ascontiguousarray(self.r.reshape(3, nc).T).ravel(), self.E.ravel()])
        d = spla.spsolve(J, rhs)
        if not np.isfinite(d).all():
            raise NumericalIssue("the direct solve of the coupled system failed")
        self.dx = np.ascontiguousarray(d[:3 * nc].reshape(nc, 3).T).ravel()
        self.dy = d[3 * nc:].reshape(nw, 4)
        return self.dx
