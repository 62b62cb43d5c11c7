"""Shared helpers for the parity tests."""
import numpy as np
import scipy.sparse as sp


def bsr_to_scipy(rowptr, col, val9):
    nb = rowptr.size - 1
    return sp.bsr_matrix((np.asarray(val9).reshape(-1, 3, 3), col, rowptr), shape=(3 * nb, 3 * nb)).tocsr()


def eqmajor_to_interleaved(v, nc):
    return np.ascontiguousarray(np.asarray(v).reshape(3, nc).T).ravel()


def interleaved_to_eqmajor(v, nc):
    return np.ascontiguousarray(np.asarray(v).reshape(nc, 3).T).ravel()


def random_block_matrix(rowptr, col, seed=1, dominance=6.0):
    """SURVEY 8d 'SpMV micro': blocks = I*(dominance+u) on the diagonal, -0.3*u off it."""
    rng = np.random.default_rng(seed)
    nb = rowptr.size - 1
    val = -0.3 * rng.random((col.size, 9))
    rows = np.repeat(np.arange(nb), np.diff(rowptr))
    d = np.flatnonzero(rows == col)
    val[d] = 0.3 * rng.random((d.size, 9))
    val[d, 0] += dominance + rng.random(d.size); val[d, 4] += dominance + rng.random(d.size); val[d, 8] += dominance + rng.random(d.size)
    return val


def rel_err(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(np.asarray(b)).max() + 1e-300)


def slot_err(a, b):
    """rel_err slot by slot: the largest, over the nine (equation, variable) slots of a block Jacobian [nnzb][9] -- or the three equations of
    an equation-major residual [3 * nc] --, of max |a - b| / max |b| WITHIN the slot.  One max-norm over all entries (rel_err) is set by the
    largest slot: the d/dX entries are ~1e10 times the d/dp ones, so at 1e-11 the whole pressure column may be several per cent off
    (DESIGN section 7a).  A slot that is identically zero in b must be so in a."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim == 1:
        a, b = a.reshape(3, -1).T, b.reshape(3, -1).T
    d, s = np.abs(a - b).max(0), np.abs(b).max(0)
    return float(np.where(s > 0, d / np.where(s > 0, s, 1.0), np.where(d > 0, np.inf, 0.0)).max())


class OracleBackend:
    """The GpuBlackoilModel interface on top of the CPU oracle (checker side of the well-coupled parity tests)."""

    def __init__(self, orc, grid, tables, params, wells=None):
        from opmgpu import capi
        self.orc, self.grid, self.tab, self.prm = orc, grid, tables, params
        self.scale = np.asarray(params.matbalscale[:])
        self.wells = wells
        self.rowptr, self.col = orc.pattern(grid, *(wells or (None, None)))
        self.nc = grid.nc
        self.position = None
        self.linear_iterations = 0
        self.capi = capi

    def prepareStep(self, dt, state=None):
        self.dt = float(dt)
        if state is not None:
            self.st = state.copy()
        self.acc0 = None

    def assemble(self, initial):
        if initial:
            self.acc0 = None
            self.dx_old = None
        self.r, self.val, self.acc0, self.binv = self.orc.assemble(self.grid, self.tab, self.dt, self.st, self.rowptr, self.col,
                                                                   scale=tuple(self.scale), accum0=self.acc0)
        self.rhs_extra = np.zeros(3 * self.nc)

    def computeFluidInPlace(self, fipnum=None, cells=False):
        """numpy restatement of BlackoilModelBase::computeFluidInPlace (BlackoilModelBase_impl.hpp:2263-2366) on the oracle's cell properties"""
        import numpy as np
        st, nc = self.st, self.grid.nc
        props = self.orc.cell_props(self.grid, self.tab, st)
        nm = self.orc.PROP_NAMES
        assert self.tab.rocktab_n == 0
        cp = self.tab.rock_comp * (st.p - self.tab.rock_pref)
        pvm = 1.0 + cp + 0.5 * cp * cp
        pv = np.asarray(self.grid.pv)
        fip = np.zeros((7, nc))
        for a, ph in enumerate("wog"):
            fip[a] = ((pvm * props[:, nm.index("b_" + ph), 0]) * st.sat[:, a]) * pv
        fip[3], fip[4] = st.rs * fip[1], st.rv * fip[2]
        fn = np.ones(nc, np.int32) if fipnum is None else np.asarray(fipnum, np.int32)
        dims = max(1, int(fn.max()))
        values, hcpv, pres = np.zeros((dims, 7)), np.zeros(dims), np.zeros(dims)
        hyd = st.sat[:, 1] + st.sat[:, 2]
        for c in range(nc):
            r = fn[c] - 1
            if r != -1:
                values[r, :5] += fip[:5, c]; hcpv[r] += pv[c] * hyd[c]; pres[r] += pv[c] * st.p[c]
        for c in range(nc):
            r = fn[c] - 1
            if r != -1:
                fip[5, c] = pv[c]
                fip[6, c] = pv[c] * st.p[c] * hyd[c] / hcpv[r] if hcpv[r] != 0 else pres[r] / pv[c]
                values[r, 5] += fip[5, c]; values[r, 6] += fip[6, c]
        return (values, fip) if cells else values

    def perfProps(self, nperf):
        props = self.orc.cell_props(self.grid, self.tab, self.st)[self.wells[1]]
        names = self.orc.PROP_NAMES
        idx = [names.index(n) for n in ["p_o", "rs", "rv", "b_w", "b_o", "b_g", "mob_w", "mob_o", "mob_g"]]
        return props[:, idx, :].reshape(nperf, 36)

    def averageB(self):
        """B_avg of getWellConvergence (BlackoilModelBase_impl.hpp:1876-1891): mean of 1/b per phase over the cells"""
        return self.binv.reshape(3, self.nc).mean(1)

    def perfPvtAt(self, press):
        """computePropertiesForWellConnectionPressures (StandardWells_impl.hpp:218-296): b_w, b_o, b_g, rsSat, rvSat of the
        perforated cells at the given pressures, with the cells' rs / rv / phase condition / oil saturation"""
        from opmgpu import capi
        cells = np.asarray(self.wells[1])
        st, t = self.st, self.tab
        pvtnum = None if self.grid.pvtnum is None else self.grid.pvtnum[cells]
        hc = st.hc[cells]
        free_gas = (hc != capi.HC_OIL_ONLY).astype(np.int8); free_oil = (hc != capi.HC_GAS_ONLY).astype(np.int8)
        if not t.has_disgas:
            free_gas[:] = 1
        if not t.has_vapoil:
            free_oil[:] = 1
        b = np.stack([self.orc.pvt(t, "bWat", press, pvtnum=pvtnum)[:, 0],
                      self.orc.pvt(t, "bOil", press, st.rs[cells], free_gas, pvtnum)[:, 0],
                      self.orc.pvt(t, "bGas", press, st.rv[cells], free_oil, pvtnum)[:, 0]], 1)
        rsmax = self.orc.pvt(t, "rsSat", press, pvtnum=pvtnum)[:, 0] if t.has_disgas else np.zeros(cells.size)
        rvmax = self.orc.pvt(t, "rvSat", press, pvtnum=pvtnum)[:, 0] if t.has_vapoil else np.zeros(cells.size)
        so, somax = st.sat[cells, 1], getattr(self, "so_max", np.zeros(self.nc))[cells]
        for vap, arr in ((t.vap2, rsmax), (t.vap1, rvmax)):          # applyVap (BlackoilPropsAdFromDeck.cpp:1052-1078)
            if vap > 0.0:
                k = (somax > 0.01) & (so < somax)
                arr[k] *= (np.maximum(so[k], 1.4901161193847656e-08) / somax[k]) ** vap
        return b, rsmax, rvmax

    def stabilizeUpdate(self, relax_type, omega):
        """NonlinearSolver::stabilizeNonlinearUpdate (NonlinearSolver_impl.hpp:260-301) on the reservoir part of dx"""
        old = getattr(self, "dx_old", None)
        if old is None or old.size != self.dx.size:
            old = np.zeros_like(self.dx)
        new = self.dx.copy()
        if omega != 1.0:
            self.dx = omega * self.dx + (1.0 - omega) * old if relax_type == 1 else omega * self.dx
        self.dx_old = new

    def addWellTerms(self, resid_delta, rc, blocks):
        nc = self.nc
        cells = np.asarray(self.wells[1])
        for a in range(3):
            np.add.at(self.r, a * nc + cells, np.asarray(resid_delta)[:, a])
        sc = np.repeat(self.scale, 3)
        rc = np.asarray(rc).reshape(-1, 2)
        # position of every (row, col) block: binary search in the row-major key list of the pattern (rows and columns ascending)
        if getattr(self, "_keys", None) is None:
            rows = np.repeat(np.arange(nc, dtype=np.int64), np.diff(self.rowptr))
            self._keys = rows * nc + self.col
        pos = np.searchsorted(self._keys, rc[:, 0].astype(np.int64) * nc + rc[:, 1])
        assert np.array_equal(self._keys[pos], rc[:, 0].astype(np.int64) * nc + rc[:, 1])
        np.add.at(self.val, pos, np.asarray(blocks) * sc)

    def addWellRhs(self, rhs_delta):
        nc = self.nc
        cells = np.asarray(self.wells[1])
        for a in range(3):
            np.add.at(self.rhs_extra, a * nc + cells, np.asarray(rhs_delta)[:, a])

    def getConvergence(self):
        st, self.B_avg, self.CNV, self.MB, self.linf, conv = self.orc.convergence(self.grid, self.prm, self.dt, self.r, self.binv)
        assert st == 0
        return conv

    def solveJacobianSystem(self, want_dx=False, single_precision=False):
        nc = self.nc
        b = np.ascontiguousarray(((self.r + self.rhs_extra) * np.repeat(self.scale, nc)).reshape(3, nc).T).ravel()
        sto, x, it, red, _ = self.orc.bicgstab(self.rowptr, self.col, self.val, b, self.prm, position=self.position, single=bool(single_precision))
        assert sto == 0, sto
        self.linear_iterations = it
        self.dx = np.ascontiguousarray(x.reshape(nc, 3).T).ravel()
        return self.dx

    def perfDx(self, nperf):
        nc = self.nc
        return np.stack([self.dx[a * nc + self.wells[1]] for a in range(3)], 1)

    def updateState(self):
        self.st = self.orc.update_state(self.grid, self.tab, self.prm, self.dx, self.st)

    def getState(self):
        return self.st

    # last_state of AdaptiveTimeStepping and BlackoilModelBase::relativeChange (BlackoilModelBase_impl.hpp:1595-1631)
    def saveState(self):
        self.saved = self.st.copy()

    def restoreState(self):
        self.st = self.saved.copy()

    def relativeChange(self):
        a, b = self.saved, self.st
        num = ((a.p - b.p) ** 2).sum() + ((a.sat - b.sat) ** 2).sum()
        den = (b.p ** 2).sum() + (b.sat ** 2).sum()
        return num / den if den > 0 else 0.0


# ------------------------------------------------------------------------------------------------------------------------
# lockstep walker: device run against oracle run, iteration by iteration (test_gpu_fullsize.py, test_gpu_well_sizes.py)
# ------------------------------------------------------------------------------------------------------------------------
def perforated_diag_mask(rowptr, col, cells):
    """blocks (c, c) of the perforated cells: the only Jacobian entries the device well model changes in the matrix itself"""
    nb = rowptr.size - 1
    rows = np.repeat(np.arange(nb, dtype=np.int64), np.diff(rowptr))
    perf = np.zeros(nb, bool); perf[np.asarray(cells, int)] = True
    return (rows == col) & perf[rows]


def lockstep_parity(gpu_lib, oracle, grid, tab, st, dt, wl, niter=2, cpr=1, reduction=1e-10, maxiter=2000, tol_p=1e-6, tol_s=1e-6,
                     single=False, gmres=0, verify=0, oracle_reduction=None, tol_jac=1e-11, tol_op=1e-9, stage2_relax=1.0):
    """Newton iterations 0..niter-1 of one time step, GPU (device wells, CPR or ILU0) and oracle (+ host well model with
    the explicit Schur complement) side by side.  Every assembly is compared at rounding level; after every update the two states are
    compared at the linear tolerance and the oracle then CONTINUES FROM THE GPU's state, so the next assembly is again a rounding-level
    comparison (a free-running comparison is test_*_newton_count below).

    single / gmres / verify select the configurations bench.py TIMES: restarted GMRES(40) (newton_use_gmres) under CPR in double -- the
    headline --, and the float variant (the Jacobian written as float, the float CPR solve, GMRES with the true-residual check).  The
    oracle side stays the f64 reference solve (ILU0 + BiCGStab) at `oracle_reduction`, the residual (always f64) stays a rounding-level
    comparison, a float Jacobian / operator are compared at float rounding level (tol_jac / tol_op)."""
    import pytest
    from opmgpu import capi, wells as W
    from opmgpu.model import GpuBlackoilModel
    oracle.set_threads(16)
    prm_g = capi.default_params(linear_solver_reduction=reduction, linear_solver_maxiter=maxiter, cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=cpr, newton_use_gmres=gmres, gmres_verify_residual=verify,
                                cpr_stage2_relax=stage2_relax)
    prm_o = capi.default_params(linear_solver_reduction=oracle_reduction or reduction, linear_solver_maxiter=4 * maxiter)
    nc = grid.nc
    gm = GpuBlackoilModel(grid, tab, prm_g)
    rowptr0, col0 = oracle.pattern(grid)
    scale = np.asarray(prm_g.matbalscale[:])
    if wl is not None:
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
        ob = OracleBackend(oracle, grid, tab, prm_o, wells=wl.arrays())
        mo = W.WellCoupledModel(ob, W.StandardWellsHost(wl, grid.z, tab.surface_density[0]), W.WellState(wl, st.p))
        diag_perf = perforated_diag_mask(rowptr0, col0, wl.cells)
    else:
        md, ob = gm, OracleBackend(oracle, grid, tab, prm_o)
        mo = ob
    md.prepareStep(dt, st); mo.prepareStep(dt, st)
    rng = np.random.default_rng(5)
    for it in range(niter):
        # ---- assembly ----
        gm.setSolvePrecision(single)
        gm.assemble(it == 0)
        mo.assemble(it == 0)            # with wells: control switching, reservoir, [connection pressures + well pre-solve], well terms
        val_res = None
        if wl is not None:
            # reservoir-only oracle Jacobian on the stencil pattern: everything but the perforated cells' diagonal blocks must match it
            _, val_res, _, _ = oracle.assemble(grid, tab, dt, ob.st, rowptr0, col0, scale=tuple(scale), accum0=ob.acc0)
            if it == 0:
                md.pull_well_state()
                assert md.presolve_converged and md.presolve_iterations == mo.wh.well_iterations
        gr, gc, gv = gm.jacobian()
        assert np.array_equal(gr, rowptr0) and np.array_equal(gc, col0)
        assert rel_err(gm.residual(), ob.r) < 1e-11, (it, rel_err(gm.residual(), ob.r))
        if wl is None:
            assert rel_err(gv, ob.val) < tol_jac, it
            assert slot_err(gv, ob.val) < tol_jac, (it, slot_err(gv, ob.val))
        else:
            keep = ~diag_perf
            assert rel_err(gv[keep], val_res[keep]) < tol_jac, (it, rel_err(gv[keep], val_res[keep]))
            assert slot_err(gv[keep], val_res[keep]) < tol_jac, (it, slot_err(gv[keep], val_res[keep]))
            # the coupled operator (matrix + factored rank-7 Schur complement per well) against the oracle's explicit clique matrix
            for _ in range(2):
                x3 = rng.standard_normal(3 * nc) * np.tile([1e5, 1e-2, 1e-2], nc)
                yo = oracle.spmv(ob.rowptr, ob.col, ob.val, x3)
                yg = gm.spmv(x3)
                assert rel_err(yg, yo) < tol_op, (it, rel_err(yg, yo))
        del gv, val_res
        # ---- convergence scalars ----
        cg = gm.getConvergence(); co = ob.getConvergence()
        assert np.allclose(gm.CNV, ob.CNV, rtol=1e-9) and np.allclose(gm.MB, ob.MB, rtol=1e-7, atol=1e-18) and np.allclose(gm.B_avg, ob.B_avg, rtol=1e-12)
        if wl is not None:
            cg = md.wellConvergence() and cg; co = mo.wh.converged(ob.B_avg) and co
            assert np.allclose(md.well_flux_residual, mo.wh.well_flux_residual, rtol=1e-7, atol=1e-14)
            assert md.well_ctrl_residual == pytest.approx(mo.wh.well_ctrl_residual, rel=1e-7, abs=1e-14)
        assert cg == co
        # ---- solve + update ----
        gm.solveJacobianSystem(single_precision=single)
        assert gm.linear_reduction <= reduction, (it, gm.linear_reduction)        # with gmres_verify_residual: the TRUE residual's reduction
        gm.updateState()
        ob.solveJacobianSystem(single_precision=False)
        if wl is not None:
            mo.wh.recover_and_update(ob.perfDx(wl.nperf), mo.ws)
        ob.updateState()
        a, b = gm.getState(), ob.getState()
        assert np.array_equal(a.hc, b.hc), it
        assert np.abs(a.p - b.p).max() <= tol_p * np.abs(b.p).max(), (it, np.abs(a.p - b.p).max() / np.abs(b.p).max())
        assert np.abs(a.sat - b.sat).max() <= tol_s, (it, np.abs(a.sat - b.sat).max())
        # rs / rv at a fixed 1e-5 (float: rs / rv of the undersaturated cells are unknowns of the float solve themselves).  Round 3 had widened
        # this to 10 * tol_p after the SPE10-like leg measured 0.9e-5 .. 1.9e-5 from run to run: the checker's 16-thread dot products were not
        # bit-reproducible (an OpenMP reduction clause).  They are summed in fixed blocks now (oracle.cpp dot_t), so the old gate is back.
        tol_r = 1e-5 if not single else 2.5 * tol_s
        assert np.abs(a.rs - b.rs).max() <= tol_r * max(np.abs(b.rs).max(), 1.0) and np.abs(a.rv - b.rv).max() <= tol_r * max(np.abs(b.rv).max(), 1e-3)
        ob.st = a.copy()                                 # lockstep: the oracle continues from the device state
        if wl is not None:
            ws = md.pull_well_state()
            assert np.allclose(ws.bhp, mo.ws.bhp, rtol=max(1e-6, tol_p)), (it, ws.bhp, mo.ws.bhp)
            assert np.allclose(ws.qs, mo.ws.qs, rtol=max(1e-5, 10 * tol_p), atol=max(1e-8, tol_p) * np.abs(mo.ws.qs).max()), it
            assert np.array_equal(ws.current, mo.ws.current), (it, np.flatnonzero(ws.current != mo.ws.current))
            # the perforation rates of this iteration's assembly (both sides assembled the same state), at test_gpu_wells.py's tolerance
            assert np.allclose(ws.perf_rates, mo.ws.perf_rates, rtol=1e-6, atol=1e-9 * np.abs(mo.ws.perf_rates).max()), it
            mo.ws.assign(ws)
    gm.close()
