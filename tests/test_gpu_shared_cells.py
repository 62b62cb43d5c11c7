"""GPU: several wells in one cell on the device well path (include/opmgpu.h, the device-well block: any number of DIFFERENT wells may perforate
a cell, their terms are summed in ascending perforation index).  The decks are those of tests/shared_cell_decks.py; the references are the
host well model (opmgpu/wells.py) on the CPU oracle with its explicit clique matrix -- which sums into a shared cell with np.add.at, in the
same order -- and the float64 restatement of the pressure stage (tests/amg_reference.py).

  A  two Newton iterations in lockstep with the oracle (util.lockstep_parity) on TWIN, CROSS and MANY49, ILU0 and CPR, BiCGStab and GMRES, at
     the walker's own tolerances; TWIN once more with the float Jacobian and the float CPR solve
  B  the columns of the coupled operator at every shared cell (unit vectors: a lost P t term cannot hide behind a well-conditioned row)
  C  the Newton increment of the first assembly against the oracle's (a lost B D^-1 E term of rhs_extra moves it by orders of magnitude more
     than the bound)
  D  two fresh contexts give the same bits (residual, Jacobian, operator, increment)
  E  the three forms of the pre-solve agree bit for bit
  F  the bordered pressure stage on TWIN: one border column per (cell, well) pair, Galerkin products, coarsest inverse and one V-cycle against
     the restatement; the inner Krylov method on A_p (k_ell_spmv)
  G  what stays refused, and opmgpu_well_shared_cells
  H  tests/golden/decks/WAG_TWIN.DATA, device run against oracle run

Every case fails on a library that refuses a cell perforated twice (opmgpu_set_device_wells returned OPMGPU_EINVAL)."""
import os

import numpy as np
import pytest

import amg_reference as ar
import shared_cell_decks as S
import well_size_decks as D
from opmgpu import capi, decks, eclio, partition, wells as W
from opmgpu.model import GpuBlackoilModel
from util import OracleBackend, lockstep_parity, rel_err

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WAG_DECK = os.path.join(HERE, "golden", "decks", "WAG_TWIN.DATA")
EPS64 = np.finfo(np.float64).eps
# tests/test_gpu_cpr_stages.py: relative 2-norm tolerance of a double V-cycle against the restatement
CYCLE_TOL = 1e-12
# util.lockstep_parity's defaults
TOL_OP, TOL_P, TOL_S = 1e-9, 1e-6, 1e-6


# ---------------------------------------------------------------- A
LOCKSTEP = [(n, c, g) for n in ("twin", "cross", "many49") for c, g in ((0, 0), (1, 0), (1, 1))] + [("twin", 0, 1)]


@pytest.mark.parametrize("name,cpr,gmres", LOCKSTEP, ids=["%s-cpr%d-gmres%d" % c for c in LOCKSTEP])
def test_lockstep_parity_with_shared_cells(gpu_lib, oracle, name, cpr, gmres):
    """Residual, off-diagonal Jacobian, coupled operator against the explicit clique matrix, convergence scalars, pre-solve count, controls,
    well and reservoir state of two Newton iterations, at the walker's own tolerances."""
    deck = S.DECKS[name]()
    lockstep_parity(gpu_lib, oracle, deck.grid, deck.tab, deck.st, deck.dt, deck.wl, niter=2, cpr=cpr, gmres=gmres)


def test_lockstep_parity_of_twin_in_float(gpu_lib, oracle):
    """TWIN with the float Jacobian and the float CPR solve (k_well_shared_rows<float>), at the tolerances of test_gpu_fullsize's cart100_f32"""
    from test_gpu_fullsize import TIMED_KW
    deck = S.twin_deck()
    lockstep_parity(gpu_lib, oracle, deck.grid, deck.tab, deck.st, deck.dt, deck.wl, niter=2, **TIMED_KW["cart100_f32"][1])


# ---------------------------------------------------------------- shared references
def _device_first_assembly(deck, **params):
    gm = GpuBlackoilModel(deck.grid, deck.tab, capi.default_params(**params))
    md = W.DeviceWellModel(gm, deck.wl, W.WellState(deck.wl, deck.st.p))
    md.prepareStep(deck.dt, deck.st)
    gm.setSolvePrecision(False)
    gm.assemble(True)
    return gm, md


@pytest.fixture(scope="module")
def twin_oracle(oracle):
    """the host well model on the oracle through TWIN's first assembly and its Newton increment at a 1e-12 reduction; computed once, read only"""
    deck = S.twin_deck()
    oracle.set_threads(16)
    mo = D.host_model(oracle, deck, reduction=1e-12)
    mo.prepareStep(deck.dt, deck.st)
    mo.assemble(True)
    dx = mo.m.solveJacobianSystem(single_precision=False).copy()
    return deck, mo, dx


# ---------------------------------------------------------------- B
def test_operator_columns_at_every_shared_cell(gpu_lib, oracle, twin_oracle):
    """gm.spmv on the three unit vectors of each shared cell against the same columns of the oracle's clique matrix, at the walker's tol_op"""
    deck, mo, _ = twin_oracle
    ob, nc = mo.m, deck.grid.nc
    gm, md = _device_first_assembly(deck)
    worst = 0.0
    for cell in S.shared_cell_list(deck.wl):
        for v in range(3):
            x = np.zeros(3 * nc)
            x[3 * cell + v] = 1.0
            yo = oracle.spmv(ob.rowptr, ob.col, ob.val, x)
            yg = gm.spmv(x)
            e = rel_err(yg, yo)
            worst = max(worst, e)
            assert e < TOL_OP, (cell, v, e)
            # the column's entries in the shared cell's own rows (where a lost term would sit), one by one
            own = slice(3 * cell, 3 * cell + 3)
            assert np.abs(yg[own] - yo[own]).max() <= TOL_OP * np.abs(yo[own]).max(), (cell, v)
    print("columns of the coupled operator at %d shared cells: worst %.1e" % (len(S.shared_cell_list(deck.wl)), worst))
    gm.close()


# ---------------------------------------------------------------- C
def test_newton_increment_of_the_first_assembly(gpu_lib, oracle, twin_oracle):
    """rhs_extra = -sum_w e_w B D^-1 E on the shared rows: the device increment from a solve at 1e-11 against the oracle's at 1e-7 relative per
    unknown type, the bound test_gpu_well_sizes.test_woodbury_correction_leaves_the_newton_increment uses"""
    deck, mo, dxo = twin_oracle
    nc = deck.grid.nc
    gm, md = _device_first_assembly(deck, **dict(capi.CPR_AMG_VCYCLE, linear_solver_reduction=1e-11, linear_solver_maxiter=2000))
    assert rel_err(gm.residual(), mo.m.r) < 1e-11
    gm.getConvergence()
    md.wellConvergence()
    dx = np.asarray(gm.solveJacobianSystem(want_dx=True, single_precision=False))
    assert gm.linear_reduction <= 1e-11
    gm.close()
    for a in range(3):
        blk = slice(a * nc, (a + 1) * nc)
        e = np.abs(dx[blk] - dxo[blk]).max() / np.abs(dxo[blk]).max()
        print("increment, unknown %d: %.1e relative" % (a, e))
        assert e <= 1e-7, (a, e)


# ---------------------------------------------------------------- D
def test_two_fresh_contexts_give_the_same_bits(gpu_lib):
    deck = S.twin_deck()
    x = np.random.default_rng(3).standard_normal(3 * deck.grid.nc) * np.tile([1e5, 1e-2, 1e-2], deck.grid.nc)
    out = []
    for _ in range(2):
        gm, md = _device_first_assembly(deck, **dict(capi.CPR_AMG_VCYCLE, newton_use_gmres=1, linear_solver_reduction=1e-10, linear_solver_maxiter=400))
        r, val, y = gm.residual(), gm.jacobian()[2], gm.spmv(x)
        gm.getConvergence()
        md.wellConvergence()
        dx = np.asarray(gm.solveJacobianSystem(want_dx=True, single_precision=False))
        out.append((r, val, y, dx))
        gm.close()
    for name, a, b in zip(("residual", "Jacobian", "spmv", "increment"), *out):
        assert np.array_equal(a, b), name


# ---------------------------------------------------------------- E
@pytest.mark.parametrize("name", ["twin", "cross"])
def test_presolve_forms_agree_with_shared_cells(gpu_lib, oracle, monkeypatch, name):
    """OPMGPU_WELL_PRESOLVE_FUSED unset / 1 / 0 / 2, as test_gpu_well_sizes.test_presolve_forms_agree_past_the_fixed_sizes runs them: the
    host's iteration count and the same controls, well state and reservoir state bit for bit"""
    from test_gpu_well_sizes import _host_first_assembly, _presolve_run
    deck = S.DECKS[name]()
    host_its = _host_first_assembly(oracle, deck).wh.well_iterations
    assert host_its >= 2
    modes = (None, "1", "0", "2")
    out = {m: _presolve_run(deck, monkeypatch, m) for m in modes}
    a = out[modes[0]]
    assert a[0] == host_its, (a[0], host_its)
    for m in modes[1:]:
        b = out[m]
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), (m, a[0], b[0])
        assert all(np.array_equal(x, y) for x, y in zip(a[2:6], b[2:6])), m
        assert np.array_equal(a[6].p, b[6].p) and np.array_equal(a[6].sat, b[6].sat), m


# ---------------------------------------------------------------- F
def _weights(gm, nb):
    w = np.zeros(3 * nb)
    gm._status(gm.lib.opmgpu_get_cpr_weights(gm.ctx, capi.dptr(w)))
    return w.reshape(3, nb)


def _rel2(a, b):
    m = np.abs(b).max()
    return np.linalg.norm((a - b) / m) / np.linalg.norm(b / m)


def test_bordered_pressure_stage_with_shared_cells(gpu_lib):
    """TWIN's hierarchy after a CPR solve, with the bounds tests/test_gpu_cpr_stages.check_hierarchy holds a double hierarchy to (that function
    asserts that no cell is perforated twice, so what is needed of it is restated here from tests/amg_reference.py)."""
    deck = S.twin_deck()
    wl, nc = deck.wl, deck.grid.nc
    gm = GpuBlackoilModel(deck.grid, deck.tab, capi.default_params(**dict(capi.CPR_AMG_VCYCLE, linear_solver_reduction=1e-6, linear_solver_maxiter=300)))
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, deck.st.p))
    md.prepareStep(deck.dt, deck.st)
    _, lin = md.nonlinearIteration(0, single_precision=False)
    rowptr, col, val9 = gm.jacobian()
    n, nnz, nwb = gm.cpr_levels()
    print("twin: %d border wells, levels %s, %d linear iterations to 1e-6" % (nwb, list(n), lin))
    assert nwb == wl.nw and n[0] == nc + wl.nw
    nl = len(n)
    levels = [gm.cpr_level(l) for l in range(nl)]
    assert all(np.diff(lv[0]).min() >= 1 for lv in levels)
    A = [ar.csr(*levels[l][:3], n[l]) for l in range(nl)]
    aggs = [levels[l][3] for l in range(nl - 1)]
    # ---- level 0: the pressure matrix of the system, then the border: one column per (cell, well) pair
    w = _weights(gm, nc)
    Ap = ar.pressure_matrix(rowptr, col, val9, w)
    dif = abs(A[0][:nc, :nc] - Ap) - 1e-15 * ar.pressure_matrix(rowptr, col, np.abs(val9), np.abs(w))
    assert (dif.max() if dif.nnz else 0.0) <= 0.0
    rp, cl = levels[0][0], levels[0][1]
    rows_of_entry = np.repeat(np.arange(n[0]), np.diff(rp))
    for cell in range(nc):
        border = cl[rp[cell]:rp[cell + 1]]
        border = border[border >= nc]
        assert (border - nc).tolist() == S.wells_of_cell(wl, cell), (cell, border)          # ascending perforation index = ascending well here
    for cell in S.shared_cell_list(wl):
        assert rp[cell + 1] - rp[cell] == rowptr[cell + 1] - rowptr[cell] + len(S.wells_of_cell(wl, cell)) and len(S.wells_of_cell(wl, cell)) >= 2
        assert (A[0][cell, nc + np.asarray(S.wells_of_cell(wl, cell))].toarray() != 0).all(), cell          # the cell sees every well's pressure
    for k in range(wl.nw):
        cols = cl[rp[nc + k]:rp[nc + k + 1]]
        cells = sorted(wl.cells[wl.connpos[k]:wl.connpos[k + 1]])
        assert sorted(cols[cols < nc].tolist()) == cells and set(cols[cols >= nc]) == {nc + k}, k          # each well row holds its cells
        rows = rows_of_entry[cl == nc + k]
        assert sorted(rows[rows < nc].tolist()) == cells and set(rows[rows >= nc]) == {nc + k}, k
    assert nnz[0] == rp[-1]
    # ---- aggregation: the well rows stay singletons, at the end
    for l, agg in enumerate(aggs):
        assert agg.min() >= 0 and agg.max() == n[l + 1] - 1 and np.bincount(agg, minlength=n[l + 1]).min() >= 1, l
        wr = agg[n[l] - nwb:]
        assert np.array_equal(wr, np.arange(n[l + 1] - nwb, n[l + 1])) and np.bincount(agg, minlength=n[l + 1])[wr].max() == 1, l
    # ---- Galerkin, level by level
    for l, agg in enumerate(aggs):
        P = ar.prolongation(agg, n[l + 1])
        ref = (P.T @ A[l] @ P).tocsr()
        d = abs(A[l + 1] - ref) - 1e-14 * (P.T @ abs(A[l]) @ P)
        assert (d.max() if d.nnz else 0.0) <= 0.0, l
    # ---- dense inverse of the coarsest level
    inv = levels[-1][4]
    assert n[-1] <= ar.DENSE_MAX and inv is not None
    Ac = A[-1].toarray()
    ref = np.linalg.inv(Ac)
    assert np.abs(inv - ref).max() <= n[-1] * EPS64 * np.linalg.cond(Ac, np.inf) * np.abs(ref).max()
    # ---- one V-cycle, restated from level 0 and the aggregates
    pd0, pd = gm.cpr_correction_factors()
    H = ar.Hierarchy(A[0], aggs)
    kw = dict(pdamp0=pd0, pdamp=pd, npost0=2, gs_first=None, npre=1)
    rng = np.random.default_rng(11)
    s = rng.standard_normal(n[0])
    Dinv = ar.inv_diag(A[0])
    for _ in range(10):
        s = s - 0.9 * Dinv * (A[0] @ s)
    shared_unit = np.zeros(n[0])
    shared_unit[S.shared_cell_list(wl)] = 1.0          # excites the shared rows' border columns alone
    for name, b in (("random", rng.standard_normal(n[0])), ("smooth", A[0] @ s), ("shared cells", shared_unit)):
        x = gm.cpr_vcycle_apply(b)
        e = _rel2(x, H.vcycle(b, **kw))
        print("twin %s: cycle %.2e" % (name, e))
        assert e <= CYCLE_TOL, (name, e)
        # the tolerance has teeth on the new ground: the restatement without ONE border column of a shared cell lies far outside it
        cell = int(S.shared_cell_list(wl)[0])
        lost = A[0].tolil(copy=True)
        lost[cell, nc + S.wells_of_cell(wl, cell)[-1]] = 0.0
        xc = ar.Hierarchy(lost.tocsr(), aggs).vcycle(b, **kw)
        assert _rel2(x, xc) >= 100 * CYCLE_TOL, (name, _rel2(x, xc))
    gm.close()


def test_inner_krylov_method_on_the_bordered_level0(gpu_lib, oracle):
    """cpr_use_amg = 0, cpr_max_ell_iter = 25: the elliptic part is an inner BiCGStab on the bordered A_p itself (k_ell_spmv walks the shared
    rows' border columns).  One Newton iteration of TWIN: the solve reaches its reduction, and the state after the update agrees with the
    oracle's at the walker's tolerances."""
    deck = S.twin_deck()
    wl = deck.wl
    red = 1e-10
    gm = GpuBlackoilModel(deck.grid, deck.tab, capi.default_params(use_cpr=1, cpr_use_amg=0, cpr_max_ell_iter=25, linear_solver_reduction=red, linear_solver_maxiter=2000))
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, deck.st.p))
    md.prepareStep(deck.dt, deck.st)
    gm.setSolvePrecision(False)
    gm.assemble(True)
    gm.getConvergence()
    md.wellConvergence()
    gm.solveJacobianSystem(single_precision=False)
    print("inner Krylov method: %d outer iterations, reduction %.1e" % (gm.linear_iterations, gm.linear_reduction))
    assert gm.linear_reduction <= red
    assert gm.cpr_levels()[2] == wl.nw
    gm.updateState()
    a = gm.getState()
    ws = md.pull_well_state()
    gm.close()
    mo = D.host_model(oracle, deck, reduction=red)
    mo.prepareStep(deck.dt, deck.st)
    mo.assemble(True)
    ob = mo.m
    ob.solveJacobianSystem(single_precision=False)
    mo.wh.recover_and_update(ob.perfDx(wl.nperf), mo.ws)
    ob.updateState()
    b = ob.getState()
    assert np.array_equal(a.hc, b.hc)
    assert np.abs(a.p - b.p).max() <= TOL_P * np.abs(b.p).max() and np.abs(a.sat - b.sat).max() <= TOL_S
    assert np.abs(a.rs - b.rs).max() <= 1e-5 * max(np.abs(b.rs).max(), 1.0) and np.abs(a.rv - b.rv).max() <= 1e-5 * max(np.abs(b.rv).max(), 1e-3)
    assert np.allclose(ws.bhp, mo.ws.bhp, rtol=1e-6) and np.allclose(ws.qs, mo.ws.qs, rtol=1e-5, atol=1e-8 * np.abs(mo.ws.qs).max())
    assert np.array_equal(ws.current, mo.ws.current)


# ---------------------------------------------------------------- G
def test_one_well_naming_a_cell_twice_is_refused(gpu_lib):
    deck, well, cell = S.within_deck()
    gm = GpuBlackoilModel(deck.grid, deck.tab, capi.default_params())
    with pytest.raises(ValueError) as ei:
        W.DeviceWellModel(gm, deck.wl, W.WellState(deck.wl, deck.st.p))
    msg = gpu_lib.opmgpu_last_error(gm.ctx).decode()
    print(msg)
    assert "well %d" % well in msg and "cell %d" % cell in msg and "twice" in msg and msg in str(ei.value)
    rows, most = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert gpu_lib.opmgpu_well_shared_cells(gm.ctx, capi.iptr(rows), capi.iptr(most)) == capi.EINVAL          # no device wells were set
    gm.close()


def test_shared_cells_are_refused_in_a_decomposed_context(gpu_lib, monkeypatch):
    """TWIN on a context with a communicator attached (the shared-memory test transport, one rank with one isolated ghost copy of cell 0):
    refused with the decomposed-run text, in whichever order the two calls come"""
    monkeypatch.setenv("OPMGPU_COMM_TRANSPORT", "shm")
    deck = S.twin_deck()
    g, st, nc = deck.grid, deck.st, deck.grid.nc
    src = np.concatenate([np.arange(nc), [0]])
    grid_b = decks.GridData(nc + 1, g.conn_cells, g.trans, g.pv[src], g.z[src])

    class Dom:
        n_owned, neigh_rank, send_ptr, send_cells = nc, capi.i32([0]), capi.i32([0, 1]), capi.i32([0])
        recv_ptr, recv_cells = capi.i32([0, 1]), capi.i32([nc])

    gm = GpuBlackoilModel(grid_b, deck.tab, capi.default_params())
    partition.attach_comm(gm, Dom, 0, 1, partition.make_unique_id())
    with pytest.raises(ValueError, match="decomposed run"):
        W.DeviceWellModel(gm, deck.wl, W.WellState(deck.wl, st.p))
    assert "perforated by several wells" in gpu_lib.opmgpu_last_error(gm.ctx).decode()
    gm.close()
    gm = GpuBlackoilModel(grid_b, deck.tab, capi.default_params())
    W.DeviceWellModel(gm, deck.wl, W.WellState(deck.wl, st.p))
    with pytest.raises(Exception, match="decomposed run"):
        partition.attach_comm(gm, Dom, 0, 1, partition.make_unique_id())
    gm.close()


def test_shared_cell_query(gpu_lib):
    for deck, want in ((D.long_deck(), (0, 0)), (S.twin_deck(), S.TWIN_SHARED), (S.cross_deck(), S.CROSS_SHARED)):
        gm = GpuBlackoilModel(deck.grid, deck.tab, capi.default_params())
        md = W.DeviceWellModel(gm, deck.wl, W.WellState(deck.wl, deck.st.p))
        assert gm.wellSharedCells() == md.shared_cells() == want == S.shared_cells(deck.wl), deck.name
        assert gpu_lib.opmgpu_well_shared_cells(gm.ctx, None, None) == capi.OK
        gm.close()


# ---------------------------------------------------------------- H
def test_wag_twin_deck_device_run_against_oracle_run(gpu_lib, oracle, tmp_path):
    """WAG_TWIN.DATA as tests/test_gpu_simulator.py::test_device_run_against_oracle_run_with_the_regression_tolerances runs SCHEDULE_SMALL:
    the device path (CPR, device well model) and the CPU oracle with the host well model, both solving tightly; the same sub-step and Newton
    counts, and the output files agree at compareECL's strict pair of tolerances (abs 2e-2, rel 1e-5)."""
    from opmgpu.simulator import Simulator
    tight = dict(linear_solver_reduction=1e-9, linear_solver_maxiter=600, tolerance_wells=1e-7)
    base_d, base_o = str(tmp_path / "DEV"), str(tmp_path / "ORC")
    sim = Simulator(WAG_DECK, params=capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, **tight), output_base=base_d)
    sim.model.max_single_precision_days = 0.0            # double solves on the device too
    rd = sim.run()
    assert sim.model.wellSharedCells() == (3, 2)
    sim.close()

    def oracle_model(grid, tables, params):
        return OracleBackend(oracle, grid, tables, params)

    def host_wells(model, wl, ws):
        if model.wells is None or list(model.wells[1]) != list(wl.arrays()[1]):      # the pattern carries the wells' cliques
            model.wells = wl.arrays()
            model.rowptr, model.col = oracle.pattern(model.grid, *model.wells)
        return W.WellCoupledModel(model, W.StandardWellsHost(wl, model.grid.z, model.tab.surface_density[0], tolerance_wells=1e-7), ws)

    so = Simulator(WAG_DECK, params=capi.default_params(**tight), output_base=base_o, model_factory=oracle_model, well_model_factory=host_wells)
    ro = so.run()
    print("device sub-steps %s newton %s; oracle sub-steps %s newton %s" % ([r["substeps"] for r in rd], [r["newton"] for r in rd], [r["substeps"] for r in ro], [r["newton"] for r in ro]))
    assert [r["days"] for r in rd] == [r["days"] for r in ro] == [10.0, 20.0, 40.0]
    assert [r["substeps"] for r in rd] == [r["substeps"] for r in ro] and [r["newton"] for r in rd] == [r["newton"] for r in ro]
    bad = eclio.compare(base_d, base_o, abs_tol=2e-2, rel_tol=1e-5)
    assert not bad, bad
