"""The CPR pressure stage, stage by stage, against the float64 restatement of tests/amg_reference.py.

Every case solves once with CPR (one V-cycle as the elliptic stage) and then reads the hierarchy of that solve back
(opmgpu_cpr_levels / _level_get) and checks:
  * level 0 against A_p(i, j) = sum_eq w_eq(i) J_ij[eq][0] from the caller's matrix and the device's CPR weights; the well border's
    structure (one row and one column per well, non-zero at that well's cells only; its values are taken as read back);
  * the aggregation invariants (onto [0, n_{l+1}), no empty aggregate, well rows singletons on every level, the shrink ratio of setup());
  * every coarse level against P^T A_l P of the level above it, and the coarsest level's dense inverse against numpy's;
  * one V-cycle (opmgpu_cpr_vcycle_apply) on a random and on an algebraically smooth right-hand side against the restated cycle built
    from level 0 and the aggregates alone, and its linearity; on the B1 cases also the whole two-stage application (opmgpu_cpr_apply).
Each cycle tolerance comes with sensitivity controls: the restatement with omega 0.9 -> 0.905, the correction factors x 1.01 and one
Galerkin contribution dropped must lie at least 100 x the tolerance away from the device's result.

Measured maxima (MI355X) are recorded next to the tolerances below; each case prints its differences and control margins (-s).
"""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_reference as ar
from opmgpu import capi, decks, wells as W
from opmgpu.model import GpuBlackoilModel, GpuNewtonIteration

pytestmark = pytest.mark.gpu

EPS64, EPS32 = np.finfo(np.float64).eps, np.finfo(np.float32).eps
# relative 2-norm tolerances of a V-cycle / a CPR application against the restatement.  Measured on MI355X: f64 at most 8.2e-14
# (GS by colour, smooth right-hand side), f32 at most 7.0e-6 (5 760 rows, smooth right-hand side)
TOL = {False: 1e-12, True: 5e-5}
SEEN = {}          # case -> (level sizes, border wells, knobs, stored entries per level): the coverage assertion at the end


def _b1_system(oracle, nx, ny, nz, seed=0, nnc=0.02):
    """second Newton iteration of a cartesian deck (the first one is easy for any preconditioner), as the caller's BSR"""
    grid = decks.cartesian_grid(nx, ny, nz, lognormal_sigma=0.8, nnc_fraction=nnc, seed=seed)
    tab = decks.satfunc_standard_tables()
    st = decks.initial_state(grid, tab, perturb=0.004)
    prm0 = capi.default_params()
    scale = np.asarray(prm0.matbalscale[:])
    rowptr, col = oracle.pattern(grid)
    nc, dt = grid.nc, 5 * decks.DAY
    r, val, acc0, _ = oracle.assemble(grid, tab, dt, st, rowptr, col, scale=tuple(scale))
    b = np.ascontiguousarray((r * np.repeat(scale, nc)).reshape(3, nc).T).ravel()
    _, x, _, _, _ = oracle.bicgstab(rowptr, col, val, b, prm0)
    st1 = oracle.update_state(grid, tab, prm0, np.ascontiguousarray(x.reshape(nc, 3).T).ravel(), st)
    r, val, _, _ = oracle.assemble(grid, tab, dt, st1, rowptr, col, scale=tuple(scale), accum0=acc0)
    b = np.ascontiguousarray((r * np.repeat(scale, nc)).reshape(3, nc).T).ravel()
    return rowptr, col, val, b


def _weights(obj, nb):
    w = np.zeros(3 * nb)
    obj._status(obj.lib.opmgpu_get_cpr_weights(obj.ctx, capi.dptr(w)))
    return w.reshape(3, nb)


def _bsr(rowptr, col, val9):
    nb = rowptr.size - 1
    return sp.bsr_matrix((np.asarray(val9).reshape(-1, 3, 3), col, rowptr), shape=(3 * nb, 3 * nb)).tocsr()


def _rel(a, b):
    m = np.abs(b).max()          # scaled first: the squares of a float-assembled system's values can leave the double range
    return np.linalg.norm((a - b) / m) / np.linalg.norm(b / m)


def check_hierarchy(obj, rowptr, col, val9, single, case, knobs=(), npost0=2, gs_first=None, cpr=None, npre=1, pilu=None, seen=SEEN):
    """all checks of the module docstring on the hierarchy `obj` (GpuNewtonIteration or GpuBlackoilModel) holds after its solve.
    seen: where the case is recorded for test_coverage_of_the_cases (callers from other modules pass a dict of their own)"""
    nb = rowptr.size - 1
    n, nnz, nw = obj.cpr_levels()
    seen[case] = (list(n), nw, tuple(knobs), list(nnz))
    nl = len(n)
    levels = [obj.cpr_level(l) for l in range(nl)]
    A = [ar.csr(*levels[l][:3], n[l]) for l in range(nl)]
    aggs = [levels[l][3] for l in range(nl - 1)]
    assert all(np.diff(lv[0]).min() >= 1 for lv in levels)

    # ---- level 0: the pressure matrix of the caller's system, then the border
    w = _weights(obj, nb)
    Ap = ar.pressure_matrix(rowptr, col, val9, w)
    A0c = A[0][:nb, :nb]
    absw = ar.pressure_matrix(rowptr, col, np.abs(val9), np.abs(w))
    tol0 = (4 * EPS32 if single else 1e-15) * absw
    dif = abs(A0c - Ap) - tol0
    assert dif.max() <= 0.0 if dif.nnz else True, (case, abs(A0c - Ap).max())
    assert ((w == 0) | (w == 1)).all()          # 0/1 weights (formEllipticSystem)
    if nw:
        # structure as exported (a BHP-controlled well's row has zero values at its cells: d g / d q = 0), values as read back
        rp, cl = levels[0][0], levels[0][1]
        cells_of = []
        for k in range(nw):
            cols = cl[rp[nb + k]:rp[nb + k + 1]]
            cells = np.sort(cols[cols < nb])
            assert set(cols[cols >= nb]) == {nb + k}, (case, k)            # a well row couples to its own unknown only
            rows = np.repeat(np.arange(n[0]), np.diff(rp))[cl == nb + k]
            assert np.array_equal(np.sort(rows[rows < nb]), cells), (case, k)   # column and row at the same (perforated) cells
            assert set(rows[rows >= nb]) == {nb + k}
            assert (A[0][cells, nb + k].toarray() != 0).all(), (case, k)   # the cells see the well's pressure
            cells_of.append(cells)
        assert all(len(c) >= 1 for c in cells_of)
        assert len(np.unique(np.concatenate(cells_of))) == sum(len(c) for c in cells_of)   # no cell perforated twice

    # ---- aggregation invariants
    for l, agg in enumerate(aggs):
        assert agg.min() >= 0 and agg.max() == n[l + 1] - 1, (case, l)
        assert np.bincount(agg, minlength=n[l + 1]).min() >= 1, (case, l)
        assert n[l + 1] * 10 <= n[l] * 8, (case, l)                        # setup(): a level has to shrink by 0.8 at least
        if nw:
            wr = agg[n[l] - nw:]
            assert np.array_equal(wr, np.arange(n[l + 1] - nw, n[l + 1])), (case, l)      # well rows stay singletons, at the end
            assert np.bincount(agg, minlength=n[l + 1])[wr].max() == 1

    # ---- Galerkin, level by level from the device's own fine level
    for l, agg in enumerate(aggs):
        P = ar.prolongation(agg, n[l + 1])
        ref = (P.T @ A[l] @ P).tocsr()
        if single:
            # each entry is the double sum of the float fine values, rounded once
            d = (A[l + 1] - ref).tocoo()
            bound = np.spacing(np.abs(np.float32(np.asarray(ref[d.row, d.col]).ravel()))).astype(float)
            assert (np.abs(d.data) <= bound * 1.0000001).all(), (case, l, np.abs(d.data).max())
        else:
            d = abs(A[l + 1] - ref) - 1e-14 * (P.T @ abs(A[l]) @ P)
            assert (d.max() if d.nnz else 0.0) <= 0.0, (case, l)

    # ---- dense inverse of the coarsest level
    inv = levels[-1][4]
    if n[-1] <= ar.DENSE_MAX:
        assert inv is not None
        Ac = A[-1].toarray()
        ref = np.linalg.inv(Ac)
        cond = np.linalg.cond(Ac, np.inf)
        assert np.abs(inv - ref).max() <= n[-1] * EPS64 * cond * np.abs(ref).max(), (case, np.abs(inv - ref).max() / np.abs(ref).max(), cond)

    # ---- one V-cycle, restated from level 0 and the aggregates
    pd0, pd = obj.cpr_correction_factors()
    H = ar.Hierarchy(A[0], aggs)
    kw = dict(pdamp0=pd0, pdamp=pd, npost0=npost0, gs_first=gs_first, npre=npre)
    rng = np.random.default_rng(11)
    nt = n[0]
    s = rng.standard_normal(nt)
    Dinv = ar.inv_diag(A[0])
    for _ in range(10):
        s = s - 0.9 * Dinv * (A[0] @ s)
    rhs = {"random": rng.standard_normal(nt), "smooth": A[0] @ s}
    tol = TOL[single]
    worst = 0.0
    for name, b in rhs.items():
        x = obj.cpr_vcycle_apply(b)
        xr = H.vcycle(b, **kw)
        e = _rel(x, xr)
        worst = max(worst, e)
        assert e <= tol, (case, name, e, "|x| %.3e |xr| %.3e |b| %.3e |A0| %.3e" % (np.abs(x).max(), np.abs(xr).max(), np.abs(b).max(), np.abs(A[0].data).max()))
        if nl == 1:
            continue          # level 0 is the coarsest level: the cycle is its dense inverse, no smoother and no correction to perturb
        # controls: omega + 0.005; the factor INTO level 0 x 1.01 alone; the factor below level 0 x 1.01 alone (only with a level below
        # level 1); one Galerkin contribution of level 0 dropped -- in f64 an off-diagonal coupling of median size, in f32 (whose rounding
        # cannot resolve that) the largest diagonal entry
        names = ["omega", "pdamp0", "pdamp", "dropped"]
        controls = [H.vcycle(b, **dict(kw, omega=ar.OMEGA + 0.005)), H.vcycle(b, **dict(kw, pdamp0=pd0 * 1.01)),
                    H.vcycle(b, **dict(kw, pdamp=pd * 1.01)) if nl >= 3 else None]
        A0 = A[0][:nb, :nb].tocoo()
        if single:
            i = int(np.argmax(np.abs(A[0].diagonal()[:nb])))
            drop = (i, i)
        else:
            off = np.flatnonzero((A0.row != A0.col) & (A0.data != 0))
            k = off[np.argsort(np.abs(A0.data[off]))[off.size // 2]]
            drop = (int(A0.row[k]), int(A0.col[k]))
        controls.append(ar.Hierarchy(A[0], aggs, drop=drop).vcycle(b, **kw))
        margins = [None if xc is None else _rel(x, xc) / tol for xc in controls]
        print("%s %s: cycle %.2e, control margins %s" % (case, name, e, ", ".join("%s %.0f" % (nm, m) for nm, m in zip(names, margins) if m is not None)))
        # f32: omega 0.9 -> 0.905 moves these cycles by only 4e-5 .. 3e-3 relative (the coarse correction dominates them), which float
        # rounding cannot resolve by 100x; the f64 run of the same deck carries that control
        for nm, m in zip(names, margins):
            if m is not None and not (single and nm == "omega"):
                assert m >= 100, (case, name, nm, m)
    b1, b2 = rhs["random"], rhs["smooth"] / np.linalg.norm(rhs["smooth"]) * np.linalg.norm(rhs["random"])
    lin = obj.cpr_vcycle_apply(0.5 * b1 - 2.0 * b2) - (0.5 * obj.cpr_vcycle_apply(b1) - 2.0 * obj.cpr_vcycle_apply(b2))
    assert np.linalg.norm(lin) <= tol * np.linalg.norm(obj.cpr_vcycle_apply(b1)), case
    # the exports leave the solver as they found it: the same cycle twice is bitwise the same
    assert np.array_equal(obj.cpr_vcycle_apply(b1), obj.cpr_vcycle_apply(b1))

    # ---- the whole two-stage application: stage 2 is the oracle's block ILU0 in the device's elimination order (float emulated in f32)
    if cpr is not None:
        oracle, J, pos, relax, gc = cpr
        st_, lu = oracle.ilu0(rowptr, col, val9, position=pos, single=single)
        assert st_ == 0

        def stage2(z):
            return oracle.ilu0_apply(rowptr, col, lu, z, position=pos, relax=relax, single=single)
        for name, b in (("random", rng.standard_normal(3 * nb)), ("smooth", J @ np.repeat(s[:nb], 3))):
            v = obj.cpr_apply(b)
            vr = ar.cpr_apply(b, J, w, Ap, lambda q: H.vcycle(q, **kw), stage2, global_constant=gc, nw=nw)
            e = _rel(v, vr)
            worst = max(worst, e)
            assert e <= tol, (case, "cpr", name, e)
            margins = [_rel(v, ar.cpr_apply(b, J, w, Ap, lambda q: H.vcycle(q, **dict(kw, pdamp0=pd0 * 1.01)), stage2, global_constant=gc, nw=nw)) / tol]
            if gc:          # the global constant removed or not
                margins.append(_rel(v, ar.cpr_apply(b, J, w, Ap, lambda q: H.vcycle(q, **kw), stage2, global_constant=False, nw=nw)) / tol)
            print("%s cpr %s: %.2e, control margins %s" % (case, name, e, ", ".join("%.0f" % m for m in margins)))
            assert min(margins) >= 100, (case, "cpr", name, margins)

    # ---- the point ILU0 of A_p that preconditions the inner elliptic solve (cpr_use_amg = 0)
    if pilu is not None:
        pos, relax = pilu
        order = np.concatenate([pos, np.arange(nb, n[0])])
        for name, b in rhs.items():
            x = obj.cpr_elliptic_ilu_apply(b)
            xr = np.empty(n[0])
            xr[:nb] = ar.point_ilu0_apply(A[0][:nb, :nb], order[:nb], b[:nb], relax)
            xr[nb:] = relax * Dinv[nb:] * b[nb:]
            e = _rel(x, xr)
            worst = max(worst, e)
            # control: the plain diagonal (Jacobi) instead of the ILU0
            m = _rel(x, relax * Dinv * b) / tol
            print("%s point ILU0 %s: %.2e, control margin %.0f" % (case, name, e, m))
            assert e <= tol and m >= 100, (case, "point ilu0", name, e, m)
    print("%s: levels %s, border wells %d, worst relative difference %.2e (tolerance %.0e)" % (case, list(n), nw, worst, tol))
    return n


# ---------------------------------------------------------------- B1: computeNewtonIncrement on a caller's BSR, no wells, no coarse space
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("dims", [(20, 18, 16), (40, 40, 40)])
def test_b1_hierarchy(gpu_lib, oracle, dims, single):
    """5 760 rows (row_sub, row_wave, dense <S,4>) and 64 000 rows (coarsest 65-96 rows: dense <S,12>); ragged SELL slices (NNCs)"""
    rowptr, col, val, b = _b1_system(oracle, *dims)
    s = GpuNewtonIteration(capi.default_params(**capi.CPR_AMG_VCYCLE, linear_solver_reduction=1e-6, linear_solver_maxiter=200))
    s.computeNewtonIncrement(rowptr, col, val, b, single)
    pos = s.ordering()[0]
    n = check_hierarchy(s, rowptr, col, val, single, "b1_%dx%dx%d_%s" % (dims + ("f32" if single else "f64",)),
                        cpr=(oracle, _bsr(rowptr, col, val), pos, 1.0, False))
    assert s.cpr_correction_factors() == (1.9, 1.9)          # external matrices keep the documented factor
    assert n[0] == rowptr.size - 1
    s.close()


def test_b1_stalled_coarsest_jacobi(gpu_lib, oracle, monkeypatch):
    """OPMGPU_AMG_MAXLEVELS=2: level 1 (> 96 rows) is the coarsest and gets Jacobi pairs instead of a dense inverse"""
    monkeypatch.setenv("OPMGPU_AMG_MAXLEVELS", "2")
    rowptr, col, val, b = _b1_system(oracle, 20, 18, 16)
    s = GpuNewtonIteration(capi.default_params(**capi.CPR_AMG_VCYCLE, linear_solver_reduction=1e-6, linear_solver_maxiter=300))
    s.computeNewtonIncrement(rowptr, col, val, b, False)
    n = check_hierarchy(s, rowptr, col, val, False, "b1_maxlevels2", knobs=(("maxlevels", 2),))
    assert len(n) == 2 and n[1] > ar.DENSE_MAX
    s.close()


def test_b1_gauss_seidel_level0(gpu_lib, oracle, monkeypatch):
    """OPMGPU_AMG_GS=1 (two-colour order of level 0): Gauss-Seidel by colour on level 0"""
    monkeypatch.setenv("OPMGPU_AMG_GS", "1")
    rowptr, col, val, b = _b1_system(oracle, 20, 18, 16, nnc=0.0)
    s = GpuNewtonIteration(capi.default_params(**capi.CPR_AMG_VCYCLE, linear_solver_reduction=1e-6, linear_solver_maxiter=300))
    s.computeNewtonIncrement(rowptr, col, val, b, False)
    pos, lev, nlev = s.ordering()
    assert nlev == 2
    check_hierarchy(s, rowptr, col, val, False, "b1_gs", knobs=(("gs", 1),), gs_first=lev == 0)
    s.close()


@pytest.mark.parametrize("single", [False, True])
def test_b1_elliptic_point_ilu0(gpu_lib, oracle, single):
    """the reference's default CPR (cpr_use_amg = 0): an inner BiCGStab on A_p preconditioned by a point ILU0 of A_p in the plan's order"""
    rowptr, col, val, b = _b1_system(oracle, 20, 18, 16)
    s = GpuNewtonIteration(capi.default_params(use_cpr=1, cpr_use_amg=0, linear_solver_reduction=1e-6, linear_solver_maxiter=200))
    s.computeNewtonIncrement(rowptr, col, val, b, single)
    pos = s.ordering()[0]
    check_hierarchy(s, rowptr, col, val, single, "b1_pilu_%s" % ("f32" if single else "f64"), pilu=(pos, 1.0))
    s.close()


# ---------------------------------------------------------------- B2: the model's own assembly
def _model(dims, single, wells=True, seed=None, rate=40.0, **prm_kw):
    tab = decks.satfunc_standard_tables()
    if seed is None:
        grid = decks.cartesian_grid(*dims, lognormal_sigma=0.5)
        st = decks.initial_state(grid, tab, perturb=0.002)
    else:
        grid = decks.cartesian_grid(*dims, lognormal_sigma=0.5, seed=seed)
        st = decks.initial_state(grid, tab, perturb=0.002, seed=seed)
    prm = capi.default_params(**dict(capi.CPR_AMG_VCYCLE, linear_solver_reduction=1e-6, linear_solver_maxiter=300, **prm_kw))
    gm = GpuBlackoilModel(grid, tab, prm)
    if wells:
        wl = W.five_spot(grid, rate_m3_per_day=rate, bhp_prod_bar=150.0)
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
        md.prepareStep(1 * decks.DAY, st)
        md.nonlinearIteration(0, single_precision=single)
    else:
        gm.prepareStep(1 * decks.DAY, st)
        gm.setSolvePrecision(single)          # before the assembly, as nonlinearIteration does: the Jacobian is written in the solve's precision
        gm.assemble(True)
        gm.getConvergence()
        gm.solveJacobianSystem(single_precision=single)
    return gm


@pytest.mark.parametrize("dims,single", [((9, 9, 12), False), ((9, 9, 12), True), ((4, 4, 4), False), ((30, 30, 30), False)])
def test_b2_bordered_level0(gpu_lib, dims, single):
    """device wells: level 0 carries one border row per well.  972 cells: row_wave + border; 27 000 cells: smooth0_residual and residual<3>
    with border workgroups; 4x4x4 + 5 wells = 69 rows: level 0 is also the coarsest level and the dense inverse must be that of the whole
    bordered operator (cells AND wells)"""
    gm = _model(dims, single)
    rowptr, col, val = gm.jacobian()
    n, _, nw = gm.cpr_levels()
    assert nw == 5
    n = check_hierarchy(gm, rowptr, col, val, single, "b2_wells_%dx%dx%d_%s" % (dims + ("f32" if single else "f64",)))
    if dims == (4, 4, 4):
        assert len(n) == 1 and n[0] == 64 + 5
    gm.close()


def test_b2_bordered_stalled_coarsest(gpu_lib, monkeypatch):
    """OPMGPU_AMG_MAXLEVELS=2 with device wells: the Jacobi pairs of the coarsest level run over the wells' singleton rows too"""
    monkeypatch.setenv("OPMGPU_AMG_MAXLEVELS", "2")
    gm = _model((9, 9, 12), False)
    rowptr, col, val = gm.jacobian()
    n = check_hierarchy(gm, rowptr, col, val, False, "b2_wells_maxlevels2", knobs=(("maxlevels", 2),))
    assert len(n) == 2 and n[1] > ar.DENSE_MAX
    gm.close()


@pytest.mark.parametrize("single", [False, True])
def test_b2_global_constant(gpu_lib, oracle, single):
    """a deck without wells on the model path: the global-constant correction of the pressure stage and 2.2 into level 0 (1.9 below)"""
    gm = _model((60, 60, 60), single, wells=False)
    rowptr, col, val = gm.jacobian()
    assert gm.cpr_correction_factors() == (2.2, 1.9)
    pos = gm.ordering()[0]
    check_hierarchy(gm, rowptr, col, val, single, "b2_nowells_60_%s" % ("f32" if single else "f64"), cpr=(oracle, _bsr(rowptr, col, val), pos, 1.0, True))
    gm.close()


@pytest.mark.parametrize("single", [False, True])
def test_b2_bench_deck(gpu_lib, single):
    """the bench deck: 100^3 with its 5-spot, GMRES (1 post-sweep on level 0); f32 = preconditioner_single (float hierarchy in a double
    solve).  Bordered level 0 above 400 000 rows, unfused prolongation, Galerkin with 1 lane per entry on the big levels"""
    gm = _model((100, 100, 100), False, seed=12345, rate=1000.0, newton_use_gmres=1, preconditioner_single=int(single))
    rowptr, col, val = gm.jacobian()
    n = check_hierarchy(gm, rowptr, col, val, single, "b2_bench_100_%s" % ("mixed" if single else "f64"), npost0=1)
    assert n[0] == 1000000 + 5 and len(n) >= 5
    gm.close()


# ---------------------------------------------------------------- knobs read once per process: one subprocess each (tests/_cpr_stage_worker.py)
KNOBS = [("OPMGPU_AMG_SUB", "0,0"), ("OPMGPU_AMG_SUB", "1,100000000"), ("OPMGPU_AMG_FUSE", "0"), ("OPMGPU_AMG_GALERKIN_LPE", "16,16"),
         ("OPMGPU_AMG_GALERKIN_LPE", "64,64"), ("OPMGPU_AMG_NPRE", "2"), ("OPMGPU_AMG_GS", "1")]


def test_knobs_in_subprocesses(gpu_lib):
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for name, value in KNOBS:
        env = dict(os.environ, **{name: value})
        p = subprocess.run([sys.executable, os.path.join(here, "_cpr_stage_worker.py"), name, value], env=env, cwd=os.path.dirname(here),
                           capture_output=True, text=True, timeout=240)
        print(p.stdout[-3000:])
        assert p.returncode == 0, (name, value, p.returncode, p.stdout[-3000:], p.stderr[-3000:])
        res = json.loads(p.stdout.strip().splitlines()[-1])
        SEEN["knob %s=%s" % (name, value)] = (res["n"], res["nw"], tuple(map(tuple, res["knobs"])), res["nnz"])


# ---------------------------------------------------------------- coverage of the cycle's code paths
def _regimes(n, nw, knobs, nnz=None):
    """the branch vcycle() / sweep() / galerkin() take for every level of one case (amg.hip's default thresholds and the case's knobs)"""
    k = dict(knobs)
    sub = tuple(int(v) for v in k.get("sub", "2000,400000").split(","))
    fuse = int(k.get("fuse", 1))
    out = set()
    for l, nl in enumerate(n):
        bord = l == 0 and nw > 0
        tag = "+border" if bord else ""
        cells = nl - (nw if l == 0 else 0)
        if l == len(n) - 1:
            out.add(("dense<4>" if nl <= 64 else ("dense<12>" if nl <= 96 else "jacobi pairs")) + tag)
            continue
        lpe = k.get("lpe")
        if lpe is None and nnz is not None:
            lpe = "1" if nnz[l + 1] > 400000 else "8"
        if lpe is not None:
            out.add("galerkin lpe " + str(lpe))
        if l == 0 and k.get("gs"):
            out.add("gs by colour")
            continue
        if not bord and sub[0] < cells <= sub[1]:
            out.add("row_sub")
        elif cells > 50000:
            out.add("residual<0>" + tag)
        elif cells > 20000:
            out.add("smooth0_residual" + tag)
        else:
            out.add("row_wave" + tag)
        if not fuse or cells > 200000:
            out.add("unfused prolongation" + tag)
        if k.get("npre", 1) != 1:
            out.add("npre 2")
    return out


WANT = {"residual<0>+border", "unfused prolongation+border", "row_sub", "smooth0_residual+border", "row_wave+border", "row_wave",
        "smooth0_residual", "dense<4>", "dense<12>", "dense<12>+border", "jacobi pairs", "galerkin lpe 1", "galerkin lpe 8",
        "galerkin lpe 16", "galerkin lpe 64", "gs by colour", "unfused prolongation", "npre 2"}


def test_coverage_of_the_cases():
    """every row of the cycle's table of code paths is reached by some level of some case above (a deck edit that moves a level across a
    threshold fails here instead of silently dropping a path).  Needs the module's other tests in the same session."""
    seen = set()
    for case, v in SEEN.items():
        seen |= _regimes(*v)
    assert WANT <= seen, ("regimes not reached by the cases run in this session: %s" % sorted(WANT - seen),
                          "cases run: %s" % {c: list(map(int, v[0])) for c, v in SEEN.items()})
