"""Analytic aquifers on the device (csrc/aquifer.hip; the rule is stated in include/opmgpu.h at opmgpu_set_aquifers) against its float64
restatement (aquifer_reference.py) and, for what the rule takes of a cell, the 50-digit cell reference (cell_reference.py):

  1  the begin-step kernels: rho0, p0 of every connection against the cell reference, A_j and B_j against the restatement
  2  the assembly kernel: nothing outside the water equation of the connected cells changes by a bit; the changes there are the restatement's
  3  the float copy of a double Jacobian and the CPR weights follow the final diagonal blocks
  4  lifecycle: commit by the documented tree bit for bit, begin twice, restore discards, save commits once, state round trip, the fused
     Newton iteration, refusals
  5  material balance of a closed box with one aquifer through AdaptiveTimeStepping
  6  tests/golden/decks/AQUIFER_SMALL.DATA through the report-step driver, with and without its aquifer keywords

Limits of 1 and 2 for p_w, rho_w, b_w: test_gpu_cell_edges.py's per (property, slot) and hydrocarbon-state group -- 8 times the oracle's
error on the edge-case cells, floor 64 ulp, relative to the slot's largest entry in the group -- taken from that file's own function.
Measured on the MI355X: DESIGN section 15."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aquifer_reference as AQ
import cell_edge_cases as E
import cell_reference as R
import twophase as TP
from opmgpu import capi, decks, wells as W
from opmgpu.model import GpuBlackoilModel, NonlinearSolver
from test_gpu_cell_edges import limits as edge_limits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DECK = os.path.join(HERE, "golden", "decks", "AQUIFER_SMALL.DATA")
DT = 3 * decks.DAY
EPS = 2.0 ** -52
PROPS = ["p_w", "b_w", "rho_w"]
# A_j, B_j of the device against the restatement GIVEN the device's own rho0, p0: the limit is 4 x the worst relative error measured on
# the MI355X and never above 1e-12.  Measured: 0 for A and for B over the 450 connections -- the device's expm1 and the
# host's agree on the three arguments, every other operation of the rule is one correctly rounded float64 operation on both sides -- so
# the limit is 0: bit for bit.
AB_MEASURED = 0.0
AB_LIMIT = min(4 * AB_MEASURED, 1e-12)
TD = [0.01, 0.05, 0.1, 0.5, 1.0, 5.0, 10.0, 50.0, 100.0, 1000.0]
PD = [0.112, 0.229, 0.315, 0.616, 0.802, 1.362, 1.651, 2.388, 2.723, 3.860]
NX, NY = 20, 16


def make_aquifers(nc=NX * NY, p_a0=260.0e5, seed=2):
    """1, 63, 64, 65 and 257 connections, both kinds; the 257 shares cells with the 64 and the 65, the 65 with the 63, the 1 with the 63"""
    rng = np.random.default_rng(seed)

    def al(n):
        w = rng.uniform(0.5, 2.0, n)
        return w / w.sum()
    assert nc >= 320
    return [AQ.Aquifer(AQ.FETKOVICH, p_a0, 2010.0, CtV0=0.05, J=6.0e-9, cells=np.arange(0, 257), alpha=al(257)),
            AQ.Aquifer(AQ.CARTER_TRACY, p_a0 + 3.0e5, 1995.0, beta=3.0e-3, Tc=1.1e5, td=TD, pd=PD, cells=np.arange(250, 315), alpha=al(65)),
            AQ.Aquifer(AQ.FETKOVICH, p_a0 - 2.0e5, 2000.0, CtV0=0.5, J=2.0e-9, cells=np.arange(100, 164)[::-1], alpha=al(64)),
            AQ.Aquifer(AQ.CARTER_TRACY, p_a0, 2003.0, beta=1.0e-3, Tc=4.0e5, td=TD[:2], pd=PD[:2], cells=np.arange(257, 320), alpha=al(63)),
            AQ.Aquifer(AQ.FETKOVICH, p_a0 + 1.0e5, 2001.0, CtV0=0.01, J=1.0e-9, cells=[319], alpha=[1.0])]


def conn_cells(aqs):
    return np.concatenate([a.cells for a in aqs])


def conn_ranges(aqs):
    ptr = np.concatenate([[0], np.cumsum([a.cells.size for a in aqs])])
    return [slice(ptr[k], ptr[k + 1]) for k in range(len(aqs))]


@pytest.fixture(scope="module")
def yard(oracle):
    """test_gpu_cell_edges.py's limits of the base edge-case set for p_w, b_w, rho_w: {group: limit[3][4]}"""
    sets, _ = E.load()
    Cs = sets["base"]
    table = E.error_table(Cs, E.oracle_props(oracle, Cs), R.NAMES[:oracle.NPROP])
    return Cs, edge_limits(Cs, table, PROPS)


def group_names(hc):
    return np.where(hc == capi.HC_GAS_AND_OIL, "gas+oil", np.where(hc == capi.HC_OIL_ONLY, "oil", "gas"))


def absolute_limits(lim, groups, ref):
    """[nc][3][4]: the relative limit of a cell's group times the slot's largest |reference| among the cells of that group.  ref: [nc][3][4]"""
    out = np.zeros_like(ref)
    for g in np.unique(groups):
        i = np.flatnonzero(groups == g)
        out[i] = lim[g][None] * np.abs(ref[i]).max(0)[None]
    return out


def ref_props(tab, grid, st):
    pvt = np.zeros(grid.nc, int) if grid.pvtnum is None else grid.pvtnum
    sat = np.zeros(grid.nc, int) if grid.satnum is None else grid.satnum
    ref, _ = R.cells(tab, pvt, sat, st)
    return ref[:, [R.NAMES.index(n) for n in PROPS]]


def sloped(g, seed=4, **more):
    """the grid with its cell depths varied by up to 15 m (a hydrostatic head per connection)"""
    z = np.asarray(g.z) + np.random.default_rng(seed).uniform(-15.0, 15.0, g.nc)
    return decks.GridData(g.nc, g.conn_cells, g.trans, g.pv, z, gravity=g.gravity, dims=g.dims, **more)


# ---------------------------------------------------------------- 1
def test_begin_step_coefficients(gpu_lib, yard):
    """20 x 16 x 1 cells holding 320 of the edge-case cells (table nodes, table ends, blends, all hydrocarbon states), aquifers with a
    history (W_e, t non-zero): rho0, p0 per connection against the 50-digit reference; A_j, B_j against the restatement fed with the
    device's own rho0, p0; q_j = A_j - B_j p0 bit for bit (the resident state is the one frozen) and qs_j / q_j = b_w."""
    Cs, lim = yard
    src = np.random.default_rng(5).permutation(Cs.nc)[:NX * NY]
    grid = sloped(decks.cartesian_grid(NX, NY, 1, lognormal_sigma=0.3), pvtnum=Cs.pvtnum[src], satnum=Cs.satnum[src])
    s = Cs.state
    st = decks.State(s.p[src], s.sat[src], s.rs[src], s.rv[src], s.hc[src])
    ref = Cs.ref[src][:, [R.NAMES.index(n) for n in PROPS]]
    groups = np.full(src.size, "", dtype=object)
    for g, idx in E.hc_groups(Cs).items():
        groups[np.isin(src, idx)] = g
    alim = absolute_limits(lim, groups, ref)
    aqs = make_aquifers()
    We0, t0 = [300.0, 40.0, -25.0, 0.0, 1.0], [4.0e5, 7.0e5, 0.0, 3.0e4, 1.0e5]
    m = GpuBlackoilModel(grid, Cs.tab, capi.default_params())
    m.setState(st)
    m.setAquifers(aqs)
    m.setAquiferState(W_e=We0, t=t0)
    m.prepareStep(DT)
    got = m.aquiferConnections()
    m.close()
    cells = conn_cells(aqs)
    assert got.shape == (450, 6)
    for k, name in ((0, "rho_w"), (1, "p_w")):
        p = PROPS.index(name)
        err, allowed = np.abs(got[:, k] - ref[cells, p, 0]), alim[cells, p, 0]
        j = int(np.argmax(err / allowed))
        print("%s0: largest error %.3g of its limit %.3g (%.2f), connection %d" % (name, err[j], allowed[j], err[j] / allowed[j], j))
        assert np.all(err <= allowed), (name, j, err[j], allowed[j])
    worst = {"A": 0.0, "B": 0.0}
    for a, r, we, t in zip(aqs, conn_ranges(aqs), We0, t0):
        a.We, a.t = we, t
        A, B = AQ.coefficients(a, AQ.scalars(a, DT), got[r, 0], got[r, 1], grid.z[a.cells], grid.gravity)
        assert np.all(B > 0) and np.all(np.abs(A) > 0)
        worst["A"] = max(worst["A"], float(np.abs(got[r, 2] / A - 1.0).max()))
        worst["B"] = max(worst["B"], float(np.abs(got[r, 3] / B - 1.0).max()))
        assert np.array_equal(got[r, 4], AQ.rates(got[r, 2], got[r, 3], got[r, 1]))
    print("A_j, B_j against the restatement, worst relative error: A %.3g, B %.3g; limit %.3g" % (worst["A"], worst["B"], AB_LIMIT))
    assert worst["A"] <= AB_LIMIT and worst["B"] <= AB_LIMIT
    p = PROPS.index("b_w")
    nz = got[:, 4] != 0.0
    assert np.all(np.abs(got[nz, 5] / got[nz, 4] - ref[cells[nz], p, 0]) <= alim[cells[nz], p, 0] + 2 * EPS * ref[cells[nz], p, 0])


# ---------------------------------------------------------------- 2, 3
def benign(kind):
    """(grid, tables, state, tables the cell reference evaluates) of a quiet 20 x 16 x 1 reservoir: three phases, or oil and water"""
    if kind == "ow":
        g = TP.grid(NX, NY, 1)
        grid = sloped(g, pvtnum=g.pvtnum, satnum=g.satnum)
        return grid, TP.tables(), TP.state(g), TP.twin_tables()
    grid = sloped(decks.cartesian_grid(NX, NY, 1, lognormal_sigma=0.3))
    tab = decks.satfunc_standard_tables()
    return grid, tab, decks.initial_state(grid, tab, perturb=0.03), tab


def one_well(grid):
    """a BHP producer in cell 300: a cell of the 65- and the 63-connection aquifers"""
    wl = W.Wells()
    wl.add_well("P", W.PRODUCER, grid.z[300], [300], 5.0 * float(np.median(grid.trans)), (0.0, 1.0, 0.0), (W.BHP, 150 * decks.BAR), limits=[])
    return wl


def assembled(grid, tab, st, aqs, variant, prm):
    m = GpuBlackoilModel(grid, tab, prm)
    if aqs is not None:
        m.setAquifers(aqs)                # before the wells: the re-plan behind them has to carry the aquifers over
    if variant == "well":
        wl = one_well(grid)
        md = W.DeviceWellModel(m, wl, W.WellState(wl, st.p))
        md.prepareStep(DT, st)
    else:
        m.prepareStep(DT, st)
    m.setSolvePrecision(variant == "float")
    m.assemble(True)
    return m


@pytest.mark.parametrize("variant", ["double", "float", "mixed", "well", "ow"])
def test_assembly_adds_the_aquifer_terms_and_nothing_else(gpu_lib, yard, variant):
    """The same state assembled with and without the aquifers.  Outside the water equation of the connected cells (their water residual,
    the water row of their diagonal block) every residual entry and every matrix block is the same bits.  There, the change is the
    restatement's -s and -scale_w d_v of cell_terms() at the 50-digit b_w, p_w of the cell, within a limit propagated term by term:
        s   = sum_j b_w q_j,  q_j = A_j - B_j p_w:      sum_j |q_j| e(b_w) + b_w B_j e(p_w)
        d_v = sum_j b_w,v q_j - b_w B_j p_w,v:          sum_j |q_j| e(b_w,v) + |b_w,v| B_j e(p_w) + B_j (|p_w,v| e(b_w) + b_w e(p_w,v))
    with e(.) the absolute limit of the slot (test_gpu_cell_edges.py's), plus 4 eps of every product summed (the device's own roundings:
    two per term and the sum) and one rounding of the entry the term is subtracted from (eps |R|; for the matrix in ITS precision).
    A_j, B_j are the device's (test 1 holds them).  Variants: a double and a float matrix, a double matrix with its float copy
    (preconditioner_single), a device well in a connected cell (set after the aquifers: a re-plan), an oil-water context."""
    _, lim = yard
    grid, tab, st, rtab = benign("ow" if variant == "ow" else "wog")
    prm = capi.default_params(**(dict(capi.CPR_AMG_VCYCLE, preconditioner_single=1) if variant == "mixed" else {}))
    aqs = make_aquifers()
    m1 = assembled(grid, tab, st, aqs, variant, prm)
    m0 = assembled(grid, tab, st, None, variant, prm)
    coef = m1.aquiferConnections()
    r1, r0 = m1.residual(), m0.residual()
    rowptr, col, J1 = m1.jacobian()
    rowptr0, col0, J0 = m0.jacobian()
    fcopy = m1.jacobianFloatCopy() if variant == "mixed" else None
    if variant == "mixed":
        with pytest.raises(ValueError, match="float copy"):
            assembled(grid, tab, st, None, "float", prm).jacobianFloatCopy()
    scale_w = m1.params.matbalscale[0]
    m1.close(); m0.close()
    nc = grid.nc
    assert np.array_equal(rowptr, rowptr0) and np.array_equal(col, col0)
    cells = conn_cells(aqs)
    touched = np.unique(cells)
    diag = np.flatnonzero(np.repeat(np.arange(nc), np.diff(rowptr)) == col)
    assert np.array_equal(col[diag], np.arange(nc))
    # nothing else changes
    rmask = np.ones(3 * nc, bool); rmask[touched] = False
    assert np.array_equal(r1[rmask], r0[rmask])
    jmask = np.ones(J1.shape, bool); jmask[diag[touched], 0:3] = False
    assert np.array_equal(J1[jmask], J0[jmask])
    assert np.any(r1[touched] != r0[touched]) and np.any(J1[diag[touched], 0:3] != J0[diag[touched], 0:3])
    # the change
    ref = ref_props(rtab, grid, st)
    alim = absolute_limits(lim, group_names(st.hc), ref)
    ipw, ibw = PROPS.index("p_w"), PROPS.index("b_w")
    store = 2.0 ** -24 if variant == "float" else EPS / 2
    worst = [0.0, 0.0]
    for c in touched:
        js = np.flatnonzero(cells == c)                         # ascending: the listing order
        A, B = coef[js, 2], coef[js, 3]
        bw, pw, ebw, epw = ref[c, ibw], ref[c, ipw], alim[c, ibw], alim[c, ipw]
        s, d = AQ.cell_terms(A, B, bw, pw)
        q = A - B * pw[0]
        prod = np.abs(A) + np.abs(B * pw[0])                    # the size of q_j's terms before they cancel
        tol_s = np.sum(np.abs(q) * ebw[0] + bw[0] * B * epw[0]) + 4 * EPS * np.sum(bw[0] * prod) + EPS * max(abs(r1[c]), abs(r0[c]))
        got_s = -(r1[c] - r0[c])
        assert abs(got_s - s) <= tol_s, (variant, c, got_s, s, tol_s)
        worst[0] = max(worst[0], abs(got_s - s) / tol_s)
        dpw = np.array([1.0, pw[2], 0.0])
        edpw = np.array([0.0, epw[2], 0.0])                     # d p_w / dp = 1 and d p_w / dX = 0 are exact
        for v in range(3):
            tol_d = np.sum(np.abs(q) * ebw[1 + v] + abs(bw[1 + v]) * B * epw[0] + B * (abs(dpw[v]) * ebw[0] + bw[0] * edpw[v]))
            tol_d += 4 * EPS * np.sum(abs(bw[1 + v]) * prod + bw[0] * B * abs(dpw[v]))
            tol_d = scale_w * tol_d + store * 2 * max(abs(J1[diag[c], v]), abs(J0[diag[c], v]))
            got_d = -(J1[diag[c], v] - J0[diag[c], v])
            assert abs(got_d - scale_w * d[v]) <= tol_d, (variant, c, v, got_d, scale_w * d[v], tol_d)
            worst[1] = max(worst[1], abs(got_d - scale_w * d[v]) / tol_d if tol_d > 0 else 0.0)      # (a slot that is exactly zero on both sides)
    print("%s: %d connected cells; nearest its limit: residual %.3f, matrix %.3f" % (variant, touched.size, worst[0], worst[1]))
    if fcopy is not None:
        # the float copy of every block is float(double block): on the aquifer rows too, whose double blocks changed after the copy was written
        want = J1.astype(np.float32).astype(np.float64)
        assert np.array_equal(fcopy[diag[touched]], want[diag[touched]])
        assert np.array_equal(fcopy, want)


def cpr_weights(m):
    w = np.zeros(3 * m.nc)
    m._chk(m.lib.opmgpu_get_cpr_weights(m.ctx, capi.dptr(w)))
    return w.reshape(3, m.nc)


def dominance_weights(rowptr, col, val):
    """formEllipticSystem's 0 / 1 weights (NewtonIterationUtilities.cpp:212-252) of a block matrix, as test_gpu_wells.py restates them"""
    nb = rowptr.size - 1
    rows = np.repeat(np.arange(nb), np.diff(rowptr))
    diag = rows == col
    v3 = val.reshape(-1, 3, 3)
    expect = np.zeros((3, nb))
    for eq in range(3):
        dj = np.abs(v3[diag, eq, 0])[np.argsort(rows[diag])]
        colsum = np.zeros(nb)
        np.add.at(colsum, col, np.abs(v3[:, eq, 0]))
        with np.errstate(divide="ignore", invalid="ignore"):
            expect[eq] = (dj / (colsum - dj) > 0.01)
    expect[1, expect.sum(0) == 0] = 1.0
    return expect


@pytest.mark.parametrize("single", [False, True])
def test_cpr_weights_of_aquifer_rows_follow_the_final_matrix(gpu_lib, single):
    """The assembly kernel writes the 0 / 1 weights of the pressure equation from the reservoir terms; the aquifer kernel then changes the
    water row of its cells' diagonal blocks, and their weights are redone (k_cpr_weights_rows).  They must be formEllipticSystem's rule
    applied to the FINAL matrix, and -- for a double matrix -- the ones of a context that takes every row's weights from the final matrix
    (k_cpr_weights): a context with a host well list of one perforation to which no well term is ever added, the same matrix.  (Such a
    context assembles in double whatever the solve's precision, so the float case has the rule alone.)
    What this cannot show: b_w B_j only ever raises the water row's pressure entry, which dominates its column already, so no weight of
    this deck depends on the refresh -- measured: 0 rows differ from the context without aquifers."""
    grid, tab, st, _ = benign("wog")
    aqs = make_aquifers()
    prm = capi.default_params(**capi.CPR_AMG_VCYCLE)
    out = []
    for host_well in ((False, True) if not single else (False,)):
        m = GpuBlackoilModel(grid, tab, prm, wells=(np.array([0, 1], np.int32), np.array([7], np.int32)) if host_well else None)
        m.setAquifers(aqs)
        m.prepareStep(DT, st)
        m.setSolvePrecision(single)
        m.assemble(True)
        m.getConvergence()
        m.solveJacobianSystem(single_precision=single)
        out.append((cpr_weights(m), m.jacobian()))
        m.close()
    w_rows, (rowptr, col, J_rows) = out[0]
    assert np.array_equal(w_rows, dominance_weights(rowptr, col, J_rows))
    if not single:
        w_full, (_, _, J_full) = out[1]
        assert np.array_equal(J_rows, J_full)
        assert np.array_equal(w_rows, w_full)


# ---------------------------------------------------------------- 4
def newton(m, fused=False):
    ns = NonlinearSolver()
    m.fused_iteration = fused
    for it in range(ns.max_iter + 1):
        conv, _ = m.nonlinearIteration(it, nonlinear_solver=ns)
        if conv and it >= ns.min_iter:
            return it
    raise AssertionError("the step did not converge")


def small_case():
    grid = sloped(decks.cartesian_grid(NX, NY, 1, dx=100.0, dy=100.0, dz=10.0, lognormal_sigma=0.3))      # 6.4e6 m3 of pore space: the aquifers move it gently
    tab = decks.satfunc_standard_tables()
    st = decks.initial_state(grid, tab, p_ref=200 * decks.BAR, gas_cap_fraction=0.0, gas_only_fraction=0.0)
    return grid, tab, st


def test_commit_follows_the_documented_tree_bit_for_bit(gpu_lib):
    """Two converged steps.  The commit's sums Q = sum q_j, Qs = sum qs_j over 1, 63, 64, 65 and 257 connections are the documented tree's
    (tree_sum) of the q_j, qs_j the read-out gives for the converged state, and W_e += dt Q, W_s += dt Qs, t += dt are one product and
    one sum each: bit for bit, because the restatement follows the tree.  p_a is the derived output."""
    grid, tab, st = small_case()
    aqs = make_aquifers(p_a0=215.0e5)
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    m.setAquifers(aqs)
    m.setState(st)
    for step, dt in enumerate((2 * decks.DAY, 5 * decks.DAY)):
        m.prepareStep(dt)
        newton(m)
        rec = m.aquiferConnections()
        m.saveState()
        We, Ws, t, pa = m.aquiferState()
        for k, (a, r) in enumerate(zip(aqs, conn_ranges(aqs))):
            AQ.commit(a, dt, rec[r, 4], rec[r, 5])
            assert (We[k], Ws[k], t[k]) == (a.We, a.Ws, a.t), (step, k, We[k] - a.We, Ws[k] - a.Ws)
            assert pa[k] == a.p_a()
            assert We[k] != 0.0
        print("step %d: W_e %s" % (step, We))
    m.close()


def test_lifecycle_begin_restore_save_and_state_round_trip(gpu_lib):
    grid, tab, st = small_case()
    aqs = make_aquifers(p_a0=215.0e5)
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    m.setAquifers(aqs)
    zero = m.aquiferState()
    assert all(np.all(v == 0.0) for v in zero[:3]) and np.array_equal(zero[3], [a.p_a0 for a in aqs])
    m.setState(st)
    m.saveState()
    # begin twice: the second begin discards the first; same state, same dt -> the same bits, and nothing is committed
    m.prepareStep(DT)
    first = m.aquiferConnections()
    m.prepareStep(DT)
    assert np.array_equal(m.aquiferConnections(), first)
    m.prepareStep(2 * DT)
    assert not np.array_equal(m.aquiferConnections()[:, 3], first[:, 3])
    assert all(np.all(v == 0.0) for v in m.aquiferState()[:3])
    # restore discards the begun step and leaves the committed state alone
    newton(m)
    moved = m.getState()
    assert not np.array_equal(moved.p, st.p)
    m.restoreState()
    assert m.lib.opmgpu_aquifer_commit_step(m.ctx) == capi.EINVAL
    assert m.lib.opmgpu_aquifer_connections_get(m.ctx, capi.dptr(np.zeros((450, 6)))) == capi.EINVAL
    assert np.array_equal(m.getState().p, st.p) and all(np.all(v == 0.0) for v in m.aquiferState()[:3])
    # without a begun step the assembly adds nothing: the residual is that of a context without aquifers
    m.dt = DT
    m.assemble(True)
    r_plain = m.residual()
    m0 = GpuBlackoilModel(grid, tab, capi.default_params())
    m0.prepareStep(DT, st); m0.assemble(True)
    assert np.array_equal(r_plain, m0.residual())
    m0.close()
    # save commits once only
    m.prepareStep(DT)
    newton(m)
    m.saveState()
    once = m.aquiferState()
    assert np.all(once[0] != 0.0) and np.all(once[2] == DT)
    m.saveState()
    assert all(np.array_equal(a, b) for a, b in zip(m.aquiferState(), once))
    # save and restore do not touch the committed state
    m.restoreState()
    assert all(np.array_equal(a, b) for a, b in zip(m.aquiferState(), once))
    # round trip; None leaves a column alone; a set discards a begun step
    We, Ws, t = np.arange(1.0, 6.0), -np.arange(2.0, 7.0), np.arange(5.0) * 1.0e4
    m.prepareStep(DT)
    m.setAquiferState(We, Ws, t)
    assert m.lib.opmgpu_aquifer_commit_step(m.ctx) == capi.EINVAL
    got = m.aquiferState()
    assert np.array_equal(got[0], We) and np.array_equal(got[1], Ws) and np.array_equal(got[2], t)
    assert got[3][0] == aqs[0].p_a0 - We[0] / aqs[0].CtV0 and got[3][1] == aqs[1].p_a0 - We[1] / aqs[1].beta
    m.setAquiferState(W_s=Ws + 1.0)
    got = m.aquiferState()
    assert np.array_equal(got[0], We) and np.array_equal(got[1], Ws + 1.0) and np.array_equal(got[2], t)
    # the aquifers and their state last through a re-plan (a new well list) and a change of the solve precision
    m.setWells([0, 2], [3, 4])
    m.setSolvePrecision(True)
    assert all(np.array_equal(a, b) for a, b in zip(m.aquiferState(), got))
    m.prepareStep(DT)
    assert m.aquiferConnections().shape == (450, 6)
    # removing them: the context is again one that never had any
    m.setAquifers(None)
    assert m.lib.opmgpu_aquifer_begin_step(m.ctx, DT) == capi.EINVAL
    m.prepareStep(DT)
    m.close()


def test_fused_iteration_and_call_by_call_leave_the_same_bits(gpu_lib):
    grid, tab, st = small_case()
    out = []
    for fused in (False, True):
        m = GpuBlackoilModel(grid, tab, capi.default_params())
        m.setAquifers(make_aquifers(p_a0=215.0e5))
        m.setState(st)
        its = []
        for dt in (2 * decks.DAY, 5 * decks.DAY):
            m.prepareStep(dt)
            its.append(newton(m, fused))
            m.saveState()
        out.append((its, m.getState(), m.aquiferState()))
        m.close()
    (i0, s0, a0), (i1, s1, a1) = out
    assert i0 == i1
    assert np.array_equal(s0.p, s1.p) and np.array_equal(s0.sat, s1.sat) and np.array_equal(s0.rs, s1.rs) and np.array_equal(s0.hc, s1.hc)
    assert all(np.array_equal(a, b) for a, b in zip(a0, a1)) and np.all(a0[0] != 0.0)


def test_refusals(gpu_lib):
    grid, tab, st = small_case()
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    good = make_aquifers()
    lib, ctx = m.lib, m.ctx

    def refused(change, text):
        aqs = make_aquifers()
        change(aqs)
        with pytest.raises(ValueError, match=text):
            m.setAquifers(aqs)
    # begin / commit without aquifers
    assert lib.opmgpu_aquifer_begin_step(ctx, DT) == capi.EINVAL and b"no aquifers" in lib.opmgpu_last_error(ctx)
    assert lib.opmgpu_aquifer_commit_step(ctx) == capi.EINVAL
    m.setAquifers(good)
    # begin before a state is set, with a bad dt; commit without a begun step
    assert lib.opmgpu_aquifer_begin_step(ctx, DT) == capi.EINVAL and b"no state" in lib.opmgpu_last_error(ctx)
    m.setState(st)
    for dt in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.opmgpu_aquifer_begin_step(ctx, dt) == capi.EINVAL and b"dt" in lib.opmgpu_last_error(ctx)
    assert lib.opmgpu_aquifer_commit_step(ctx) == capi.EINVAL and b"no step has begun" in lib.opmgpu_last_error(ctx)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda a: setattr(a[0], "CtV0", bad), "CtV0")
        refused(lambda a: setattr(a[2], "J", bad), "J is not")
        refused(lambda a: setattr(a[1], "beta", bad), "beta")
        refused(lambda a: setattr(a[3], "Tc", bad), "Tc")
    refused(lambda a: setattr(a[0], "p_a0", float("nan")), "p_a0")
    refused(lambda a: setattr(a[0], "datum", float("inf")), "datum")
    refused(lambda a: setattr(a[0], "kind", 2), "kind")
    refused(lambda a: setattr(a[0], "alpha", a[0].alpha * (1.0 + 1.0e-11)), "sum to 1")
    refused(lambda a: a[0].alpha.__setitem__(3, -a[0].alpha[3]), "alpha")
    refused(lambda a: a[1].cells.__setitem__(5, grid.nc), "out of range")
    refused(lambda a: a[1].cells.__setitem__(5, -1), "out of range")
    refused(lambda a: a[1].cells.__setitem__(5, a[1].cells[9]), "twice")
    refused(lambda a: (setattr(a[4], "cells", np.zeros(0, np.int64)), setattr(a[4], "alpha", np.zeros(0))), "no connections")
    refused(lambda a: (setattr(a[1], "td", [1.0]), setattr(a[1], "pd", [1.0])), "fewer than 2")
    refused(lambda a: setattr(a[1], "td", TD[:5] + [1.0] + TD[6:]), "strictly increasing")
    refused(lambda a: setattr(a[1], "pd", PD[:5] + [float("nan")] + PD[6:]), "non-finite")
    # every refusal left the previous set in force
    m.prepareStep(DT)
    assert m.aquiferConnections().shape == (450, 6)
    with pytest.raises(ValueError):
        m.setAquiferState(W_e=[float("nan")] * 5)
    # a Carter-Tracy table whose den = P - t_D P' is not positive: an error status from begin, no step begun, no NaN in the matrix
    convex = [AQ.Aquifer(AQ.CARTER_TRACY, 2.0e7, 2000.0, beta=1.0e-3, Tc=1.0e5, td=[0.0, 1.0, 2.0, 3.0], pd=[0.0, 1.0, 4.0, 9.0], cells=[1, 2], alpha=[0.5, 0.5])]
    m.setAquifers(convex)
    m.setAquiferState(t=[2.5e5])
    assert lib.opmgpu_aquifer_begin_step(ctx, 1.0e4) == capi.ENUMERICAL and b"den" in lib.opmgpu_last_error(ctx)
    assert lib.opmgpu_aquifer_commit_step(ctx) == capi.EINVAL
    m.dt = DT
    m.assemble(True)
    assert np.all(np.isfinite(m.residual())) and np.all(np.isfinite(m.jacobian()[2]))
    convex[0].t = 2.5e5
    with pytest.raises(ValueError, match="den"):          # (the restatement refuses the same step)
        AQ.scalars(convex[0], 1.0e4)
    m.close()


def test_decomposed_contexts_and_aquifers_refuse_each_other(gpu_lib):
    """opmgpu_comm_init* refuses a context with aquifers (and attach_comm says so before it gets there)"""
    from opmgpu import partition
    grid, tab, st = small_case()
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    m.setAquifers(make_aquifers())
    with pytest.raises(ValueError, match="aquifers"):
        partition.attach_comm(m, None, 0, 1, None)
    uid = (C.c_uint8 * capi.UNIQUE_ID_BYTES)()
    z = np.zeros(2, np.int32)
    st_ = m.lib.opmgpu_comm_init(m.ctx, 0, 1, uid, grid.nc, 0, capi.iptr(z), capi.iptr(z), capi.iptr(z), capi.iptr(z), capi.iptr(z))
    assert st_ == capi.EINVAL and b"aquifers" in m.lib.opmgpu_last_error(m.ctx)
    m.close()


# ---------------------------------------------------------------- 5
def test_material_balance_of_a_closed_box(gpu_lib):
    """A closed 5 x 4 x 3 box without wells under a Fetkovich aquifer 20 bar above it, 6 report steps through AdaptiveTimeStepping: the
    water in place (computeFluidInPlace, surface volume) grows by W_s and the oil in place stays.
    Bound: a converged sub-step of length dt has MB_a = B_a |sum_c R_a,c| dt / sum pv < tolerance_mb (opmgpu_convergence; B_a the mean of
    1 / b_a).  sum_c R_w,c dt is the change of the water in place over the sub-step minus dt sum_j b_w q_j -- the fluxes between cells
    cancel in the sum, the box has no other source --, and the commit adds exactly dt sum_j b_w q_j of the same converged state to W_s.
    So every sub-step leaves at most tolerance_mb sum pv / B_a unaccounted for, and with 1 / B_a <= the largest b_a met (b_w and the
    undersaturated b_o rise with the pressure, which rises from the initial to the final state: the larger of the two states' maxima)
    the bound is  n_substeps tolerance_mb sum pv max b_a."""
    from opmgpu import timestepping as ts
    grid = decks.cartesian_grid(5, 4, 3, dx=100.0, dy=100.0, dz=5.0, lognormal_sigma=0.3)
    tab = decks.satfunc_standard_tables()
    st = decks.initial_state(grid, tab, p_ref=200 * decks.BAR, gas_cap_fraction=0.0, gas_only_fraction=0.0)
    prm = capi.default_params()
    m = GpuBlackoilModel(grid, tab, prm)
    bottom = np.arange(40, 60)
    aq = AQ.Aquifer(AQ.FETKOVICH, float(st.p[bottom].mean()) + 20 * decks.BAR, float(grid.z[bottom].mean()), CtV0=1.0, J=2.0e-9, cells=bottom,
                    alpha=np.full(20, 0.05))
    m.setAquifers([aq])
    m.setState(st)
    fip0 = m.computeFluidInPlace()[0]
    b0 = m.simulatorData()
    ats = ts.AdaptiveTimeStepping(initial_timestep_days=1.0)

    class Solver:
        def step(self, model):
            ns = NonlinearSolver()
            return ns.step(model)
    nsub, t = 0, 0.0
    for _ in range(6):
        rep = ats.step(t, 5 * decks.DAY, Solver(), m)
        t += 5 * decks.DAY
        nsub += len(rep["substeps"])
    fip1 = m.computeFluidInPlace()[0]
    b1 = m.simulatorData()
    We, Ws, ta, pa = m.aquiferState()
    p_end = m.getState().p
    m.close()
    assert ta[0] == pytest.approx(t, rel=1e-12) and Ws[0] > 0 and p_end.mean() > st.p.mean() + 5 * decks.BAR
    pvsum = float(np.sum(grid.pv))
    bmax = [max(b0[k].max(), b1[k].max()) for k in ("1OVERBW", "1OVERBO")]
    bound = [nsub * prm.tolerance_mb * pvsum * b for b in bmax]
    dw = fip1[0] - fip0[0]
    do = (fip1[1] + fip1[4]) - (fip0[1] + fip0[4])
    print("%d sub-steps; water in place +%.6f sm3, W_s %.6f sm3: difference %.3g, bound %.3g; oil in place changes by %.3g, bound %.3g"
          % (nsub, dw, Ws[0], dw - Ws[0], bound[0], do, bound[1]))
    assert abs(dw - Ws[0]) <= bound[0]
    assert abs(do) <= bound[1]
    assert Ws[0] > 10 * bound[0]             # the influx is far above what the bound lets pass: the comparison means something


# ---------------------------------------------------------------- 6
def without_aquifers(text):
    """the deck without its AQUFETP, AQUCT, AQUTAB and AQUANCON keywords (AQUDIMS stays: it only sizes)"""
    out, skip = [], False
    for line in text.splitlines():
        word = line.strip()
        if re.fullmatch(r"[A-Z][A-Z0-9]*", word):
            skip = word in ("AQUFETP", "AQUCT", "AQUTAB", "AQUANCON")
        if not skip:
            out.append(line)
    return "\n".join(out) + "\n"


def test_golden_deck_with_and_without_its_aquifers(gpu_lib, tmp_path):
    from opmgpu.simulator import Simulator
    closed = tmp_path / "CLOSED.DATA"
    closed.write_text(without_aquifers(open(DECK).read()))
    end = {}
    for name, path in (("aquifers", DECK), ("closed", str(closed))):
        sim = Simulator(path)
        reports = sim.run()
        st = sim.model.getState()
        end[name] = (reports, float(np.sum(sim.grid.pv * st.p) / np.sum(sim.grid.pv)), sim.aquifers)
        sim.close()
    reports, p_aq, aqs = end["aquifers"]
    creports, p_closed, none = end["closed"]
    assert len(reports) == len(creports) == 5 and none == [] and len(aqs) == 2
    assert all("aquifers" not in r for r in creports)
    hist = np.array([r["aquifers"] for r in reports])              # [step][aquifer][W_e, W_s, p_a]
    assert hist.shape == (5, 2, 3)
    print("pore-volume weighted pressure: %.3f bar with the aquifers, %.3f bar closed; W_e per step %s" % (p_aq / 1e5, p_closed / 1e5, hist[:, :, 0].tolist()))
    assert p_aq < hist[-1, 0, 2] and p_aq < aqs[1].p_a0            # the field stays below the Fetkovich aquifer's pressure and the Carter-Tracy one's p_a0 ...
    assert np.all(np.diff(np.concatenate([np.zeros((1, 2)), hist[:, :, 0]]), axis=0) > 0)       # ... so W_e rises from step to step
    assert np.all(hist[:, :, 1] > 0) and np.all(np.diff(hist[:, :, 2], axis=0) < 0)
    assert p_aq > p_closed
