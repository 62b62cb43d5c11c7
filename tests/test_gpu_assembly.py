"""GPU parity: property evaluation, TPFA residual + 3x3-block Jacobian, convergence scalars, state update
and whole Newton iterations vs the CPU oracle, through the C ABI (B2 boundary)."""
import numpy as np
import pytest

from opmgpu import capi, decks
from opmgpu.model import GpuBlackoilModel, NumericalIssue, newton_step
from util import rel_err, slot_err

pytestmark = pytest.mark.gpu

# tolerances (north_star: "within a stated floating-point tolerance")
RTOL_JAC = 1e-11      # Jacobian blocks / residual: f64, differences = summation order + FMA contraction
P_RTOL, S_ATOL = 1e-6, 1e-6   # pressures 1e-6 relative, saturations 1e-6 absolute per Newton step


def _cases():
    act = np.random.default_rng(5).random(7 * 6 * 5) > 0.3
    # pore volumes that differ from cell to cell: the accumulation term and max |R| / pv read pv by the cell's INTERNAL row
    g = decks.cartesian_grid(7, 6, 5, lognormal_sigma=0.7)
    varied = decks.GridData(g.nc, g.conn_cells, g.trans, g.pv * np.random.default_rng(6).uniform(0.5, 2.0, g.nc), g.z, gravity=g.gravity, dims=g.dims)
    return [
        ("pv", varied, None),
        ("cart", decks.cartesian_grid(7, 6, 5, lognormal_sigma=0.7), None),
        ("nnc", decks.cartesian_grid(6, 6, 4, nnc_fraction=0.06, lognormal_sigma=0.3), None),
        ("actnum+thpres", decks.cartesian_grid(7, 6, 5, actnum=act, thpres=0.05 * decks.BAR), None),
        ("wells", decks.cartesian_grid(6, 5, 5), (np.array([0, 3, 8], np.int32), np.array([2, 32, 62, 27, 57, 87, 117, 147], np.int32))),
    ]


@pytest.mark.parametrize("ordering", [capi.ORDER_NATURAL, capi.ORDER_MULTICOLOR])
def test_assembly_parity(gpu_lib, oracle, ordering):
    tab = decks.satfunc_standard_tables()
    prm = capi.default_params(ilu_ordering=ordering)
    scale = tuple(prm.matbalscale)
    for name, grid, wells in _cases():
        for seed in (1, 2):
            st = decks.random_state(grid, tab, seed=seed)
            m = GpuBlackoilModel(grid, tab, prm, wells=wells)
            dt = 3 * decks.DAY
            m.prepareStep(dt, st)
            m.assemble(True)
            rowptr, col = oracle.pattern(grid, *(wells or (None, None)))
            r0, v0, acc0, binv = oracle.assemble(grid, tab, dt, st, rowptr, col, scale=scale)
            gr, gc, gv = m.jacobian()
            assert np.array_equal(gr, rowptr) and np.array_equal(gc, col), name
            assert rel_err(gv, v0) < RTOL_JAC, (name, rel_err(gv, v0))
            assert slot_err(gv, v0) < RTOL_JAC, (name, slot_err(gv, v0))
            assert rel_err(m.residual(), r0) < RTOL_JAC, name                 # initial: accum1 == accum0, flux part only
            # second assembly on a different state with the stored accum0 (Newton iteration > 0)
            st2 = decks.random_state(grid, tab, seed=seed + 10)
            st2.hc[:] = st.hc                                              # keep the primary-variable sets comparable
            m.setState(st2)
            m.assemble(False)
            r1, v1, _, binv1 = oracle.assemble(grid, tab, dt, st2, rowptr, col, scale=scale, accum0=acc0)
            _, _, gv1 = m.jacobian()
            assert rel_err(gv1, v1) < RTOL_JAC, (name, rel_err(gv1, v1))
            assert slot_err(gv1, v1) < RTOL_JAC, (name, slot_err(gv1, v1))
            assert rel_err(m.residual(), r1) < RTOL_JAC, (name, rel_err(m.residual(), r1))
            # convergence scalars
            so, B, CNV, MB, linf, conv = oracle.convergence(grid, prm, dt, r1, binv1)
            try:
                gconv = m.getConvergence()
                assert so == 0 and gconv == conv
            except NumericalIssue:
                assert so == capi.ENUMERICAL
            assert np.allclose(m.B_avg, B, rtol=1e-12) and np.allclose(m.CNV, CNV, rtol=1e-10) and np.allclose(m.linf, linf, rtol=1e-10)
            assert np.allclose(m.MB, MB, rtol=1e-7, atol=1e-12 * np.abs(MB).max())
            m.close()


def test_initial_residual_is_flux_only(gpu_lib, oracle):
    """With initial_assembly the accumulation difference vanishes: R = div(flux) exactly as in the oracle."""
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(6, 5, 4, lognormal_sigma=0.5)
    st = decks.initial_state(grid, tab, perturb=0.02)
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    m.prepareStep(decks.DAY, st)
    m.assemble(True)
    rowptr, col = oracle.pattern(grid)
    r0, _, _, _ = oracle.assemble(grid, tab, decks.DAY, st, rowptr, col)
    assert rel_err(m.residual(), r0) < RTOL_JAC
    m.close()


def test_update_state_parity(gpu_lib, oracle):
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(9, 8, 6)
    prm = capi.default_params()
    rng = np.random.default_rng(4)
    nc = grid.nc
    for seed in (1, 2, 3):
        st = decks.random_state(grid, tab, seed=seed)
        dx = np.concatenate([rng.standard_normal(nc) * 30 * decks.BAR, rng.standard_normal(nc) * 0.25,
                             rng.standard_normal(nc) * np.where(st.hc == capi.HC_OIL_ONLY, 30.0, np.where(st.hc == capi.HC_GAS_ONLY, 1e-4, 0.25))])
        dx[rng.random(3 * nc) < 0.1] = 0.0
        m = GpuBlackoilModel(grid, tab, prm)
        m.prepareStep(decks.DAY, st)
        m.updateState(dx)
        g, o = m.getState(), oracle.update_state(grid, tab, prm, dx, st)
        assert np.array_equal(g.hc, o.hc)
        assert np.allclose(g.p, o.p, rtol=1e-14, atol=0) and np.allclose(g.sat, o.sat, rtol=0, atol=1e-14)
        assert np.allclose(g.rs, o.rs, rtol=1e-13, atol=1e-13) and np.allclose(g.rv, o.rv, rtol=1e-13, atol=1e-18)
        m.close()


@pytest.mark.parametrize("single", [False, True])
def test_newton_iterations_parity(gpu_lib, oracle, single):
    """Whole Newton iterations (assemble -> solve -> update) GPU vs oracle.
    f64 solve: both trajectories run freely from the same start and must stay within 1e-6 (p relative,
    s absolute) after every iteration.  f32 solve (the reference's dt < 20 d mode): the attainable
    accuracy of dx is cond(A)*eps_f32, so every iteration restarts the oracle from the GPU's state and
    the increment / updated state are compared relative to the size of the increment."""
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(10, 8, 6, lognormal_sigma=0.8)
    st = decks.initial_state(grid, tab, perturb=0.01)
    red = 1e-4 if single else 1e-11            # f64: tight, so that solver noise stays below the state tolerance
    prm = capi.default_params(linear_solver_reduction=red, linear_solver_maxiter=400)
    scale = np.asarray(prm.matbalscale[:])
    dt = 5 * decks.DAY
    nc = grid.nc
    m = GpuBlackoilModel(grid, tab, prm)
    m.prepareStep(dt, st)
    rowptr, col = oracle.pattern(grid)
    pos = None
    so, acc0 = st.copy(), None
    for it in range(3):
        m.assemble(it == 0)
        m.getConvergence()
        dxg = m.solveJacobianSystem(want_dx=True, single_precision=single)
        m.updateState()
        if pos is None:
            pos = m.ordering()[0]
        r, val, acc0, binv = oracle.assemble(grid, tab, dt, so, rowptr, col, scale=tuple(scale), accum0=acc0)
        b = np.ascontiguousarray((r * np.repeat(scale, nc)).reshape(3, nc).T).ravel()
        sto, x, ito, redo, _ = oracle.bicgstab(rowptr, col, val, b, prm, position=pos, single=single)
        assert sto == 0
        dx = np.ascontiguousarray(x.reshape(nc, 3).T).ravel()
        so = oracle.update_state(grid, tab, prm, dx, so)
        g = m.getState()
        if not single:
            assert np.array_equal(g.hc, so.hc), it
            assert np.abs(g.p - so.p).max() / np.abs(so.p).max() < P_RTOL, it
            assert np.abs(g.sat - so.sat).max() < S_ATOL, it
        else:
            # f32 solve: the solver controls the residual, not the error (cond(A)*eps_f32 limits the error of
            # both implementations and depends on the rounding path).  Yardstick = the oracle's own TRUE
            # residual on the f64 system.
            from util import bsr_to_scipy
            A = bsr_to_scipy(rowptr, col, val)
            xg = np.ascontiguousarray(dxg.reshape(3, nc).T).ravel()
            res_g = np.linalg.norm(A @ xg - b) / np.linalg.norm(b)
            res_o = np.linalg.norm(A @ x - b) / np.linalg.norm(b)
            # dx solves the system to the linear tolerance -- or, where f32 rounding of the recurrence
            # residual is the limit, at least as well as the CPU f32 implementation does
            # (the f32 attainable accuracy cond(A)*eps_f32 ~ 1e-3..1e-4 here depends on the rounding path: same order of magnitude, not equal)
            assert m.linear_reduction <= red, (it, m.linear_reduction)
            assert res_g <= max(3.0 * red, 10.0 * res_o), (it, res_g, res_o)
            so = g.copy()               # restart the oracle from the device state
    m.close()


def test_newton_step_converges_and_reenters(gpu_lib):
    """NonlinearSolver::step on the device; re-entry with a rolled-back state and chopped dt
    (AdaptiveTimeStepping_impl.hpp:343-372) gives the same answer as a fresh context."""
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(12, 10, 6, lognormal_sigma=0.5)
    st = decks.initial_state(grid, tab, perturb=0.005)
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    m.prepareStep(10 * decks.DAY, st)
    n1, l1 = newton_step(m)
    assert 1 <= n1 <= 10
    m.prepareStep(3.3 * decks.DAY, st)          # rollback + dt * 0.33
    n2, l2 = newton_step(m)
    a = m.getState()
    m2 = GpuBlackoilModel(grid, tab, capi.default_params())
    m2.prepareStep(3.3 * decks.DAY, st)
    newton_step(m2)
    b = m2.getState()
    assert np.array_equal(a.p, b.p) and np.array_equal(a.sat, b.sat) and np.array_equal(a.hc, b.hc)
    m.close(); m2.close()


def test_numerical_issue_contract(gpu_lib):
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(5, 4, 3)
    st = decks.initial_state(grid, tab)
    st.p[7] = np.nan
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    m.prepareStep(decks.DAY, st)
    m.assemble(True)
    with pytest.raises(NumericalIssue):
        m.getConvergence()
    m.close()


def test_perf_props_and_well_terms(gpu_lib, oracle):
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(6, 5, 5)
    wells = (np.array([0, 3, 8], np.int32), np.array([2, 32, 62, 27, 57, 87, 117, 147], np.int32))
    st = decks.random_state(grid, tab, seed=9)
    prm = capi.default_params()
    m = GpuBlackoilModel(grid, tab, prm, wells=wells)
    m.prepareStep(decks.DAY, st)
    m.assemble(True)
    pp = m.perfProps(8).reshape(8, 9, 4)
    ref = oracle.cell_props(grid, tab, st)[wells[1]]
    names = oracle.PROP_NAMES
    for k, nm in enumerate(["p_o", "rs", "rv", "b_w", "b_o", "b_g", "mob_w", "mob_o", "mob_g"]):
        # (derivative entries that are cancellation residues -- 4e-14 next to 1e3 -- carry no relative accuracy: absolute floor per property)
        assert np.allclose(pp[:, k], ref[:, names.index(nm)], rtol=1e-11, atol=1e-13 * np.abs(ref[:, names.index(nm)]).max()), nm
    # Schur blocks / residual corrections are scattered into the right rows, scaled by matbalscale
    r0 = m.residual(); _, _, v0 = m.jacobian()
    rng = np.random.default_rng(0)
    delta = rng.standard_normal((8, 3))
    rc = np.array([[2, 32], [32, 2], [27, 147], [62, 62]], np.int32)
    blocks = rng.standard_normal((4, 9))
    m.addWellTerms(delta, rc, blocks)
    r1 = m.residual(); rowptr, col, v1 = m.jacobian()
    nc = grid.nc
    exp = r0.copy()
    for i, c in enumerate(wells[1]):
        for a in range(3):
            exp[a * nc + c] += delta[i, a]
    assert np.allclose(r1, exp, rtol=0, atol=1e-12)
    expv = v0.copy()
    sc = np.repeat(np.asarray(prm.matbalscale[:]), 3)
    for k, (r, c) in enumerate(rc):
        s = rowptr[r] + np.searchsorted(col[rowptr[r]:rowptr[r + 1]], c)
        expv[s] += blocks[k] * sc
    assert np.allclose(v1, expv, rtol=1e-13, atol=1e-13)
    m.close()


def test_dead_oil_dry_gas_tables(gpu_lib, oracle):
    """PVCDO/PVDG deck of the reference's test_boprops_ad (tests/fluid.data): no DISGAS/VAPOIL."""
    tab = decks.fluid_data_tables()
    grid = decks.cartesian_grid(5, 4, 3)
    st = decks.random_state(grid, tab, seed=2)
    st.rs[:] = 0; st.rv[:] = 0
    st.p[:] = (10 + 700 * np.random.default_rng(1).random(grid.nc)) * decks.BAR
    prm = capi.default_params()
    m = GpuBlackoilModel(grid, tab, prm)
    m.prepareStep(decks.DAY, st)
    m.assemble(True)
    rowptr, col = oracle.pattern(grid)
    r0, v0, _, _ = oracle.assemble(grid, tab, decks.DAY, st, rowptr, col, scale=tuple(prm.matbalscale))
    assert rel_err(m.jacobian()[2], v0) < RTOL_JAC and rel_err(m.residual(), r0) < RTOL_JAC
    assert slot_err(m.jacobian()[2], v0) < RTOL_JAC, slot_err(m.jacobian()[2], v0)
    m.close()


def test_endscale_assembly_and_update_parity(gpu_lib, oracle):
    """ENDSCALE (two-point end-point scaling, per-cell SWL..SOGCR): Jacobian / residual / updateState vs the oracle, whose
    scaled curves are pinned by the reference's GwsegEPS* known answers (tests/test_oracle_golden.py)."""
    tab = decks.satfunc_standard_tables(pc_scale=1.0)
    base = decks.cartesian_grid(7, 6, 5, lognormal_sigma=0.5)
    grid = decks.with_endpoints(base, decks.random_endpoints(base, seed=3))
    prm = capi.default_params()
    scale = tuple(prm.matbalscale)
    rowptr, col = oracle.pattern(grid)
    rng = np.random.default_rng(8)
    nc = grid.nc
    for seed in (1, 2):
        st = decks.random_state(grid, tab, seed=seed)
        m = GpuBlackoilModel(grid, tab, prm)
        m.prepareStep(2 * decks.DAY, st)
        m.assemble(True)
        r0, v0, _, _ = oracle.assemble(grid, tab, 2 * decks.DAY, st, rowptr, col, scale=scale)
        # the scaling must matter for this to be a test of it
        r_plain, v_plain, _, _ = oracle.assemble(base, tab, 2 * decks.DAY, st, rowptr, col, scale=scale)
        assert rel_err(v_plain, v0) > 1e-3
        assert rel_err(m.jacobian()[2], v0) < RTOL_JAC, rel_err(m.jacobian()[2], v0)
        assert slot_err(m.jacobian()[2], v0) < RTOL_JAC, slot_err(m.jacobian()[2], v0)
        assert rel_err(m.residual(), r0) < RTOL_JAC
        dx = np.concatenate([rng.standard_normal(nc) * 30 * decks.BAR, rng.standard_normal(nc) * 0.25,
                             rng.standard_normal(nc) * np.where(st.hc == capi.HC_OIL_ONLY, 30.0, np.where(st.hc == capi.HC_GAS_ONLY, 1e-4, 0.25))])
        m.updateState(dx)
        g, o = m.getState(), oracle.update_state(grid, tab, prm, dx, st)
        assert np.array_equal(g.hc, o.hc)
        assert np.allclose(g.p, o.p, rtol=1e-14, atol=0) and np.allclose(g.sat, o.sat, rtol=0, atol=1e-14)
        assert np.allclose(g.rs, o.rs, rtol=1e-13, atol=1e-13) and np.allclose(g.rv, o.rv, rtol=1e-13, atol=1e-18)
        m.close()


def test_endscale_known_answers_on_device(gpu_lib):
    """The reference's GwsegEPS_A known answers (tests/test_satfunc.cpp:227-307) checked on the DEVICE path directly, without
    the oracle: kr = mobility * mu from opmgpu_perf_props.  mu_w, mu_o are constant here (no capillary pressure, one pressure,
    one undersaturated rs) and are read off an unscaled twin model where kr is a plain table value (GwsegEPSBase)."""
    import json
    import os
    G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "satfunc_eps.json")))["cases"]
    A, B = G["GwsegEPS_A"], G["GwsegEPSBase"]
    # tables, column grid and per-cell end points straight from the reference's deck file (fixture copy), capillary pressure zeroed
    from opmgpu import deck
    d = deck.read_deck(os.path.join(os.path.dirname(__file__), "golden", "decks", "satfuncEPS_A.DATA"))
    tab = d.tables()
    tab.swof_pcow[:] = 0.0; tab.sgof_pcgo[:] = 0.0
    full = d.grid()
    g0 = decks.cartesian_grid(1, 1, 8)
    eps = {k: full.eps[i][:8] for i, k in enumerate(decks.GridData.EPS_NAMES)}
    for k, v in A["endpoints"].items():
        assert np.array_equal(eps[k], np.asarray(v, float)[:8]), k
    wells = (np.array([0, 8], np.int32), np.arange(8, dtype=np.int32))
    prm = capi.default_params()

    def state(sw):
        return decks.State(np.full(8, 200 * decks.BAR), np.tile([sw, 1.0 - sw, 0.0], (8, 1)), np.full(8, 10.0), np.zeros(8),
                           np.full(8, capi.HC_OIL_ONLY, np.int8))

    def perf(m, sw):
        m.prepareStep(decks.DAY, state(sw))
        return m.perfProps(8).reshape(8, 9, 4)        # p rs rv b_w b_o b_g mob_w mob_o mob_g, each (v, d/dP, d/dSw, d/dX)

    plain = GpuBlackoilModel(g0, tab, prm, wells=wells)
    mu_w = B["krw"][10] / perf(plain, 1.0)[0, 6, 0]
    mu_o = B["kro"][1] / perf(plain, 0.1)[0, 7, 0]
    plain.close()
    m = GpuBlackoilModel(decks.with_endpoints(g0, eps), tab, prm, wells=wells)
    tol = A["reltol_percent"] / 100.0

    def close(a, b):
        return abs(a - b) <= tol * max(abs(a), abs(b)) or (abs(a) < 1e-14 and abs(b) < 1e-14)

    for i in range(11):
        pp = perf(m, 0.1 * i)
        for c in range(8):
            assert close(pp[c, 6, 0] * mu_w, A["krw"][c][i]), (c, i, "krw", pp[c, 6, 0] * mu_w, A["krw"][c][i])
            assert close(pp[c, 7, 0] * mu_o, A["kro"][c][i]), (c, i, "kro", pp[c, 7, 0] * mu_o, A["kro"][c][i])
            assert close(pp[c, 6, 2] * mu_w, A["DkrwDsw"][c][i]), (c, i, "DkrwDsw", pp[c, 6, 2] * mu_w, A["DkrwDsw"][c][i])
            assert close(pp[c, 7, 2] * mu_o, A["DkroDsw"][c][i]), (c, i, "DkroDsw", pp[c, 7, 2] * mu_o, A["DkroDsw"][c][i])
    m.close()


def test_stabilize_update_dampen_and_sor(gpu_lib, oracle):
    """stabilizeNonlinearUpdate (NonlinearSolver_impl.hpp:260-301) on the resident increment, observed through updateState."""
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(6, 5, 4)
    prm = capi.default_params()
    rng = np.random.default_rng(11)
    nc = grid.nc
    st = decks.random_state(grid, tab, seed=3)

    def rand_dx():
        return np.concatenate([rng.standard_normal(nc) * 5 * decks.BAR, rng.standard_normal(nc) * 0.05,
                               rng.standard_normal(nc) * np.where(st.hc == capi.HC_OIL_ONLY, 5.0, np.where(st.hc == capi.HC_GAS_ONLY, 1e-5, 0.05))])

    def check(m, dx_expected):
        m.setState(st)
        m.updateState()
        g, o = m.getState(), oracle.update_state(grid, tab, prm, dx_expected, st)
        assert np.array_equal(g.hc, o.hc)
        assert np.allclose(g.p, o.p, rtol=1e-13, atol=0) and np.allclose(g.sat, o.sat, rtol=0, atol=1e-13)

    for rtype in (capi.RELAX_DAMPEN, capi.RELAX_SOR):
        m = GpuBlackoilModel(grid, tab, prm)
        m.prepareStep(decks.DAY, st)
        m.assemble(True)                                   # iteration 0 zeroes dx_old
        dx1, dx2 = rand_dx(), rand_dx()
        m.updateState(dx1)
        m.stabilizeUpdate(rtype, 1.0)                      # omega == 1: dx untouched, dx_old <- dx1
        check(m, dx1)
        m.updateState(dx2)
        m.stabilizeUpdate(rtype, 0.6)
        check(m, 0.6 * dx2 if rtype == capi.RELAX_DAMPEN else 0.6 * dx2 + 0.4 * dx1)
        m.close()


def test_cpp_host_mirror_runs_a_time_step(gpu_lib):
    """The C++ mirror (host/opmgpu.hpp: BlackoilModelGpu + NonlinearSolverGpu) drives one time step of a hand-authored
    dead-oil deck through the C ABI -- the binding a flow_legacy maintainer would compile."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "host_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host_check: converged in" in out.stdout and "host_check: report step of 20 d in" in out.stdout and "one-call Newton loop" in out.stdout and "RESV coefficients" in out.stdout, out.stdout
    assert "host_check: fluids in place" in out.stdout, out.stdout          # BlackoilModelGpu::computeFluidInPlace


def test_vappars_rocktab_parity(gpu_lib, oracle):
    """VAPPARS (applyVap, BlackoilPropsAdFromDeck.cpp:1052-1078) and ROCKTAB (RockCompressibility.cpp:86-125): assembly and
    updateState vs the oracle, soMax handling (updateSatOilMax, :933-945) included."""
    rocktab = [(100.0, 0.98, 0.95), (200.0, 1.0, 1.0), (300.0, 1.03, 1.08), (500.0, 1.05, 1.12)]
    plain = decks.satfunc_standard_tables()
    tab = decks.satfunc_standard_tables(vappars=(0.7, 1.3), rocktab=rocktab)
    grid = decks.cartesian_grid(7, 6, 5, lognormal_sigma=0.5)
    prm = capi.default_params()
    scale = tuple(prm.matbalscale)
    rowptr, col = oracle.pattern(grid)
    rng = np.random.default_rng(21)
    nc = grid.nc
    try:
        for seed in (1, 2):
            st = decks.random_state(grid, tab, seed=seed)
            m = GpuBlackoilModel(grid, tab, prm)
            m.prepareStep(2 * decks.DAY, st)
            assert np.all(m.satOilMax() == 0.0)                       # starts at zero like the reference's
            m.updateSatOilMax()
            assert np.array_equal(m.satOilMax(), st.sat[:, 1])        # first report step: soMax = so
            so_max = np.maximum(st.sat[:, 1], rng.uniform(0.2, 0.9, nc))
            m.setSatOilMax(so_max)
            m.updateSatOilMax()
            assert np.array_equal(m.satOilMax(), so_max)
            oracle.set_sat_oil_max(so_max)
            m.assemble(True)
            r0, v0, _, _ = oracle.assemble(grid, tab, 2 * decks.DAY, st, rowptr, col, scale=scale)
            oracle.set_sat_oil_max(None)
            r_plain, v_plain, _, _ = oracle.assemble(grid, plain, 2 * decks.DAY, st, rowptr, col, scale=scale)
            oracle.set_sat_oil_max(so_max)
            assert rel_err(v_plain, v0) > 1e-3                        # the keywords matter for this state
            assert rel_err(m.jacobian()[2], v0) < RTOL_JAC, rel_err(m.jacobian()[2], v0)
            assert slot_err(m.jacobian()[2], v0) < RTOL_JAC, slot_err(m.jacobian()[2], v0)
            assert rel_err(m.residual(), r0) < RTOL_JAC
            dx = np.concatenate([rng.standard_normal(nc) * 30 * decks.BAR, rng.standard_normal(nc) * 0.25,
                                 rng.standard_normal(nc) * np.where(st.hc == capi.HC_OIL_ONLY, 30.0, np.where(st.hc == capi.HC_GAS_ONLY, 1e-4, 0.25))])
            m.updateState(dx)
            g, o = m.getState(), oracle.update_state(grid, tab, prm, dx, st)
            assert np.array_equal(g.hc, o.hc)
            assert np.allclose(g.p, o.p, rtol=1e-14, atol=0) and np.allclose(g.sat, o.sat, rtol=0, atol=1e-14)
            assert np.allclose(g.rs, o.rs, rtol=1e-12, atol=1e-12) and np.allclose(g.rv, o.rv, rtol=1e-12, atol=1e-17)
            # wells re-plan keeps soMax
            m.setWells(np.array([0, 3], np.int32), np.array([2, 44, 86], np.int32))
            assert np.array_equal(m.satOilMax(), so_max)
            m.close()
    finally:
        oracle.set_sat_oil_max(None)


def test_float_assembly_for_a_float_solve(gpu_lib, oracle):
    """opmgpu_set_solve_precision(1): the Jacobian is written as float by the assembly kernels themselves (no f64 copy, no
    conversion pass).  Values = the f64 Jacobian rounded to float; the residual stays f64; a Newton iteration through this
    path lands where the f64-assembly + conversion path lands (same f32 system up to the rounding of the diagonal seed)."""
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(8, 7, 5, lognormal_sigma=0.6)
    st = decks.initial_state(grid, tab, perturb=0.01)
    prm = capi.default_params(linear_solver_reduction=1e-5, linear_solver_maxiter=300)
    rowptr, col = oracle.pattern(grid)
    dt = 5 * decks.DAY
    r0, v0, _, _ = oracle.assemble(grid, tab, dt, st, rowptr, col, scale=tuple(prm.matbalscale))
    a = GpuBlackoilModel(grid, tab, prm)
    a.prepareStep(dt, st)
    a.setSolvePrecision(True)
    a.assemble(True)
    _, _, va = a.jacobian()
    assert rel_err(va, v0) < 2e-7 and np.abs(va - v0.astype(np.float32)).max() <= 2e-7 * np.abs(v0).max()
    assert rel_err(a.residual(), r0) < RTOL_JAC
    b = GpuBlackoilModel(grid, tab, prm)
    b.prepareStep(dt, st)
    b.setSolvePrecision(False)
    b.assemble(True)
    for m in (a, b):
        m.getConvergence()
        m.solveJacobianSystem(single_precision=True)
        m.updateState()
    sa, sb = a.getState(), b.getState()
    assert np.array_equal(sa.hc, sb.hc)
    # two f32 systems that differ by one rounding of the entries: the solutions differ by cond(A) * eps_f32 (the pressure level of
    # a closed, nearly incompressible system is the badly conditioned mode) -- the same size as either one's distance to the f64 solve
    c = GpuBlackoilModel(grid, tab, prm)
    c.prepareStep(dt, st); c.assemble(True); c.getConvergence(); c.solveJacobianSystem(single_precision=False); c.updateState()
    sc_ = c.getState()
    c.close()
    ea, eb = np.abs(sa.p - sc_.p).max(), np.abs(sb.p - sc_.p).max()
    assert ea <= 5e-4 * np.abs(sc_.p).max() and eb <= 5e-4 * np.abs(sc_.p).max(), (ea, eb)
    assert np.abs(sa.sat - sc_.sat).max() <= 1e-4 and np.abs(sa.sat - sb.sat).max() <= 1e-4
    # a double solve after a float assembly works on the widened values
    a.setState(st); a.setSolvePrecision(True); a.assemble(True); a.getConvergence()
    a.solveJacobianSystem(single_precision=False)
    a.close(); b.close()


@pytest.mark.parametrize("case", ["scalecrs", "vertical", "hysteresis", "all"])
def test_satfunc_options_parity(gpu_lib, oracle, case):
    """SURVEY row a5 beyond two-point ENDSCALE -- three-point scaling (SCALECRS), vertical scaling (KRW / KRO / KRG / PCW / PCG) and
    Carlson relative-permeability hysteresis (IMBNUM regions, history on the device) -- device assembly, hysteresis update and
    updateState against the oracle (whose options are checked against their defining properties in tests/test_satfunc_options.py)."""
    from test_satfunc_options import _hyst_tables
    tab = _hyst_tables()                                   # region 0 = drainage curves, region 1 = imbibition curves
    base = decks.cartesian_grid(7, 6, 5, lognormal_sigma=0.5)
    nc = base.nc
    rng = np.random.default_rng(5)
    eps = decks.random_endpoints(base, seed=3)
    eps["SOWCR"] = np.clip(eps["SOWCR"] + 0.08, 0.0, 0.5); eps["SOGCR"] = np.clip(eps["SOGCR"] + 0.05, 0.0, 0.5)
    kw = {}
    if case in ("scalecrs", "all"):
        kw["scalecrs"] = True
    if case in ("vertical", "all"):
        kw["eps_v"] = {"KRW": rng.uniform(0.3, 0.9, nc), "KRO": rng.uniform(0.6, 1.0, nc), "KRG": rng.uniform(0.5, 1.0, nc),
                       "PCW": rng.uniform(0.5, 2.0, nc) * decks.BAR, "PCG": rng.uniform(1.0, 3.0, nc) * decks.BAR}
    if case in ("hysteresis", "all"):
        kw["imbnum"] = np.ones(nc, np.int32)
        if case == "all":
            ie = decks.random_endpoints(base, seed=4)
            ie["SGCR"] = np.clip(ie["SGCR"] + 0.15, 0.0, 0.6)
            kw["ieps"] = ie
    if case == "hysteresis":                               # hysteresis alone: no end-point scaling at all
        grid = decks.GridData(nc, base.conn_cells, base.trans, base.pv, base.z, dims=base.dims, satnum=np.zeros(nc, np.int32), imbnum=kw["imbnum"])
    else:
        grid = decks.with_endpoints(base, eps, **kw)
    prm = capi.default_params()
    scale = tuple(prm.matbalscale)
    rowptr, col = oracle.pattern(grid)
    hist = oracle.Hysteresis(nc) if "imbnum" in kw else None
    oracle.set_hysteresis(hist)
    try:
        m = GpuBlackoilModel(grid, tab, prm)
        for seed in (1, 2, 3):
            st = decks.random_state(grid, tab, seed=seed)
            m.prepareStep(2 * decks.DAY, st)
            if hist is not None:                           # the state becomes history (start of a report step), then a NEW state is evaluated
                m.updateHysteresis()
                hist.update(grid, tab, st.sat)
                got = m.getHysteresis()
                for a, b in zip(got, (hist.mdc_ow, hist.mdc_go, hist.d_ow, hist.d_go)):
                    assert np.allclose(a, b, rtol=1e-13, atol=1e-15)
                assert np.abs(hist.d_go).max() > 1e-3 and np.abs(hist.d_ow).max() > 1e-3
                st = decks.random_state(grid, tab, seed=10 + seed)
                m.prepareStep(2 * decks.DAY, st)
                on_imb = ((1.0 - st.sat[:, 2]) > hist.mdc_go).mean()
                assert 0.05 < on_imb < 0.95                # both branches occur
            m.assemble(True)
            r0, v0, _, _ = oracle.assemble(grid, tab, 2 * decks.DAY, st, rowptr, col, scale=scale)
            assert rel_err(m.jacobian()[2], v0) < RTOL_JAC, (case, seed, rel_err(m.jacobian()[2], v0))
            assert slot_err(m.jacobian()[2], v0) < RTOL_JAC, (case, seed, slot_err(m.jacobian()[2], v0))
            assert rel_err(m.residual(), r0) < RTOL_JAC
            dx = np.concatenate([rng.standard_normal(nc) * 30 * decks.BAR, rng.standard_normal(nc) * 0.25,
                                 rng.standard_normal(nc) * np.where(st.hc == capi.HC_OIL_ONLY, 30.0, np.where(st.hc == capi.HC_GAS_ONLY, 1e-4, 0.25))])
            m.updateState(dx)
            g, o = m.getState(), oracle.update_state(grid, tab, prm, dx, st)
            assert np.array_equal(g.hc, o.hc)
            assert np.allclose(g.p, o.p, rtol=1e-14, atol=0) and np.allclose(g.sat, o.sat, rtol=0, atol=1e-14)
        if hist is not None:                               # restart: set the history, the shifts follow
            m2 = GpuBlackoilModel(grid, tab, prm)
            m2.prepareStep(2 * decks.DAY, st)
            m2.setHysteresis(hist.mdc_ow, hist.mdc_go)
            for a, b in zip(m2.getHysteresis(), (hist.mdc_ow, hist.mdc_go, hist.d_ow, hist.d_go)):
                assert np.allclose(a, b, rtol=1e-13, atol=1e-15)
            m2.close()
        # the options matter: without them the Jacobian differs
        plain = decks.with_endpoints(base, eps) if case != "hysteresis" else decks.GridData(nc, base.conn_cells, base.trans, base.pv, base.z, dims=base.dims)
        oracle.set_hysteresis(None)
        _, v_plain, _, _ = oracle.assemble(plain, tab, 2 * decks.DAY, st, rowptr, col, scale=scale)
        assert rel_err(v_plain, v0) > 1e-4
        m.close()
    finally:
        oracle.set_hysteresis(None)


@pytest.mark.parametrize("single", [False, True])
def test_update_equations_scaling(gpu_lib, oracle, single):
    """BlackoilModelBase::updateEquationsScaling (BlackoilModelBase_impl.hpp:909, :919-947; default off): matbalscale[a] = mean over the cells
    of 1 / b_a of the state being assembled; the system of THAT assembly is scaled with it (the reference's linear solver reads
    residual.matbalscale after assemble).  Device factors == the oracle's cell properties; Jacobian and right-hand side carry them."""
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(7, 6, 4, lognormal_sigma=0.6, seed=3)
    st = decks.random_state(grid, tab, seed=5)
    prm = capi.default_params(update_equations_scaling=1, linear_solver_reduction=1e-10, linear_solver_maxiter=400)
    m = GpuBlackoilModel(grid, tab, prm)
    dt = 2 * decks.DAY
    m.prepareStep(dt, st)
    m.setSolvePrecision(single)
    for initial, state in ((True, st), (False, decks.random_state(grid, tab, seed=6))):
        if not initial:
            state.hc[:] = st.hc
            m.setState(state)
        m.assemble(initial)
        props = oracle.cell_props(grid, tab, state)
        want = np.array([np.mean(1.0 / props[:, oracle.PROP_NAMES.index("b_" + c), 0]) for c in "wog"])
        got = np.zeros(3)
        m._chk(m.lib.opmgpu_get_matbalscale(m.ctx, capi.dptr(got)))
        assert np.allclose(got, want, rtol=1e-13), (got, want)
        rowptr, col = oracle.pattern(grid)
        if initial:
            r, v, acc0, _ = oracle.assemble(grid, tab, dt, state, rowptr, col, scale=tuple(want))
        else:
            r, v, _, _ = oracle.assemble(grid, tab, dt, state, rowptr, col, scale=tuple(want), accum0=acc0)
        _, _, gv = m.jacobian()
        assert rel_err(gv, v) < (2e-6 if single else RTOL_JAC)
        assert slot_err(gv, v) < (2e-6 if single else RTOL_JAC), slot_err(gv, v)
        assert rel_err(m.residual(), r) < RTOL_JAC             # the residual itself is unscaled
    # the solve uses the same factors for the right-hand side: its dx solves the oracle's scaled system
    m.getConvergence()
    dx = m.solveJacobianSystem(want_dx=True, single_precision=False) if not single else None
    if dx is not None:
        nc = grid.nc
        b = np.ascontiguousarray((r * np.repeat(want, nc)).reshape(3, nc).T).ravel()
        y = oracle.spmv(rowptr, col, v, np.ascontiguousarray(dx.reshape(3, nc).T).ravel())
        assert np.abs(y - b).max() <= 1e-7 * np.abs(b).max()
    m.close()
    # off (the default): the constants of BlackoilModelBase_impl.hpp:139 stay
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    m.prepareStep(dt, st); m.assemble(True)
    got = np.zeros(3)
    m._chk(m.lib.opmgpu_get_matbalscale(m.ctx, capi.dptr(got)))
    assert np.array_equal(got, [1.1169, 1.0031, 0.0031])
    m.close()


def test_compute_fluid_in_place(gpu_lib, oracle):
    """BlackoilModelBase::computeFluidInPlace (BlackoilModelBase_impl.hpp:2263-2445, serial branch) for the resident state against a numpy
    restatement on the oracle's cell properties: fip[phase] = pv_mult b s pv per cell, rs / rv volumes, and per region the sums, the pore
    volume and the hydrocarbon-pore-volume weighted pressure -- with cells outside every region (fipnum 0) and a region without
    hydrocarbons (the reference's pres / pv branch, :2358-2360)."""
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(7, 6, 5, lognormal_sigma=0.6, seed=3)
    st = decks.random_state(grid, tab, seed=11)
    nc = grid.nc
    water = np.arange(nc) < 12                       # region 1: water only
    st.sat[water] = [1.0, 0.0, 0.0]
    rng = np.random.default_rng(4)
    fipnum = rng.choice([0, 2, 3], nc).astype(np.int32)
    fipnum[water] = 1
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    m.prepareStep(1 * decks.DAY, st)
    values, cells = m.computeFluidInPlace(fipnum, cells=True)
    # numpy restatement
    props = oracle.cell_props(grid, tab, st)
    nm = oracle.PROP_NAMES
    b = [props[:, nm.index("b_" + a), 0] for a in "wog"]
    assert tab.rocktab_n == 0
    cp = tab.rock_comp * (st.p - tab.rock_pref)
    pvm = 1.0 + cp + 0.5 * cp * cp
    pv = np.asarray(grid.pv)
    fip = np.zeros((7, nc))
    for a in range(3):
        fip[a] = ((pvm * b[a]) * st.sat[:, a]) * pv
    fip[3], fip[4] = st.rs * fip[1], st.rv * fip[2]
    dims = int(fipnum.max())
    expect = np.zeros((dims, 7))
    hyd = st.sat[:, 1] + st.sat[:, 2]
    hcpv, pres = np.zeros(dims), np.zeros(dims)
    for c in range(nc):
        r = fipnum[c] - 1
        if r == -1:
            continue
        expect[r, :5] += fip[:5, c]
        hcpv[r] += pv[c] * hyd[c]
        pres[r] += pv[c] * st.p[c]
    for c in range(nc):
        r = fipnum[c] - 1
        if r == -1:
            continue
        fip[5, c] = pv[c]
        fip[6, c] = pv[c] * st.p[c] * hyd[c] / hcpv[r] if hcpv[r] != 0 else pres[r] / pv[c]
        expect[r, 5] += fip[5, c]
        expect[r, 6] += fip[6, c]
    assert hcpv[0] == 0.0 and (hcpv[1:] > 0).all() and (fipnum == 0).any()
    assert np.allclose(values, expect, rtol=1e-11, atol=0.0), (values, expect)
    assert np.allclose(cells, fip, rtol=1e-11, atol=1e-300)
    # one region of all cells
    v1 = m.computeFluidInPlace()
    assert v1.shape == (1, 7) and np.allclose(v1[0, :5], fip[:5].sum(1), rtol=1e-11) and np.isclose(v1[0, 5], pv.sum(), rtol=1e-13)
    # regions outside the declared range are refused
    import ctypes as C
    out = np.zeros((2, 7))
    assert m.lib.opmgpu_compute_fluid_in_place(m.ctx, capi.iptr(fipnum), 2, None, capi.dptr(out)) == capi.EINVAL
    m.close()


def test_table_set_too_large_for_lds(gpu_lib):
    """A table set past the 24 KiB the property kernels stage in LDS: they then read the tables from the device blob instead, a path
    of its own in the value pass, the row assembly and updateState.  24 IDENTICAL PVT and saturation regions with random PVTNUM / SATNUM
    must give what the single-region set gives, whatever path reads them: Jacobian and residual within RTOL_JAC, the updated state
    within the bounds of test_update_state_parity with hc exactly equal, the perforation PVT and the voidage coefficients within
    RTOL_JAC (f64 evaluation of equal tables: what may differ is FMA contraction between the instantiations)."""
    R = 24
    one, many = decks.satfunc_standard_tables(), decks.satfunc_standard_tables(regions=R)
    # the device blob holds at least the caller's float64 arrays (then the index arrays and the slopes)
    assert sum(a.nbytes for a in vars(many).values() if isinstance(a, np.ndarray) and a.dtype == np.float64) > 24 * 1024
    assert sum(a.nbytes for a in vars(one).values() if isinstance(a, np.ndarray)) * 2 < 24 * 1024      # the single set fits, slopes included
    g1 = decks.cartesian_grid(7, 6, 5, lognormal_sigma=0.7)
    nc = g1.nc
    rng = np.random.default_rng(12)
    gR = decks.GridData(nc, g1.conn_cells, g1.trans, g1.pv, g1.z, gravity=g1.gravity, dims=g1.dims,
                        pvtnum=rng.integers(0, R, nc), satnum=rng.integers(0, R, nc))
    assert len(set(gR.pvtnum)) > 1 and len(set(gR.satnum)) > 1 and (gR.pvtnum != gR.satnum).any()
    wells = (np.array([0, 3, 8], np.int32), np.array([2, 32, 62, 27, 57, 87, 117, 147], np.int32))
    prm = capi.default_params()
    n = 16
    vp, vrs, vrv = capi.f64((60 + 380 * rng.random(n)) * decks.BAR), capi.f64(250 * rng.random(n)), capi.f64(5e-4 * rng.random(n))
    for seed in (1, 2):
        st = decks.random_state(g1, one, seed=seed)
        dx = np.concatenate([rng.standard_normal(nc) * 30 * decks.BAR, rng.standard_normal(nc) * 0.25,
                             rng.standard_normal(nc) * np.where(st.hc == capi.HC_OIL_ONLY, 30.0, np.where(st.hc == capi.HC_GAS_ONLY, 1e-4, 0.25))])
        dx[rng.random(3 * nc) < 0.1] = 0.0
        press = (60 + 380 * rng.random(8)) * decks.BAR
        got = []
        for grid, tab in ((g1, one), (gR, many)):
            m = GpuBlackoilModel(grid, tab, prm, wells=wells)
            m.prepareStep(3 * decks.DAY, st)
            m.assemble(True)
            jac, res = m.jacobian()[2], m.residual()
            b, rs_sat, rv_sat = m.perfPvtAt(press)
            coeff = np.zeros((n, 3))
            reg = capi.i32(rng.integers(0, tab.n_pvt, n))
            m._chk(m.lib.opmgpu_voidage_coefficients(m.ctx, n, capi.dptr(vp), capi.dptr(vrs), capi.dptr(vrv), capi.iptr(reg), capi.dptr(coeff)))
            m.updateState(dx)
            got.append((jac, res, np.column_stack([b, rs_sat, rv_sat]), coeff, m.getState()))
            m.close()
        (j1, r1, pvt1, c1, s1), (jR, rR, pvtR, cR, sR) = got
        assert rel_err(jR, j1) < RTOL_JAC and rel_err(rR, r1) < RTOL_JAC, seed
        assert slot_err(jR, j1) < RTOL_JAC, (seed, slot_err(jR, j1))
        for k in range(5):
            assert rel_err(pvtR[:, k], pvt1[:, k]) < RTOL_JAC, (seed, k)
        assert rel_err(cR, c1) < RTOL_JAC, seed
        assert np.array_equal(sR.hc, s1.hc)
        assert np.allclose(sR.p, s1.p, rtol=1e-14, atol=0) and np.allclose(sR.sat, s1.sat, rtol=0, atol=1e-14)
        assert np.allclose(sR.rs, s1.rs, rtol=1e-13, atol=1e-13) and np.allclose(sR.rv, s1.rv, rtol=1e-13, atol=1e-18)
