"""Well-coupled Newton iterations: the device model and the CPU oracle driven by the SAME host well model
(opmgpu/wells.py) must walk the same Newton path on the SPE1-like deck (BASELINE configs[0])."""
import numpy as np
import pytest

from opmgpu import capi, decks, wells as W
from opmgpu.model import GpuBlackoilModel
from test_wells_host import _setup
from util import OracleBackend

pytestmark = pytest.mark.gpu


def test_well_coupled_newton_parity(gpu_lib, oracle):
    grid, tab, st, wl = _setup()
    prm = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500)
    dt = 2 * decks.DAY
    gm = GpuBlackoilModel(grid, tab, prm, wells=wl.arrays())
    ob = OracleBackend(oracle, grid, tab, prm, wells=wl.arrays())
    ob.position = gm.ordering()[0]
    mg = W.WellCoupledModel(gm, W.StandardWellsHost(wl, grid.z, tab.surface_density[0]), W.WellState(wl, st.p))
    mo = W.WellCoupledModel(ob, W.StandardWellsHost(wl, grid.z, tab.surface_density[0]), W.WellState(wl, st.p))
    mg.prepareStep(dt, st); mo.prepareStep(dt, st)
    for step in range(2):
        it = 0
        while True:
            cg, lg = mg.nonlinearIteration(it, single_precision=False)
            co, lo = mo.nonlinearIteration(it, single_precision=False)
            assert cg == co, (step, it)
            it += 1
            a, b = gm.getState(), ob.getState()
            assert np.array_equal(a.hc, b.hc), (step, it)
            assert np.abs(a.p - b.p).max() <= 1e-6 * np.abs(b.p).max(), (step, it)
            assert np.abs(a.sat - b.sat).max() <= 1e-6, (step, it)
            assert np.allclose(mg.ws.bhp, mo.ws.bhp, rtol=1e-7) and np.allclose(mg.ws.qs, mo.ws.qs, rtol=1e-6, atol=1e-9 * np.abs(mo.ws.qs).max())
            assert np.allclose(gm.CNV, ob.CNV, rtol=1e-5, atol=1e-9) and np.allclose(mg.wh.flux_eq, mo.wh.flux_eq, rtol=1e-5, atol=1e-12)
            if cg and it >= 1:
                break
            assert it <= 12
        mg.prepareStep(dt); mo.prepareStep(dt)
    assert mg.ws.qs[0, 0] > 0 and mg.ws.qs[1, 1] < 0
    gm.close()


@pytest.mark.parametrize("cpr", [0, 1])
def test_device_wells_match_host_wells_on_the_oracle(gpu_lib, oracle, cpr):
    """Wells ON THE DEVICE (csrc/wells.hip: factored Schur complement, rank-7 operator per well inside the SpMV) vs the CPU
    oracle driven by the host well model with the explicit Schur complement: same Newton path, same well state."""
    grid, tab, st, wl = _setup()
    prm = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500, cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=cpr)
    prm_o = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500)
    dt = 2 * decks.DAY
    gm = GpuBlackoilModel(grid, tab, prm)
    ob = OracleBackend(oracle, grid, tab, prm_o, wells=wl.arrays())
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    mo = W.WellCoupledModel(ob, W.StandardWellsHost(wl, grid.z, tab.surface_density[0]), W.WellState(wl, st.p))
    md.prepareStep(dt, st); mo.prepareStep(dt, st)
    for step in range(2):
        it = 0
        while True:
            cd, ld = md.nonlinearIteration(it, single_precision=False)
            co, lo = mo.nonlinearIteration(it, single_precision=False)
            assert cd == co, (step, it)
            assert np.allclose(md.well_flux_residual, mo.wh.well_flux_residual, rtol=1e-5, atol=1e-12), (step, it)
            assert md.well_ctrl_residual == pytest.approx(mo.wh.well_ctrl_residual, rel=1e-5, abs=1e-12)
            it += 1
            a, b = gm.getState(), ob.getState()
            ws = md.pull_well_state()
            assert np.array_equal(a.hc, b.hc), (step, it)
            assert np.abs(a.p - b.p).max() <= 1e-6 * np.abs(b.p).max(), (step, it)
            assert np.abs(a.sat - b.sat).max() <= 1e-6, (step, it)
            assert np.allclose(ws.bhp, mo.ws.bhp, rtol=1e-7), (step, it, ws.bhp, mo.ws.bhp)
            assert np.allclose(ws.qs, mo.ws.qs, rtol=1e-6, atol=1e-9 * np.abs(mo.ws.qs).max()), (step, it)
            assert np.allclose(ws.perf_rates, mo.ws.perf_rates, rtol=1e-6, atol=1e-9 * np.abs(mo.ws.perf_rates).max())
            assert np.allclose(gm.CNV, ob.CNV, rtol=1e-5, atol=1e-9)
            if cd and it >= 1:
                break
            assert it <= 12
        md.prepareStep(dt); mo.prepareStep(dt)
    assert ws.qs[0, 0] > 0 and ws.qs[1, 1] < 0
    gm.close()


@pytest.mark.parametrize("single", [False, True])
def test_device_wells_five_spot_vs_host_wells(gpu_lib, single):
    """5-spot with full-column wells (SURVEY 8d synthetic wells) on a deck with all three hydrocarbon states: the device well
    model against the host well model (explicit cliques), both on the GPU reservoir path, tight linear tolerance."""
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(9, 9, 12, lognormal_sigma=0.5)
    st = decks.initial_state(grid, tab, perturb=0.002)
    wl = W.five_spot(grid, rate_m3_per_day=40.0, bhp_prod_bar=150.0)
    red = 1e-6 if single else 1e-11
    prm = capi.default_params(linear_solver_reduction=red, linear_solver_maxiter=500)
    dt = 1 * decks.DAY
    gh = GpuBlackoilModel(grid, tab, prm, wells=wl.arrays())
    gd = GpuBlackoilModel(grid, tab, prm)
    mh = W.WellCoupledModel(gh, W.StandardWellsHost(wl, grid.z, tab.surface_density[0]), W.WellState(wl, st.p))
    md = W.DeviceWellModel(gd, wl, W.WellState(wl, st.p))
    mh.prepareStep(dt, st); md.prepareStep(dt, st)
    tol_p, tol_s = (1e-4, 1e-4) if single else (1e-6, 1e-6)        # f32: two different f32 systems (explicit clique vs factored operator, float assembly)
    for step in range(2):
        it = 0
        while True:
            ch, _ = mh.nonlinearIteration(it, single_precision=single)
            cd, _ = md.nonlinearIteration(it, single_precision=single)
            it += 1
            a, b = gd.getState(), gh.getState()
            ws = md.pull_well_state()
            assert np.array_equal(a.hc, b.hc), (step, it)
            assert np.abs(a.p - b.p).max() <= tol_p * np.abs(b.p).max(), (step, it, np.abs(a.p - b.p).max() / np.abs(b.p).max())
            assert np.abs(a.sat - b.sat).max() <= tol_s, (step, it)
            assert np.allclose(ws.bhp, mh.ws.bhp, rtol=10 * tol_p), (step, it)
            assert np.allclose(ws.qs, mh.ws.qs, rtol=0, atol=50 * tol_p * np.abs(mh.ws.qs).max()), (step, it)
            if not single:
                assert ch == cd, (step, it)
            if (ch and cd and it >= 1) or it > 12:
                break
        assert it <= 12
        mh.prepareStep(dt); md.prepareStep(dt)
    assert ws.qs[0, 0] > 0 and (ws.qs[1:, 1] < 0).all()
    gh.close(); gd.close()


def test_waterflood_material_balance_through_adaptive_stepping(gpu_lib, oracle):
    """End to end on the device: SPE1-like deck, device wells, NonlinearSolver with update stabilisation, AdaptiveTimeStepping over
    a 30-day report step.  Physics check that needs no reference solver: for every converged sub-step the change of each
    component's surface volume in place equals dt times the wells' surface rates (implicit Euler), to the Newton tolerance."""
    from opmgpu import timestepping as ts
    from opmgpu.model import NonlinearSolver
    grid, tab, st, wl = _setup()
    # tight tolerances: the default ones (MB 1e-5 of the pore volume, wells 1e-4 m3/s) allow hundreds of m3 of imbalance per step
    prm = capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, tolerance_mb=1e-10, tolerance_cnv=1e-6, linear_solver_reduction=1e-8, linear_solver_maxiter=300)
    gm = GpuBlackoilModel(grid, tab, prm)
    model = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p), tolerance_wells=1e-9, tolerance_well_control=1e-9)
    gm.setState(st)
    names = oracle.PROP_NAMES

    def in_place():
        props = oracle.cell_props(grid, tab, gm.getState())
        return np.array([(props[:, names.index("accum_" + c), 0] * grid.pv).sum() for c in "wog"])

    class Recorder:                      # wraps the solver: records (dt, volumes before/after, well rates) of every converged sub-step
        def __init__(self):
            self.inner, self.steps = NonlinearSolver(), []

        def step(self, m):
            before = in_place()
            out = self.inner.step(m, single_precision=False)
            ws = model.pull_well_state()
            self.steps.append((m.m.dt, before, in_place(), ws.qs.copy()))
            return out

    rec = Recorder()
    ats = ts.AdaptiveTimeStepping(initial_timestep_days=1.0)
    rep = ats.step(0.0, 30 * decks.DAY, rec, model)
    assert rep["converged"] and len(rep["substeps"]) >= 3 and sum(rep["substeps"]) == pytest.approx(30 * decks.DAY)
    inj_rate = 2000.0 / 86400.0
    for dt, before, after, qs in rec.steps[-len(rep["substeps"]):]:
        net = qs.sum(axis=0) * dt                                        # surface volumes added by all wells, per component
        scale = inj_rate * dt
        assert np.all(np.abs((after - before) - net) <= 1e-5 * np.array([scale, scale, 200 * scale])), (dt / decks.DAY, after - before, net)
        assert abs(qs[0, 0] - inj_rate) <= 1e-9 and qs[1, 1] < 0
    gm.close()


@pytest.mark.parametrize("case", ["bhp_limit_midstep", "presolve_switch", "prod_rate_limit", "thp"])
@pytest.mark.parametrize("cpr", [0, 1])
def test_device_well_controls_match_host(gpu_lib, oracle, case, cpr):
    """updateWellControls / solveWellEq / THP on the DEVICE (csrc/wells.hip) against the host well model on the oracle: the same
    control switches at the same Newton iterations, the same pre-solve iteration count, the same well and reservoir state.
      bhp_limit_midstep: a rate-controlled injector runs into its BHP limit after the first Newton update (switch at iteration 1);
      presolve_switch:   the limit is already broken with the reservoir frozen (solveWellEq switches before the first linearisation);
      prod_rate_limit:   a BHP-controlled producer with an oil-rate limit;   thp: a producer on THP control through a VFP table."""
    from test_wells_host import _limits_setup
    kw = {"bhp_limit_midstep": dict(inj_bhp_limit_bar=262.0), "presolve_switch": dict(inj_bhp_limit_bar=255.0),
          "prod_rate_limit": dict(inj_bhp_limit_bar=600.0, prod_rate_limit=150.0), "thp": dict(inj_bhp_limit_bar=600.0, thp=True)}[case]
    grid, tab, st, wl, tables = _limits_setup(**kw)
    prm = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500, cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=cpr)
    prm_o = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500)
    dt = 5 * decks.DAY
    gm = GpuBlackoilModel(grid, tab, prm)
    ob = OracleBackend(oracle, grid, tab, prm_o, wells=wl.arrays())
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p), vfp_tables=tables)
    mo = W.WellCoupledModel(ob, W.StandardWellsHost(wl, grid.z, tab.surface_density[0], vfp_tables=tables), W.WellState(wl, st.p))
    md.prepareStep(dt, st); mo.prepareStep(dt, st)
    history = []
    it = 0
    while True:
        cd, _ = md.nonlinearIteration(it, single_precision=False)
        co, _ = mo.nonlinearIteration(it, single_precision=False)
        ws = md.pull_well_state()
        if it == 0:
            assert md.presolve_converged and md.presolve_iterations == mo.wh.well_iterations, (md.presolve_iterations, mo.wh.well_iterations)
        assert cd == co, it
        assert np.array_equal(ws.current, mo.ws.current), (it, ws.current, mo.ws.current)
        assert np.allclose(md.well_flux_residual, mo.wh.well_flux_residual, rtol=1e-5, atol=1e-12), it
        assert md.well_ctrl_residual == pytest.approx(mo.wh.well_ctrl_residual, rel=1e-5, abs=1e-9), it
        a, b = gm.getState(), ob.getState()
        assert np.array_equal(a.hc, b.hc), it
        assert np.abs(a.p - b.p).max() <= 1e-6 * np.abs(b.p).max() and np.abs(a.sat - b.sat).max() <= 1e-6, it
        assert np.allclose(ws.bhp, mo.ws.bhp, rtol=1e-7), (it, ws.bhp, mo.ws.bhp)
        assert np.allclose(ws.qs, mo.ws.qs, rtol=1e-6, atol=1e-9 * np.abs(mo.ws.qs).max()), it
        assert np.allclose(ws.thp, mo.ws.thp, rtol=1e-6, atol=1.0), (it, ws.thp, mo.ws.thp)
        history.append(ws.current.copy())
        it += 1
        if (cd and it > 1) or it > 12:
            break
    assert cd and it <= 12
    if case == "bhp_limit_midstep":
        assert history[0][0] == 0 and history[1][0] == 1 and ws.bhp[0] == pytest.approx(262 * decks.BAR, rel=1e-12)
    elif case == "presolve_switch":
        assert history[0][0] == 1 and ws.bhp[0] == pytest.approx(255 * decks.BAR, rel=1e-12)
    elif case == "prod_rate_limit":
        assert ws.current[1] == 1 and ws.qs[1, 1] == pytest.approx(-150.0 / 86400.0, rel=1e-9)
    else:
        assert ws.current[1] == 0 and ws.thp[1] == pytest.approx(30 * decks.BAR, rel=1e-5)
    gm.close()


@pytest.mark.parametrize("case", ["presolve_switch", "prod_rate_limit", "thp", "thp5"])
def test_well_presolve_forms_agree(gpu_lib, monkeypatch, case):
    """solveWellEq on the device in its three forms -- one fused launch with a counter barrier per iteration (default), two launches per
    iteration (OPMGPU_WELL_PRESOLVE_FUSED=0) and the single-workgroup fallback that takes over when the fused kernel's barrier gives up
    (forced by OPMGPU_WELL_PRESOLVE_FUSED=2; ADVICE r2: a scheduling condition must not surface as a NumericalIssue) -- must give the same
    pre-solve iteration count, the same control switches and the same well state, bit for bit.
    thp5: the producer on THP control through a 5-axis VFP table, ALQ between nodes (tests/vfp_cases.py, the deck of test_gpu_vfp.py)."""
    from test_wells_host import _limits_setup
    if case == "thp5":
        import vfp_cases
        c = vfp_cases.lockstep_case("prod_thp5")
        grid, tab, st, wl, tables = c["grid"], c["tab"], c["st"], c["wells"], c["tables"]
    else:
        kw = {"presolve_switch": dict(inj_bhp_limit_bar=255.0), "prod_rate_limit": dict(inj_bhp_limit_bar=600.0, prod_rate_limit=150.0),
              "thp": dict(inj_bhp_limit_bar=600.0, thp=True)}[case]
        grid, tab, st, wl, tables = _limits_setup(**kw)
    out = {}
    for mode in ("1", "0", "2"):
        monkeypatch.setenv("OPMGPU_WELL_PRESOLVE_FUSED", mode)
        gm = GpuBlackoilModel(grid, tab, capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500))
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p), vfp_tables=tables)
        md.prepareStep(5 * decks.DAY, st)
        conv, _ = md.nonlinearIteration(0, single_precision=False)
        ws = md.pull_well_state()
        assert md.presolve_converged and md.presolve_iterations >= 1
        out[mode] = (md.presolve_iterations, ws.current.copy(), ws.bhp.copy(), ws.qs.copy(), ws.thp.copy(), gm.getState())
        gm.close()
    for mode in ("0", "2"):
        a, b = out["1"], out[mode]
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), (mode, a[0], b[0])
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), mode
        assert np.array_equal(a[5].p, b[5].p) and np.array_equal(a[5].sat, b[5].sat), mode


# bhp step limit of test_well_presolve_without_convergence
PRESOLVE_DBHP_MAX_REL = 1e-4


@pytest.mark.parametrize("name", ["presolve_switch", "many65"])
def test_well_presolve_without_convergence(gpu_lib, oracle, monkeypatch, name):
    """solveWellEq that does NOT converge, in its three forms: the exit after max_it = 15 steps and "well_state = well_state0"
    (BlackoilModelBase_impl.hpp:1124-1126).  dbhp_max_rel = 1e-4 lets the bottom-hole pressure move by 0.025 bar per step, so the rate
    controlled injectors cannot reach their rates.  The host restatement (solve_well_eq, checked here too) returns (False, 15) with finite
    residuals on both decks: last B_avg * max |flux eq| = 1.6e-2 on presolve_switch, 6.7e-2 on many65 (65 wells: one past the 64-lane stride
    of the maxima loop), against tolerance_wells = 1e-4.  With 1e-3, the first value tried, presolve_switch converges in 10 iterations
    (many65: (False, 15)); 5e-4 and 3e-4 give (False, 15) on both.
    Every form must report not converged after 15 iterations, raise no error bit and leave the well state as it was.  bhp, qs, thp and
    current are compared with the state handed to the device.  perf_rates and perf_press are rewritten by the assembly that follows the
    pre-solve in the same call, from the restored state: they are compared with a run whose pre-solve is switched off
    (solve_welleq_initially = 0), and so are the other four.  After the Newton update the three forms agree bit for bit."""
    from test_wells_host import _limits_setup
    import well_size_decks as D
    if name == "many65":
        deck = D.many_deck(65)
        grid, tab, st, wl, dt = deck.grid, deck.tab, deck.st, deck.wl, deck.dt
    else:
        grid, tab, st, wl, _ = _limits_setup(inj_bhp_limit_bar=255.0)
        dt = 5 * decks.DAY
    rel = PRESOLVE_DBHP_MAX_REL
    fields = ("bhp", "qs", "thp", "perf_rates", "perf_press", "current")

    class Host(W.StandardWellsHost):
        def solve_well_eq(self, *a, **kw):
            self.presolve = super().solve_well_eq(*a, **kw)
            self.presolve_residuals = np.concatenate([self.flux_eq.ravel(), self.ctrl_eq.ravel()])
            return self.presolve

    wh = Host(wl, grid.z, tab.surface_density[0], dbhp_max_rel=rel)
    mo = W.WellCoupledModel(OracleBackend(oracle, grid, tab, capi.default_params(dbhp_max_rel=rel), wells=wl.arrays()), wh, W.WellState(wl, st.p))
    mo.prepareStep(dt, st)
    mo.assemble(True)
    assert wh.presolve == (False, 15) and np.isfinite(wh.presolve_residuals).all(), wh.presolve

    def first_assembly(mode, presolve=1):
        monkeypatch.setenv("OPMGPU_WELL_PRESOLVE_FUSED", mode)
        gm = GpuBlackoilModel(grid, tab, capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=2000, dbhp_max_rel=rel,
                                                            solve_welleq_initially=presolve))
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
        md.prepareStep(dt, st)
        gm.setSolvePrecision(False)
        gm.assemble(True)
        return gm, md, md.pull_well_state().copy()

    gm, md, ref = first_assembly("1", presolve=0)
    gm.close()
    start = W.WellState(wl, st.p)
    out = {}
    for mode in ("1", "0", "2"):
        gm, md, ws = first_assembly(mode)
        assert not md.presolve_converged and md.presolve_iterations == 15, (mode, md.presolve_converged, md.presolve_iterations)
        for f in ("bhp", "qs", "thp", "current"):
            assert np.array_equal(getattr(ws, f), getattr(start, f)), (mode, f)
        for f in fields:
            assert np.array_equal(getattr(ws, f), getattr(ref, f)), (mode, f)
        gm.getConvergence()
        md.wellConvergence()                 # raises on a stray error bit (opmgpu_well_convergence != OPMGPU_OK)
        gm.solveJacobianSystem(single_precision=False)
        gm.updateState()
        ws = md.pull_well_state()
        out[mode] = ([getattr(ws, f).copy() for f in fields], gm.getState())
        gm.close()
    for mode in ("0", "2"):
        a, b = out["1"], out[mode]
        assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])), mode
        assert np.array_equal(a[1].p, b[1].p) and np.array_equal(a[1].sat, b[1].sat), mode


@pytest.mark.parametrize("gmres", [0, 1])
def test_reference_cpr_formulation_with_device_wells(gpu_lib, gmres):
    """cpr_reference_transform on the model path with the device well model: the matrix, the wells' rank-7 rows P_w and the right-hand side are
    transformed by L, the bordered pressure column follows the pressure row's 200-bar scaling -- the Newton path must be the untransformed
    run's (tight linear tolerance), with the same convergence decisions."""
    grid, tab, st, wl = _setup()
    out = {}
    for tr in (0, 1, 2):         # 2: with the reference's own second stage, the point ILU0 of the transformed scalar system
        gm = GpuBlackoilModel(grid, tab, capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, newton_use_gmres=gmres, cpr_reference_transform=tr, linear_solver_reduction=1e-11, linear_solver_maxiter=400))
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
        md.prepareStep(2 * decks.DAY, st)
        hist = []
        for it in range(4):
            conv, lin = md.nonlinearIteration(it, single_precision=False)
            hist.append((conv, lin))
        ws = md.pull_well_state()
        out[tr] = (gm.getState(), ws.bhp.copy(), ws.qs.copy(), hist)
        gm.close()
    a = out[0]
    for tr in (1, 2):
        b = out[tr]
        assert [h[0] for h in a[3]] == [h[0] for h in b[3]], tr
        assert np.array_equal(a[0].hc, b[0].hc), tr
        assert np.abs(a[0].p - b[0].p).max() <= 1e-6 * np.abs(a[0].p).max() and np.abs(a[0].sat - b[0].sat).max() <= 1e-6, tr
        assert np.allclose(a[1], b[1], rtol=1e-7) and np.allclose(a[2], b[2], rtol=1e-6, atol=1e-9 * np.abs(a[2]).max()), tr


CPR_VARIANTS = {
    # the reference CPR plug-in's documented defaults (NewtonIterationBlackoilCPR.hpp:59-63): no AMG -- the elliptic part by an ILU0-preconditioned
    # inner BiCGStab --, relax 1.0
    "reference_defaults": dict(use_cpr=1),
    "ilu0_inner_cg": dict(use_cpr=1, cpr_use_bicgstab=0),
    "amg_inner_bicgstab": dict(use_cpr=1, cpr_use_amg=1),
    "amg_inner_cg": dict(use_cpr=1, cpr_use_amg=1, cpr_use_bicgstab=0),
    "amg_vcycle_relax_0.9": dict(use_cpr=1, cpr_use_amg=1, cpr_max_ell_iter=0, cpr_relax=0.9),
    "reference_defaults_relax_0.9_tight_inner": dict(use_cpr=1, cpr_relax=0.9, cpr_solver_tol=1e-4, cpr_max_ell_iter=60),
    # cpr_ilu_n: block ILU(n) with level-of-fill as the second stage (csrc/fillilu.inl)
    "reference_defaults_ilu1": dict(use_cpr=1, cpr_ilu_n=1),
    "amg_vcycle_ilu2": dict(use_cpr=1, cpr_use_amg=1, cpr_max_ell_iter=0, cpr_ilu_n=2),
}


@pytest.mark.parametrize("gmres", [0, 1])
def test_cpr_parameters_of_the_reference_give_the_same_newton_path(gpu_lib, gmres):
    """cpr_relax / cpr_ilu_n / cpr_use_amg / cpr_use_bicgstab of NewtonIterationBlackoilCPR.hpp:59-63 (+ the inner solve's
    cpr_solver_tol / cpr_max_ell_iter).  Every pressure stage is a PRECONDITIONER: with a tight outer tolerance the Newton path with device
    wells (bordered pressure system) must be the one of the AMG V-cycle stage, whatever solves the elliptic part."""
    import ctypes as C
    grid, tab, st, wl = _setup()
    out = {}
    for name, kw in dict(base=dict(capi.CPR_AMG_VCYCLE), **CPR_VARIANTS).items():
        # (an inner Krylov method makes the preconditioner a DIFFERENT operator in every application.  BiCGStab's recurrences hold for that --
        # x and r are updated with the same vectors --, left-preconditioned GMRES's do not: its Arnoldi relation assumes one fixed M, and the
        # residual it tracks then drifts from the real one (measured here: it reports 1e-11 with 6e-4 left in the pressures).  The
        # reference's CPR + newton_use_gmres has that property by construction; here the true-residual check restarts the cycle from the
        # real defect until it is met.)
        gm = GpuBlackoilModel(grid, tab, capi.default_params(newton_use_gmres=gmres, gmres_verify_residual=gmres, linear_solver_reduction=1e-11, linear_solver_maxiter=400, **kw))
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
        md.prepareStep(2 * decks.DAY, st)
        hist = []
        for it in range(3):
            conv, lin = md.nonlinearIteration(it, single_precision=False)
            hist.append((conv, lin))
        ws = md.pull_well_state()
        solves, its = C.c_int64(0), C.c_int64(0)
        gm._chk(gm.lib.opmgpu_cpr_elliptic_stats(gm.ctx, C.byref(solves), C.byref(its)))
        out[name] = (gm.getState(), ws.bhp.copy(), ws.qs.copy(), hist, solves.value, its.value)
        gm.close()
    a = out["base"]
    assert a[4] == 0 and a[5] == 0                                   # one V-cycle per application: no inner method
    for name in CPR_VARIANTS:
        b = out[name]
        assert [h[0] for h in a[3]] == [h[0] for h in b[3]], name
        assert np.array_equal(a[0].hc, b[0].hc), name
        assert np.abs(a[0].p - b[0].p).max() <= 1e-6 * np.abs(a[0].p).max() and np.abs(a[0].sat - b[0].sat).max() <= 1e-6, name
        assert np.allclose(a[1], b[1], rtol=1e-7) and np.allclose(a[2], b[2], rtol=1e-6, atol=1e-9 * np.abs(a[2]).max()), name
        if "vcycle" in name:
            assert b[4] == 0
        else:
            # one inner solve per preconditioner application, each within its iteration limit
            limit = CPR_VARIANTS[name].get("cpr_max_ell_iter", 25)
            assert b[4] >= sum(h[1] for h in b[3]) and 1 <= b[5] <= limit * b[4], (name, b[4], b[5])
    # a better elliptic solve makes the outer method need fewer iterations: the inner-Krylov stages never need more than the single cycle
    # plus a small margin, and the reference-default stage (ILU0) needs more inner iterations than the AMG one
    lin = {k: sum(h[1] for h in v[3]) for k, v in out.items()}
    if not gmres:          # (under GMRES the restarts of the true-residual check add outer iterations: see the note at the top of the loop)
        assert lin["amg_inner_bicgstab"] <= lin["base"] + 2, lin
    assert out["reference_defaults"][5] / out["reference_defaults"][4] > out["amg_inner_bicgstab"][5] / out["amg_inner_bicgstab"][4], (out["reference_defaults"][4:], out["amg_inner_bicgstab"][4:])


@pytest.mark.parametrize("gmres", [0, 1])
def test_float_preconditioner_walks_the_double_newton_path_with_device_wells(gpu_lib, gmres):
    """opmgpu_params.preconditioner_single on the model path with device wells: the float copy of the Jacobian is written by the assembly, the
    wells' diagonal contributions follow it, ILU0 / pressure stage / stage-2 residual run in float inside the double Krylov method.  At the
    tightest reductions the option is documented for (1e-8 under BiCGStab, 1e-6 under GMRES) the Newton path is the pure double solve's to
    the linear tolerance, with the same convergence decisions; also with the damped second stage and without CPR."""
    grid, tab, st, wl = _setup()
    red = 1e-6 if gmres else 1e-8
    for kw in (dict(capi.CPR_AMG_VCYCLE), dict(capi.CPR_AMG_VCYCLE, cpr_stage2_relax=0.9), dict(use_cpr=0)):
        out = {}
        for mixed in (0, 1):
            gm = GpuBlackoilModel(grid, tab, capi.default_params(newton_use_gmres=gmres, preconditioner_single=mixed, linear_solver_reduction=red, linear_solver_maxiter=400, **kw))
            md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
            md.prepareStep(2 * decks.DAY, st)
            hist = [md.nonlinearIteration(it, single_precision=False) for it in range(3)]
            ws = md.pull_well_state()
            out[mixed] = (gm.getState(), ws.bhp.copy(), ws.qs.copy(), hist)
            gm.close()
        a, b = out[0], out[1]
        tol = 300 * red             # (cond(A) acts on the linear tolerance: measured ~30 x on this deck)
        assert [h[0] for h in a[3]] == [h[0] for h in b[3]], kw
        assert np.array_equal(a[0].hc, b[0].hc), kw
        assert np.abs(a[0].p - b[0].p).max() <= tol * np.abs(a[0].p).max() and np.abs(a[0].sat - b[0].sat).max() <= tol, (kw, gmres)
        assert np.allclose(a[1], b[1], rtol=tol) and np.allclose(a[2], b[2], rtol=10 * tol, atol=tol * np.abs(a[2]).max()), (kw, gmres)
        assert sum(h[1] for h in b[3]) <= sum(h[1] for h in a[3]) + 6, (kw, [h[1] for h in a[3]], [h[1] for h in b[3]])


def test_cpr_parameter_combinations_that_are_not_built_are_refused(gpu_lib):
    """cpr_ilu_n outside 0..8 (or with the point-ILU0 comparison mode) and the one-application stage without the AMG are errors at the first solve,
    not silent fallbacks"""
    from opmgpu.model import LinearSolverProblem  # noqa: F401
    grid, tab, st, _ = _setup()
    for kw, text in ((dict(use_cpr=1, cpr_ilu_n=9), "cpr_ilu_n"), (dict(use_cpr=1, cpr_ilu_n=1, cpr_reference_transform=2, cpr_use_amg=1, cpr_max_ell_iter=0), "cpr_ilu_n"), (dict(use_cpr=1, cpr_use_amg=0, cpr_max_ell_iter=0), "cpr_max_ell_iter"), (dict(use_cpr=1, cpr_relax=0.0), "cpr_relax")):
        gm = GpuBlackoilModel(grid, tab, capi.default_params(**kw))
        gm.prepareStep(2 * decks.DAY, st)
        gm.assemble(True); gm.getConvergence()
        with pytest.raises(Exception) as e:
            gm.solveJacobianSystem(single_precision=False)
        assert text in str(e.value), (kw, str(e.value))
        gm.close()


def test_stabilized_update_relaxes_the_well_increment_too(gpu_lib, oracle):
    """NonlinearSolver::stabilizeNonlinearUpdate acts on the WHOLE increment (NonlinearSolver_impl.hpp:260-301): with device wells the
    recovered (q_s, bhp) increment is relaxed with the reservoir part -- device vs host well model with a forced relaxation of 0.6."""
    from opmgpu.model import NonlinearSolver
    grid, tab, st, wl = _setup()
    # Newton tolerances that are never met: every iteration solves and relaxes
    prm = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500, tolerance_mb=1e-30, tolerance_cnv=1e-30)
    gm = GpuBlackoilModel(grid, tab, prm)
    ob = OracleBackend(oracle, grid, tab, prm, wells=wl.arrays())
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    mo = W.WellCoupledModel(ob, W.StandardWellsHost(wl, grid.z, tab.surface_density[0]), W.WellState(wl, st.p))

    class Forced(NonlinearSolver):          # oscillation "detected" at every iteration >= 1: relaxation 0.9, 0.8, ...
        def detectOscillations(self, hist, it):
            return it >= 1, False

    for relax_type in (capi.RELAX_DAMPEN, capi.RELAX_SOR):
        ns = Forced(relax_type=relax_type)
        md.prepareStep(2 * decks.DAY, st); mo.prepareStep(2 * decks.DAY, st)
        md.ws = W.WellState(wl, st.p); md.push_well_state(); mo.ws.assign(W.WellState(wl, st.p))
        for it in range(4):
            md.nonlinearIteration(it, single_precision=False, nonlinear_solver=ns)
            mo.nonlinearIteration(it, single_precision=False, nonlinear_solver=ns)
            ws = md.pull_well_state()
            a, b = gm.getState(), ob.getState()
            assert np.abs(a.p - b.p).max() <= 1e-6 * np.abs(b.p).max() and np.abs(a.sat - b.sat).max() <= 1e-6, (relax_type, it)
            assert np.allclose(ws.bhp, mo.ws.bhp, rtol=1e-7) and np.allclose(ws.qs, mo.ws.qs, rtol=1e-6, atol=1e-9 * np.abs(mo.ws.qs).max()), (relax_type, it)
        assert md.current_relaxation == pytest.approx(0.7) and mo.current_relaxation == pytest.approx(0.7)
    gm.close()


@pytest.mark.parametrize("with_wells", [True, False])
def test_one_call_newton_iteration_equals_the_call_by_call_sequence(gpu_lib, with_wells):
    """opmgpu_nonlinear_iteration (the whole of BlackoilModelBase::nonlinearIteration + the NonlinearSolver's update stabilisation in one
    library call) against the seven single calls the host mirrors issue: same convergence flags, iteration counts, relaxation, and
    bit-identical reservoir and well states over a time step that needs relaxing."""
    from opmgpu.model import NonlinearSolver
    grid, tab, st, wl = _setup()
    prm = capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1)
    out = []
    for fused in (False, True):
        gm = GpuBlackoilModel(grid, tab, prm)
        gm.fused_iteration = fused
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p)) if with_wells else gm
        ns = NonlinearSolver(relax_rel_tol=1e9)        # "oscillation" from the third iteration on whenever two norms moved: the relaxation path runs
        md.prepareStep(20 * decks.DAY, st)
        hist = []
        for it in range(7):
            conv, lin = md.nonlinearIteration(it, single_precision=True, nonlinear_solver=ns)
            hist.append((bool(conv), int(lin), float(md.current_relaxation)))
            if conv and it >= ns.min_iter:
                break
        s = gm.getState()
        ws = md.pull_well_state() if with_wells else None
        out.append((hist, s, ws))
        gm.close()
    (h0, s0, w0), (h1, s1, w1) = out
    assert h0 == h1, (h0, h1)
    assert np.array_equal(s0.p, s1.p) and np.array_equal(s0.sat, s1.sat) and np.array_equal(s0.hc, s1.hc)
    if with_wells:
        assert np.array_equal(w0.bhp, w1.bhp) and np.array_equal(w0.qs, w1.qs)
    lib = capi.load()
    ctl = capi.NewtonCtl(1, 1, capi.RELAX_DAMPEN, 0.5, 0.1, 0.2)
    gm = GpuBlackoilModel(grid, tab, prm)
    gm.prepareStep(5 * decks.DAY, st)
    import ctypes as C
    conv, lin = C.c_int(0), C.c_int(0)
    # iterations of a step must be consecutive from 0
    assert lib.opmgpu_nonlinear_iteration(gm.ctx, gm.dt, 1, 1, C.byref(ctl), C.byref(conv), C.byref(lin), None, None) == capi.EINVAL
    gm.close()


@pytest.mark.parametrize("single", [False, True])
def test_cpr_weights_with_device_wells_follow_the_final_matrix(gpu_lib, single):
    """With device wells the assembly kernel writes the CPR weights of every row from the reservoir equations and the well model redoes the
    rows of its perforated cells after adding its diagonal terms (k_cpr_weights_rows).  What the solver then uses must be
    formEllipticSystem's rule (NewtonIterationUtilities.cpp:212-252, as in test_cpr_pressure_equation_weights) applied to the FINAL matrix."""
    grid, tab, st, wl = _setup()
    gm = GpuBlackoilModel(grid, tab, capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1))
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    md.prepareStep(150 * decks.DAY, st)          # long enough to need several Newton iterations
    checked = 0
    for it in range(4):                     # from the second iteration on the well prologue runs on its side stream
        conv, _ = md.nonlinearIteration(it, single_precision=single)
        if conv and it >= 1:
            break                           # converged: no solve, nothing to check
        checked += 1
        # after the iteration: the matrix of THIS iteration is still resident, so are the weights of its solve
        rowptr, col, val = gm.jacobian()
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
        w = np.zeros(3 * nb)
        assert gm.lib.opmgpu_get_cpr_weights(gm.ctx, capi.dptr(w)) == capi.OK
        bad = np.flatnonzero((w.reshape(3, nb) != expect).any(0))
        assert bad.size == 0, (it, bad[:10], w.reshape(3, nb)[:, bad[:4]], expect[:, bad[:4]], sorted(set(wl.arrays()[1].tolist()) & set(bad.tolist())))
    assert checked >= 2
    gm.close()


def test_update_equations_scaling_with_device_wells_and_cpr(gpu_lib):
    """updateEquationsScaling (default off) with the device well model under CPR: the wells' bordered pressure column, the CPR
    weights and the matrix must all carry the factors of THIS assembly -- the run with the option walks the Newton path of the run without it
    (a row scaling changes no solution; tight linear tolerance), and its factors are the means of 1 / b of the assembled state."""
    grid, tab, st, wl = _setup()
    out = {}
    for ues in (0, 1):
        gm = GpuBlackoilModel(grid, tab, capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, update_equations_scaling=ues, linear_solver_reduction=1e-11, linear_solver_maxiter=400))
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
        md.prepareStep(2 * decks.DAY, st)
        hist, scales = [], []
        for it in range(4):
            conv, lin = md.nonlinearIteration(it, single_precision=False)
            got = np.zeros(3)
            gm._chk(gm.lib.opmgpu_get_matbalscale(gm.ctx, capi.dptr(got)))
            hist.append((conv, lin)); scales.append(got.copy())
        ws = md.pull_well_state()
        out[ues] = (gm.getState(), ws.bhp.copy(), ws.qs.copy(), hist, scales)
        gm.close()
    a, b = out[0], out[1]
    assert all(np.array_equal(s, [1.1169, 1.0031, 0.0031]) for s in a[4])
    assert all(0.5 < s[0] < 1.5 and 0.5 < s[1] < 2.0 and 0.0 < s[2] < 0.1 for s in b[4]) and not np.array_equal(b[4][0], b[4][-1])     # mean 1 / b, moving with the state
    assert [h[0] for h in a[3]] == [h[0] for h in b[3]]
    assert max(h[1] for h in b[3]) <= 2 * max(h[1] for h in a[3]) + 2          # the preconditioner stays consistent: no blow-up of the iteration counts
    assert np.array_equal(a[0].hc, b[0].hc)
    assert np.abs(a[0].p - b[0].p).max() <= 1e-6 * np.abs(a[0].p).max() and np.abs(a[0].sat - b[0].sat).max() <= 1e-6
    assert np.allclose(a[1], b[1], rtol=1e-7) and np.allclose(a[2], b[2], rtol=1e-6, atol=1e-9 * np.abs(a[2]).max())
