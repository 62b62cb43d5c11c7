"""The passes and launches a CPR + GMRES solve does without (LinSolver::lean_solve, LinSolver::cpr_cancel_p).  Every case
builds two contexts, one with the switch at 0 (the plain launches) and one at 1 (the default); the switches are read when the context is created.

OPMGPU_LEAN_SOLVE (no clear of x, the solution stored where the model reads it, gmbuf cleared by k_ctl_init, no k_gm_reset_s behind that
clear, the V-cycle's restriction with eight lanes per aggregate) keeps every bit: the check is np.array_equal.
OPMGPU_CPR_CANCEL_P (the pressure correction added inside the ILU0 sweeps) rounds differently: the three statements of
test_gpu_gmres_closed_form._same_solve, and equality wherever its conditions do not hold."""
import numpy as np
import pytest

import test_gpu_cpr_stages as stages
import test_gpu_gmres_closed_form as closed_form
from opmgpu import capi, decks
from opmgpu import wells as W
from opmgpu.model import GpuBlackoilModel, GpuNewtonIteration, NonlinearSolver

pytestmark = pytest.mark.gpu

LEAN, CANCEL = "OPMGPU_LEAN_SOLVE", "OPMGPU_CPR_CANCEL_P"


def _solve(monkeypatch, key, on, system, single=False, gmres=1, **kw):
    monkeypatch.setenv(key, "1" if on else "0")
    rowptr, col, val, b, A = system
    s = GpuNewtonIteration(capi.default_params(newton_use_gmres=gmres, ilu_ordering=capi.ORDER_MULTICOLOR, linear_solver_maxiter=400, **kw))
    x = s.computeNewtonIncrement(rowptr, col, val, b, single)
    out = dict(x=x, iterations=s.iterations(), reduction=s.reduction, nlevels=s.ordering()[2], true=np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    s.close()
    return out


def _identical(monkeypatch, key, system, **kw):
    off = _solve(monkeypatch, key, False, system, **kw)
    on = _solve(monkeypatch, key, True, system, **kw)
    print("%s: iterations off %d on %d; reduction off %.3e on %.3e; levels %d" % (key, off["iterations"], on["iterations"], off["reduction"], on["reduction"], off["nlevels"]))
    assert on["iterations"] == off["iterations"]
    assert np.array_equal(off["x"], on["x"])
    return off, on


# ---------------------------------------------------------------- OPMGPU_LEAN_SOLVE: bit for bit
@pytest.mark.parametrize("single,red,kw", [(False, 1e-10, {}), (True, 1e-5, {}), (True, 1e-10, dict(ignore_convergence_failure=1))],
                         ids=["double", "float_1e-5", "float_1e-10"])
def test_lean_cpr_gmres(gpu_lib, oracle, monkeypatch, single, red, kw):
    """CPR + GMRES(40) on the 12 x 10 x 8 system; float vectors to 1e-5 and to 1e-10 (two cycles: the second accumulates on x).
    Measured: 20 columns in double, 11 (1e-5) and 52 (1e-10, reduction 9.3e-11) in float, in both runs; x identical."""
    off, _ = _identical(monkeypatch, LEAN, closed_form._system(oracle, "b1"), single=single, linear_solver_reduction=red, **dict(capi.CPR_AMG_VCYCLE, **kw))
    assert off["iterations"] > 0 and np.abs(off["x"]).max() > 0


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
def test_lean_restart(gpu_lib, oracle, monkeypatch, single):
    """linear_solver_restart = 3: the first cycle writes x, every later one accumulates on it.  Measured: 36 columns (double, 1e-10) and
    17 (float, 1e-5) in both runs."""
    off, _ = _identical(monkeypatch, LEAN, closed_form._system(oracle, "b1"), single=single, linear_solver_reduction=1e-5 if single else 1e-10,
                        linear_solver_restart=3, **capi.CPR_AMG_VCYCLE)
    assert off["iterations"] > 3


def test_lean_ilu0_gmres(gpu_lib, oracle, monkeypatch):
    """ILU0 + GMRES (use_cpr = 0) to 1e-6: 56 columns in both runs"""
    off, _ = _identical(monkeypatch, LEAN, closed_form._system(oracle, "b1"), linear_solver_reduction=1e-6, use_cpr=0, ilu_relaxation=1.0)
    assert off["iterations"] > 0


@pytest.mark.parametrize("on", [False, True], ids=["plain", "lean"])
def test_lean_zero_rhs(gpu_lib, oracle, monkeypatch, on):
    """a zero right-hand side behind a solve that left a solution in x: 0 iterations, and x is all zeros (nothing combines into it, so the
    lean path has to clear it at that exit)"""
    monkeypatch.setenv(LEAN, "1" if on else "0")
    rowptr, col, val, b, _ = closed_form._system(oracle, "b1")
    s = GpuNewtonIteration(capi.default_params(newton_use_gmres=1, ilu_ordering=capi.ORDER_MULTICOLOR, linear_solver_maxiter=400, linear_solver_reduction=1e-10,
                                               **capi.CPR_AMG_VCYCLE))
    x = s.computeNewtonIncrement(rowptr, col, val, b, False)
    assert s.iterations() > 0 and np.abs(x).max() > 0
    x = s.computeNewtonIncrement(rowptr, col, val, np.zeros_like(b), False)
    assert s.iterations() == 0
    assert np.array_equal(x, np.zeros_like(b))
    s.close()


def test_lean_irregular_deck(gpu_lib, oracle, monkeypatch):
    """baseline_decks.random_irregular(3): 4 ILU levels, irregular aggregates.  Measured: 54 columns in both runs."""
    off, _ = _identical(monkeypatch, LEAN, closed_form._system(oracle, "irregular"), linear_solver_reduction=1e-10, **capi.CPR_AMG_VCYCLE)
    assert off["nlevels"] > 2


def test_lean_bicgstab(gpu_lib, oracle, monkeypatch):
    """CPR + BiCGStab: it shares the restriction, nothing else of the switch reaches it.  Measured: 12 iterations in both runs."""
    off, _ = _identical(monkeypatch, LEAN, closed_form._system(oracle, "b1"), gmres=0, linear_solver_reduction=1e-10, **capi.CPR_AMG_VCYCLE)
    assert off["iterations"] > 0


def _newton_run(monkeypatch, key, on):
    """three Newton iterations of test_gpu_gmres_closed_form._newton_run (10 x 10 x 4, device 5-spot), then a fourth taken apart: the increment
    the model holds after the solve (what updateState applies: the solver's mirror, or the copy of x), and the state behind it"""
    monkeypatch.setenv(key, "1" if on else "0")
    grid = decks.cartesian_grid(10, 10, 4, lognormal_sigma=0.5)
    tab = decks.satfunc_standard_tables()
    st = decks.initial_state(grid, tab, perturb=0.01)
    wl = W.five_spot(grid, rate_m3_per_day=20.0, bhp_prod_bar=150.0)
    gm = GpuBlackoilModel(grid, tab, capi.default_params(newton_use_gmres=1, **capi.CPR_AMG_VCYCLE))
    m = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    m.prepareStep(decks.DAY, st)
    ns = NonlinearSolver()
    lin = [m.nonlinearIteration(it, single_precision=False, nonlinear_solver=ns)[1] for it in range(3)]
    s3 = gm.getState()
    gm.setSolvePrecision(False)
    gm.assemble(False)
    gm.getConvergence()
    dx = gm.solveJacobianSystem(want_dx=True, single_precision=False)
    lin.append(gm.linear_iterations)
    gm.updateState()
    s4 = gm.getState()
    n, _, nw = gm.cpr_levels()
    gm.close()
    return lin, s3, dx, s4, nw


def _state_equal(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("p", "sat", "rs", "rv", "hc"))


def test_lean_newton_with_wells(gpu_lib, monkeypatch):
    """the model path: a bordered level 0 with singleton well aggregates, and the solver's mirror feeding k_update_state.  The plain run
    copies x into the model's increment, the lean run has the combination store it there: the same increment, the same state.
    Measured: linear iterations [3, 6, 5, 4] in both runs, 5 border wells."""
    lin0, a3, dx0, a4, nw = _newton_run(monkeypatch, LEAN, False)
    lin1, b3, dx1, b4, _ = _newton_run(monkeypatch, LEAN, True)
    print("linear iterations plain %s lean %s; border wells %d; |dx| %.3e" % (lin0, lin1, nw, np.abs(dx0).max()))
    assert nw == 5 and lin0[0] > 0 and lin0[3] > 0 and lin1 == lin0
    assert _state_equal(a3, b3)
    assert np.abs(dx0).max() > 0 and np.array_equal(dx0, dx1)
    assert _state_equal(a4, b4) and not np.array_equal(a4.p, a3.p)


def _aggregate_sizes(obj):
    n, _, _ = obj.cpr_levels()
    return [np.bincount(obj.cpr_level(l)[3], minlength=n[l + 1]) for l in range(len(n) - 1)]


def test_lean_restriction_alone(gpu_lib, oracle, monkeypatch):
    """one V-cycle (opmgpu_cpr_vcycle_apply) on a seeded random right-hand side, on the hierarchies of the 972-cell model deck with wells and of
    the 5 760-row B1 deck, with the restriction of one thread and of eight lanes per aggregate: the same bits.  The level data show that every
    branch of the lanes' loop ran: a singleton, a last batch that is not full, more than one batch.  Measured: 986 aggregates of 1 .. 26
    rows, 10 singletons, 849 no multiple of 8, 364 above 8."""
    b1 = stages._b1_system(oracle, 20, 18, 16)
    out = {}
    sizes = []
    for on in (False, True):
        monkeypatch.setenv(LEAN, "1" if on else "0")
        gm = stages._model((9, 9, 12), False)
        s = GpuNewtonIteration(capi.default_params(**capi.CPR_AMG_VCYCLE, linear_solver_reduction=1e-6, linear_solver_maxiter=200))
        s.computeNewtonIncrement(*b1, False)
        for name, obj in (("model", gm), ("b1", s)):
            n, _, nw = obj.cpr_levels()
            assert len(n) >= 2 and n[0] == {"model": 972 + 5, "b1": 5760}[name]
            rhs = np.random.default_rng(7).standard_normal(n[0])
            out[name, on] = obj.cpr_vcycle_apply(rhs)
            if on:
                sizes += _aggregate_sizes(obj)
                if name == "model":
                    assert nw == 5 and (sizes[-len(n) + 1][-nw:] == 1).all()          # the wells' singleton aggregates
        gm.close()
        s.close()
    allsz = np.concatenate(sizes)
    print("aggregate sizes: min %d max %d, singletons %d, not a multiple of 8: %d, above 8: %d of %d" % (allsz.min(), allsz.max(), (allsz == 1).sum(), (allsz % 8 != 0).sum(),
                                                                                                     (allsz > 8).sum(), allsz.size))
    assert (allsz == 1).any() and (allsz % 8 != 0).any() and (allsz > 8).any()
    for name in ("model", "b1"):
        assert np.abs(out[name, False]).max() > 0
        assert np.array_equal(out[name, False], out[name, True]), name


# ---------------------------------------------------------------- OPMGPU_CPR_CANCEL_P: the statements of the closed form's check
def _same_solve(monkeypatch, system, red, **kw):
    """test_gpu_gmres_closed_form._same_solve for this switch: same iteration count, both below the reduction, the new path's true residual
    within 5 %"""
    plain = _solve(monkeypatch, CANCEL, False, system, linear_solver_reduction=red, **kw)
    new = _solve(monkeypatch, CANCEL, True, system, linear_solver_reduction=red, **kw)
    print("iterations plain %d cancel %d; reduction plain %.3e cancel %.3e; true residual plain %.6e cancel %.6e (ratio %.6f); levels %d"
          % (plain["iterations"], new["iterations"], plain["reduction"], new["reduction"], plain["true"], new["true"], new["true"] / plain["true"], plain["nlevels"]))
    assert new["iterations"] == plain["iterations"]
    assert plain["reduction"] < red and new["reduction"] < red
    assert new["true"] <= 1.05 * plain["true"]
    return plain, new


@pytest.mark.parametrize("kw", [{}, dict(linear_solver_restart=3)], ids=["gmres40", "restart3"])
def test_cancel_p(gpu_lib, oracle, monkeypatch, kw):
    """CPR + GMRES in double to 1e-10 on the 12 x 10 x 8 system (a two-level plan).  Measured: 20 columns in both runs, true residual
    1.760002e-11 (plain) / 1.761569e-11 (cancel): ratio 1.000891; restart 3: 36 columns, 4.426347e-12 / 4.570775e-12: ratio 1.032629."""
    plain, new = _same_solve(monkeypatch, closed_form._system(oracle, "b1"), 1e-10, **dict(capi.CPR_AMG_VCYCLE, **kw))
    assert plain["nlevels"] == 2
    assert not np.array_equal(plain["x"], new["x"])          # (the path ran: it rounds differently)


@pytest.mark.parametrize("name,gmres,single,kw", [("b1", 1, False, dict(cpr_stage2_relax=0.9)), ("b1", 1, False, dict(cpr_relax=0.9)), ("irregular", 1, False, {}),
                                                  ("b1", 0, False, {}), ("b1", 1, True, {})],
                         ids=["stage2_relax_0.9", "cpr_relax_0.9", "four_levels", "bicgstab", "float"])
def test_cancel_p_conditions(gpu_lib, oracle, monkeypatch, name, gmres, single, kw):
    """a relaxation factor other than 1, more than two levels, BiCGStab, a float solve: the plain sequence, bit for bit"""
    off, _ = _identical(monkeypatch, CANCEL, closed_form._system(oracle, name), gmres=gmres, single=single, linear_solver_reduction=1e-5 if single else 1e-10,
                        **dict(capi.CPR_AMG_VCYCLE, **kw))
    assert off["iterations"] > 0


def test_cancel_p_newton_with_wells(gpu_lib, monkeypatch):
    """three (and a fourth) Newton iterations with device wells: the same linear iterations, pressures equal to 1e-12 relative.
    Measured: [3, 6, 5, 4] in both runs, largest relative pressure difference 4.2e-16, saturation difference 5.9e-15."""
    lin0, _, _, a4, _ = _newton_run(monkeypatch, CANCEL, False)
    lin1, _, _, b4, _ = _newton_run(monkeypatch, CANCEL, True)
    dp = np.abs(b4.p - a4.p).max() / np.abs(a4.p).max()
    print("linear iterations plain %s cancel %s; max relative pressure difference %.3e, saturation difference %.3e" % (lin0, lin1, dp, np.abs(b4.sat - a4.sat).max()))
    assert lin0[0] > 0 and lin1 == lin0
    assert dp <= 1e-12
