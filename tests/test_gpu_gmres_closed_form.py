"""Closed form of the GMRES product on the level-0 rows (k_spmv GM mode, LinSolver::gmres): every case runs the same solve with the explicit
product on all rows (OPMGPU_CLOSED=0) and with the closed form (OPMGPU_CLOSED=1, the default); the switch is read when the context is created."""
import numpy as np
import pytest

from opmgpu import baseline_decks, capi, decks
from opmgpu import wells as W
from opmgpu.model import GpuBlackoilModel, GpuNewtonIteration, NonlinearSolver
from util import bsr_to_scipy

pytestmark = pytest.mark.gpu

_systems = {}


def _system(oracle, name):
    """(rowptr, col, val, b, A) of a deck, assembled once by the oracle: 'b1' = the 12 x 10 x 8 deck of test_gmres_option, 'irregular' =
    baseline_decks.random_irregular(3): 44 x 22 x 7 with 48 % of the cells inactive at random and NNCs (3.5 k cells: no need to reduce it)"""
    if name not in _systems:
        if name == "b1":
            grid = decks.cartesian_grid(12, 10, 8, lognormal_sigma=0.8)
            tab = decks.satfunc_standard_tables()
            st = decks.initial_state(grid, tab, perturb=0.01)
        else:
            grid, tab, st, _, _ = baseline_decks.random_irregular(3)
        scale = np.asarray(capi.default_params().matbalscale[:])
        rowptr, col = oracle.pattern(grid)
        nc = grid.nc
        r, val, _, _ = oracle.assemble(grid, tab, 5 * decks.DAY, st, rowptr, col, scale=tuple(scale))
        b = np.ascontiguousarray((r * np.repeat(scale, nc)).reshape(3, nc).T).ravel()
        _systems[name] = (rowptr, col, val, b, bsr_to_scipy(rowptr, col, val))
    return _systems[name]


def _solve(monkeypatch, closed, system, single=False, **kw):
    monkeypatch.setenv("OPMGPU_CLOSED", "1" if closed else "0")
    rowptr, col, val, b, A = system
    s = GpuNewtonIteration(capi.default_params(newton_use_gmres=1, ilu_ordering=capi.ORDER_MULTICOLOR, linear_solver_maxiter=400, **kw))
    x = s.computeNewtonIncrement(rowptr, col, val, b, single)
    out = dict(x=x, iterations=s.iterations(), reduction=s.reduction, nlevels=s.ordering()[2], true=np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    s.close()
    return out


def _same_solve(monkeypatch, system, red, **kw):
    """the three statements of every case: same iteration count, both below the reduction, the closed run's true residual within 5 %"""
    full = _solve(monkeypatch, False, system, linear_solver_reduction=red, **kw)
    closed = _solve(monkeypatch, True, system, linear_solver_reduction=red, **kw)
    print("iterations full %d closed %d; reduction full %.3e closed %.3e; true residual full %.6e closed %.6e (ratio %.6f); levels %d"
          % (full["iterations"], closed["iterations"], full["reduction"], closed["reduction"], full["true"], closed["true"], closed["true"] / full["true"],
             full["nlevels"]))
    assert closed["iterations"] == full["iterations"]
    assert full["reduction"] < red and closed["reduction"] < red
    assert closed["true"] <= 1.05 * full["true"]
    return full, closed


def test_b1_matrix(gpu_lib, oracle, monkeypatch):
    """CPR (one V-cycle + block ILU0) + GMRES(40) in double to 1e-10 on the 12 x 10 x 8 deck, 2-colour order: half of the rows are level-0 rows.
    Measured: 20 columns in both runs, true residual 1.760968e-11 (full) / 1.760002e-11 (closed): ratio 0.99945."""
    full, closed = _same_solve(monkeypatch, _system(oracle, "b1"), 1e-10, **capi.CPR_AMG_VCYCLE)
    assert full["nlevels"] == 2
    assert not np.array_equal(full["x"], closed["x"])        # (the closed form ran: the two paths round differently)


def test_restart(gpu_lib, oracle, monkeypatch):
    """linear_solver_restart = 3: every cycle after the first starts from the true defect r = b - A x, which then is the base vector.
    Measured: 36 columns in both runs, true residual 4.352e-12 / 4.426e-12: ratio 1.0171."""
    full, _ = _same_solve(monkeypatch, _system(oracle, "b1"), 1e-10, linear_solver_restart=3, **capi.CPR_AMG_VCYCLE)
    assert full["iterations"] > 3


@pytest.mark.parametrize("relax", [1.0, 0.9])
def test_ilu0_gmres(gpu_lib, oracle, monkeypatch, relax):
    """ILU0 + GMRES (use_cpr = 0) to 1e-6: the closed form with c = 0.  It needs relaxation 1; at the default 0.9 the launch is the explicit one
    and the two runs are identical.  Measured: 56 columns in both runs, true residual 5.250877e-07 in both: ratio 1.000000."""
    full, closed = _same_solve(monkeypatch, _system(oracle, "b1"), 1e-6, use_cpr=0, ilu_relaxation=relax)
    if relax != 1.0:
        assert np.array_equal(full["x"], closed["x"])


def _newton_run(monkeypatch, closed):
    monkeypatch.setenv("OPMGPU_CLOSED", "1" if closed else "0")
    grid = decks.cartesian_grid(10, 10, 4, lognormal_sigma=0.5)
    tab = decks.satfunc_standard_tables()
    st = decks.initial_state(grid, tab, perturb=0.01)
    wl = W.five_spot(grid, rate_m3_per_day=20.0, bhp_prod_bar=150.0)
    gm = GpuBlackoilModel(grid, tab, capi.default_params(newton_use_gmres=1, **capi.CPR_AMG_VCYCLE))
    m = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    m.prepareStep(decks.DAY, st)
    ns = NonlinearSolver()
    lin = [m.nonlinearIteration(it, single_precision=False, nonlinear_solver=ns)[1] for it in range(3)]
    lev = gm.ordering()[1]
    out = gm.getState()
    gm.close()
    return lin, out, lev[np.asarray(wl.cells)]


def test_wells_on_level0_rows(gpu_lib, monkeypatch):
    """The model path with device wells (5-spot of full columns on 10 x 10 x 4): a perforated level-0 row is no multiple of the base vector
    (the well operator adds P t_w) and takes the full row product (the mask branch).  Three Newton iterations of a 1-day step, linear
    reduction 1e-2: the same linear iteration counts, pressures equal to 1e-9 relative.  Measured: linear iterations [3, 6, 5] in both runs, 10 of the 20 perforated rows on level 0,
    largest relative pressure difference 4.3e-16, saturation difference 6.0e-15."""
    lin0, s0, lev0 = _newton_run(monkeypatch, False)
    lin1, s1, lev1 = _newton_run(monkeypatch, True)
    dp = np.abs(s1.p - s0.p).max() / np.abs(s0.p).max()
    print("linear iterations full %s closed %s; perforated rows on level 0: %d of %d; max relative pressure difference %.3e, saturation difference %.3e"
          % (lin0, lin1, int((lev1 == 0).sum()), lev1.size, dp, np.abs(s1.sat - s0.sat).max()))
    assert (lev1 == 0).sum() >= 1 and np.array_equal(lev0, lev1)
    assert lin0[0] > 0 and lin1 == lin0
    assert dp <= 1e-9


def test_more_than_two_colours(gpu_lib, oracle, monkeypatch):
    """An irregular deck (inactive cells, NNCs): the NNCs break the 2-colouring, the level-0 rows are fewer than half and the later levels
    have lower entries on several earlier ones.  Measured: 4 levels, 54 columns in both runs, true residual 2.846630e-11 / 2.846235e-11: ratio 0.99986."""
    full, _ = _same_solve(monkeypatch, _system(oracle, "irregular"), 1e-10, **capi.CPR_AMG_VCYCLE)
    assert full["nlevels"] > 2


@pytest.mark.parametrize("single,kw", [(False, dict(cpr_stage2_relax=0.9)), (True, {}), (False, dict(newton_use_gmres=2)), (False, dict(gmres_verify_residual=1))],
                         ids=["stage2_relax_0.9", "float", "flexible", "verified"])
def test_exclusions_are_bit_for_bit(gpu_lib, oracle, monkeypatch, single, kw):
    """settings the closed form does not cover keep the explicit product: x is identical with the switch on and off"""
    prm = dict(capi.CPR_AMG_VCYCLE, linear_solver_reduction=1e-5 if single else 1e-10)
    prm.update(kw)
    gm = prm.pop("newton_use_gmres", 1)
    runs = []
    for closed in (False, True):
        monkeypatch.setenv("OPMGPU_CLOSED", "1" if closed else "0")
        rowptr, col, val, b, _ = _system(oracle, "b1")
        s = GpuNewtonIteration(capi.default_params(newton_use_gmres=gm, ilu_ordering=capi.ORDER_MULTICOLOR, linear_solver_maxiter=400, **prm))
        runs.append(s.computeNewtonIncrement(rowptr, col, val, b, single))
        assert s.iterations() > 0
        s.close()
    assert np.array_equal(runs[0], runs[1])
