"""The schedule of the ILU0 factorisation (LinSolver::factor_ahead, LinSolver::solve) changes WHEN the factorisation runs, not
what is computed.  Three schedules, each read when the context is created: the default (the factorisation starts at the end of the
assembly, on its own stream), OPMGPU_FACTOR_EARLY=0 (it starts inside the solve, behind the pressure stage's pass over the matrix) and
OPMGPU_FACTOR_OVERLAP=0 (it runs on the solve's own stream).  The same kernels run on the same inputs in all three; only the stream and the
starting point differ, so every check is an equality."""
import numpy as np
import pytest

from opmgpu import capi, decks
from opmgpu import wells as W
from opmgpu.model import GpuBlackoilModel, NonlinearSolver

pytestmark = pytest.mark.gpu

SCHEDULES = [("default", None), ("early_off", "OPMGPU_FACTOR_EARLY"), ("overlap_off", "OPMGPU_FACTOR_OVERLAP")]

SETS = {
    "gmres_double": (dict(newton_use_gmres=1), False),
    "bicgstab_float": (dict(newton_use_gmres=0), True),
    "gmres_mixed": (dict(newton_use_gmres=1, preconditioner_single=1), False),
}


def _newton_run(monkeypatch, switch, prm, single):
    """test_gpu_lean_solve._newton_run with the schedule's switch set around the constructor: three Newton iterations of the 10 x 10 x 4 deck
    with the device five-spot through nonlinearIteration, then a fourth matrix whose increment is read through opmgpu_solve(..., dx)"""
    if switch:
        monkeypatch.setenv(switch, "0")
    grid = decks.cartesian_grid(10, 10, 4, lognormal_sigma=0.5)
    tab = decks.satfunc_standard_tables()
    st = decks.initial_state(grid, tab, perturb=0.01)
    wl = W.five_spot(grid, rate_m3_per_day=20.0, bhp_prod_bar=150.0)
    gm = GpuBlackoilModel(grid, tab, capi.default_params(**dict(capi.CPR_AMG_VCYCLE, **prm)))
    if switch:
        monkeypatch.delenv(switch)
    m = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    m.prepareStep(decks.DAY, st)
    ns = NonlinearSolver()
    lin = [m.nonlinearIteration(it, single_precision=single, nonlinear_solver=ns)[1] for it in range(3)]
    s3 = gm.getState()
    gm.setSolvePrecision(single)
    gm.assemble(False)
    gm.getConvergence()
    dx = gm.solveJacobianSystem(want_dx=True, single_precision=single)
    lin.append(gm.linear_iterations)
    gm.close()
    return lin, s3, dx


@pytest.mark.parametrize("name", list(SETS))
def test_schedule_keeps_every_bit(gpu_lib, monkeypatch, name):
    """CPR + GMRES in double, CPR + BiCGStab in float (the Jacobian assembled as float), CPR + GMRES in double with the preconditioner in
    float: the linear iterations of every Newton iteration, the state after three of them and the fourth matrix's increment are equal
    under the three schedules."""
    prm, single = SETS[name]
    runs = {tag: _newton_run(monkeypatch, switch, prm, single) for tag, switch in SCHEDULES}
    lin0, s0, dx0 = runs["default"]
    print("%s: linear iterations %s; |dx| %.3e" % (name, {t: r[0] for t, r in runs.items()}, np.abs(dx0).max()))
    assert all(k > 0 for k in lin0) and np.abs(dx0).max() > 0
    for tag in ("early_off", "overlap_off"):
        lin, s, dx = runs[tag]
        assert lin == lin0, tag
        for f in ("p", "sat", "rs", "rv", "hc"):
            assert np.array_equal(getattr(s, f), getattr(s0, f)), (tag, f)
        assert np.array_equal(dx, dx0), tag
