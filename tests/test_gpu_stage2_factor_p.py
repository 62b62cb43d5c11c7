"""The top level's stage-2 pressure residual sent through the ILU0 factor (LinSolver::cpr_factor_p, k_cpr_presidual_l0, k_ilu_lower's FP form;
DESIGN section 5).  Every case builds two contexts in one process, one with OPMGPU_CPR_FACTOR_P=0 (the full-grid residual and the plain
forward sweep) and one with 1 (the default); the switch is read when the context is created.

The path rounds differently from the plain sequence.  The operator cases compare one application (opmgpu_cpr_apply behind a double GMRES
solve, which leaves the context on the solve's path) with the switch on against off; the bound is the relative 2-norm difference 1e-12,
the f64 bound of tests/test_gpu_cpr_stages.py for the whole application against its float64 restatement (measured there: <= 8.2e-14).
Control for the bound: the sweep WITHOUT its diagonal term A_ii[:,0] x_p,i on the top rows, restated from the exported pieces (the
Jacobian, the CPR weights, opmgpu_cpr_vcycle_apply, the ordering) and the oracle's block ILU0, must lie at least 100 x the bound away.
The solve cases make the statements of tests/test_gpu_lean_solve.py for OPMGPU_CPR_CANCEL_P, with its bounds and on its decks, and
np.array_equal wherever the path's conditions do not hold.

Measured (MI355X) figures are recorded in the docstrings; each case prints its own (-s)."""
import numpy as np
import pytest

import amg_reference as ar
import test_gpu_cpr_stages as stages
import test_gpu_gmres_closed_form as closed_form
import test_gpu_lean_solve as lean
from opmgpu import capi, decks
from opmgpu import wells as W
from opmgpu.model import GpuNewtonIteration
from util import bsr_to_scipy

pytestmark = pytest.mark.gpu

FACTOR, CANCEL = "OPMGPU_CPR_FACTOR_P", "OPMGPU_CPR_CANCEL_P"
TOL = 1e-12          # tests/test_gpu_cpr_stages.py, TOL[False]

_systems = {}


def _ragged_system(oracle):
    """13 x 11 x 7 = 1 001 rows, two colours of 501 and 500 rows: no multiple of 64 or 256, so the last wave, slice and chunk of both
    levels are ragged, and the slice at the boundary holds rows of both levels"""
    if "ragged" not in _systems:
        grid = decks.cartesian_grid(13, 11, 7, lognormal_sigma=0.8)
        tab = decks.satfunc_standard_tables()
        st = decks.initial_state(grid, tab, perturb=0.01)
        scale = np.asarray(capi.default_params().matbalscale[:])
        rowptr, col = oracle.pattern(grid)
        nc = grid.nc
        r, val, _, _ = oracle.assemble(grid, tab, 5 * decks.DAY, st, rowptr, col, scale=tuple(scale))
        b = np.ascontiguousarray((r * np.repeat(scale, nc)).reshape(3, nc).T).ravel()
        _systems["ragged"] = (rowptr, col, val, b, bsr_to_scipy(rowptr, col, val))
    return _systems["ragged"]


def _b1_context(system):
    rowptr, col, val, b, _ = system
    s = GpuNewtonIteration(capi.default_params(newton_use_gmres=1, ilu_ordering=capi.ORDER_MULTICOLOR, linear_solver_maxiter=400, linear_solver_reduction=1e-10,
                                               **capi.CPR_AMG_VCYCLE))
    s.computeNewtonIncrement(rowptr, col, val, b, False)
    assert s.iterations() > 0
    return s, (rowptr, col, val)


def _model_context():
    gm = stages._model((9, 9, 12), False, newton_use_gmres=1)
    return gm, gm.jacobian()


def _right_hand_sides(obj, J, nb):
    """a random vector and an algebraically smooth one (ten damped Jacobi sweeps on level 0 of the pressure hierarchy, through J), seeded"""
    n, _, _ = obj.cpr_levels()
    A0 = ar.csr(*obj.cpr_level(0)[:3], n[0])
    rng = np.random.default_rng(11)
    s = rng.standard_normal(n[0])
    Dinv = ar.inv_diag(A0)
    for _ in range(10):
        s = s - 0.9 * Dinv * (A0 @ s)
    return {"random": rng.standard_normal(3 * nb), "smooth": J @ np.repeat(s[:nb], 3)}


def _without_diagonal_term(obj, oracle, rowptr, col, val, d3, v_on):
    """what the application gives when the top rows' sweep leaves A_ii[:,0] x_p,i out: the sweeps are linear, so that is
    v + ILU0^-1 e with e_i = A_ii[:,0] x_p,i on the top rows and 0 on level 0.  x_p = V-cycle(sum_eq w_eq d_eq) from the exports (no coarse
    space on these decks: an external matrix, or wells), ILU0 the oracle's in the device's elimination order"""
    nb = rowptr.size - 1
    pos, lev, nlev = obj.ordering()
    assert nlev == 2
    w = stages._weights(obj, nb)
    n, _, nw = obj.cpr_levels()
    d = np.asarray(d3).reshape(nb, 3)
    xp = obj.cpr_vcycle_apply(np.concatenate([w[0] * d[:, 0] + w[1] * d[:, 1] + w[2] * d[:, 2], np.zeros(nw)]))[:nb]
    rows = np.repeat(np.arange(nb), np.diff(rowptr))
    diag = np.asarray(val).reshape(-1, 3, 3)[col == rows]
    assert diag.shape[0] == nb
    e = diag[:, :, 0] * xp[:, None] * (lev == 1)[:, None]
    st, lu = oracle.ilu0(rowptr, col, val, position=pos, single=False)
    assert st == 0
    return v_on + oracle.ilu0_apply(rowptr, col, lu, e.ravel(), position=pos, relax=1.0, single=False)


def _operator_case(monkeypatch, oracle, make, case, perforated=None):
    ctx = {}
    for on in (False, True):
        monkeypatch.setenv(FACTOR, "1" if on else "0")
        ctx[on], (rowptr, col, val) = make()
    off, new = ctx[False], ctx[True]
    nb = rowptr.size - 1
    pos, lev, nlev = new.ordering()
    assert nlev == 2
    n0 = int((lev == 0).sum())
    print("%s: %d rows, level 0 %d, top level %d" % (case, nb, n0, nb - n0))
    if perforated is not None:
        pl = lev[np.asarray(perforated)]
        print("%s: perforated rows on level 0: %d, on the top level: %d" % (case, int((pl == 0).sum()), int((pl == 1).sum())))
        assert (pl == 0).any() and (pl == 1).any()
    out = {}
    for name, d3 in _right_hand_sides(new, stages._bsr(rowptr, col, val), nb).items():
        v0, v1 = off.cpr_apply(d3), new.cpr_apply(d3)
        assert np.array_equal(v1, new.cpr_apply(d3)), (case, name)          # the same bits twice
        vc = _without_diagonal_term(new, oracle, rowptr, col, val, d3, v1)
        e = stages._rel(v1, v0)
        margin = stages._rel(vc, v0) / TOL
        print("%s %s: switch on against off %.3e (bound %.0e); without the diagonal term %.3e = %.0f x the bound" % (case, name, e, TOL, margin * TOL, margin))
        assert np.abs(v0).max() > 0 and not np.array_equal(v0, v1), (case, name)          # (the path ran: it rounds differently)
        assert e <= TOL, (case, name, e)
        assert margin >= 100, (case, name, margin)
        out[name] = v1
    off.close()
    new.close()
    return out, (n0, nb - n0)


# ---------------------------------------------------------------- the operator, switch on against off
def test_operator_b1(gpu_lib, oracle, monkeypatch):
    """opmgpu_cpr_apply on the 12 x 10 x 8 system of the lean-solve tests (960 rows, 480 + 480).  Measured: 1.7e-16 on both vectors, the
    control at 1.33 / 1.35 relative."""
    _operator_case(monkeypatch, oracle, lambda: _b1_context(closed_form._system(oracle, "b1")), "b1_12x10x8")


def test_operator_ragged_levels(gpu_lib, oracle, monkeypatch):
    """13 x 11 x 7: 1 001 rows, levels of 501 and 500 rows.  Measured: 1.6e-16 on both vectors, the control at 1.33 relative."""
    _, levels = _operator_case(monkeypatch, oracle, lambda: _b1_context(_ragged_system(oracle)), "b1_13x11x7")
    assert levels == (501, 500)


def test_operator_with_device_wells(gpu_lib, oracle, monkeypatch):
    """9 x 9 x 12 with its device 5-spot (full columns: perforated rows on both colours), the model's own assembly and bordered level 0.
    Measured: 30 perforated rows on each level, 1.8e-16 / 1.7e-16, the control at 0.95 / 1.44 relative."""
    grid = decks.cartesian_grid(9, 9, 12, lognormal_sigma=0.5)
    wl = W.five_spot(grid, rate_m3_per_day=40.0, bhp_prod_bar=150.0)
    _operator_case(monkeypatch, oracle, _model_context, "model_9x9x12_wells", perforated=wl.cells)


# ---------------------------------------------------------------- the solve: the statements made for OPMGPU_CPR_CANCEL_P
def _same_solve(monkeypatch, system, red, **kw):
    plain = lean._solve(monkeypatch, FACTOR, False, system, linear_solver_reduction=red, **kw)
    new = lean._solve(monkeypatch, FACTOR, True, system, linear_solver_reduction=red, **kw)
    print("iterations plain %d factor-p %d; reduction plain %.3e factor-p %.3e; true residual plain %.6e factor-p %.6e (ratio %.6f); levels %d"
          % (plain["iterations"], new["iterations"], plain["reduction"], new["reduction"], plain["true"], new["true"], new["true"] / plain["true"], plain["nlevels"]))
    assert new["iterations"] == plain["iterations"]
    assert plain["reduction"] < red and new["reduction"] < red
    assert new["true"] <= 1.05 * plain["true"]
    return plain, new


@pytest.mark.parametrize("kw", [{}, dict(linear_solver_restart=3)], ids=["gmres40", "restart3"])
def test_solve(gpu_lib, oracle, monkeypatch, kw):
    """CPR + GMRES in double to 1e-10 on the 12 x 10 x 8 system (a two-level plan): equal column counts, both below the reduction, the true
    residual ||b - A x|| / ||b|| within 5 % of the plain sequence's.  Measured: 20 columns in both runs, 1.761569e-11 (plain) /
    1.761053e-11: ratio 0.999707; restart 3: 36 columns, 4.570775e-12 / 4.435253e-12: ratio 0.970350."""
    plain, new = _same_solve(monkeypatch, closed_form._system(oracle, "b1"), 1e-10, **dict(capi.CPR_AMG_VCYCLE, **kw))
    assert plain["nlevels"] == 2
    assert not np.array_equal(plain["x"], new["x"])          # (the path ran)


def test_newton_with_wells(gpu_lib, monkeypatch):
    """three (and a fourth) Newton iterations with device wells on 10 x 10 x 4: the same linear iterations, pressures equal to 1e-12 relative.
    Measured: [3, 6, 5, 4] in both runs, largest relative pressure difference 6.3e-16, saturation difference 1.4e-14."""
    lin0, _, _, a4, _ = lean._newton_run(monkeypatch, FACTOR, False)
    lin1, _, _, b4, _ = lean._newton_run(monkeypatch, FACTOR, True)
    dp = np.abs(b4.p - a4.p).max() / np.abs(a4.p).max()
    print("linear iterations plain %s factor-p %s; max relative pressure difference %.3e, saturation difference %.3e" % (lin0, lin1, dp, np.abs(b4.sat - a4.sat).max()))
    assert lin0[0] > 0 and lin1 == lin0
    assert dp <= 1e-12


# ---------------------------------------------------------------- the path switches itself off
@pytest.mark.parametrize("name,gmres,single,kw,env", [("irregular", 1, False, {}, {}), ("b1", 1, False, dict(cpr_stage2_relax=0.9), {}), ("b1", 1, False, dict(cpr_relax=0.9), {}),
                                                      ("b1", 1, True, {}, {}), ("b1", 1, False, dict(preconditioner_single=1), {}), ("b1", 0, False, {}, {}),
                                                      ("b1", 1, False, {}, {CANCEL: "0"})],
                         ids=["four_levels", "stage2_relax_0.9", "cpr_relax_0.9", "float", "preconditioner_single", "bicgstab", "cancel_p_0"])
def test_conditions(gpu_lib, oracle, monkeypatch, name, gmres, single, kw, env):
    """more than two levels, a relaxation factor other than 1, a float solve, a float preconditioner in a double solve, BiCGStab, the
    cancellation switched off: the plain sequence, bit for bit, and the same iteration count.  Measured: 54 / 20 / 20 / 11 / 20 / 12 / 20."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    off, _ = lean._identical(monkeypatch, FACTOR, closed_form._system(oracle, name), gmres=gmres, single=single, linear_solver_reduction=1e-5 if single else 1e-10,
                             **dict(capi.CPR_AMG_VCYCLE, **kw))
    assert off["iterations"] > 0
    if name == "irregular":
        assert off["nlevels"] > 2


def test_two_runs_identical(gpu_lib, oracle, monkeypatch):
    """two solves with the switch on, each in a context of its own: identical bits and iteration counts"""
    system = closed_form._system(oracle, "b1")
    a = lean._solve(monkeypatch, FACTOR, True, system, linear_solver_reduction=1e-10, **capi.CPR_AMG_VCYCLE)
    b = lean._solve(monkeypatch, FACTOR, True, system, linear_solver_reduction=1e-10, **capi.CPR_AMG_VCYCLE)
    assert a["iterations"] == b["iterations"] > 0
    assert np.array_equal(a["x"], b["x"])
