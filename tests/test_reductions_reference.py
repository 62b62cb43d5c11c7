"""CPU: the float64 restatement of getConvergence / relativeChange (tests/reductions_reference.py) against the oracle's own loops, its
status rules, its error bounds, and the conditioning of the decks tests/test_gpu_reductions.py runs on the device: every planted change
and every single 1/b term must stand far above the bound of the sum it is meant to move, or a dropped row could hide in the tolerance."""
import math

import numpy as np
import pytest

from opmgpu import capi, decks

import reductions_reference as ref


def _small(seed=3, nc=37):
    rng = np.random.default_rng(seed)
    base = decks.cartesian_grid(nc, 1, 1, lognormal_sigma=0.5)
    grid = decks.GridData(nc, base.conn_cells, base.trans, base.pv * rng.uniform(0.5, 2.0, nc), base.z, dims=base.dims)
    R = rng.standard_normal((3, nc)) * np.array([[1e-3], [2e-2], [5.0]])
    binv = rng.uniform(0.5, 1.5, (3, nc)) * np.array([[1.0], [1.0], [5e-3]])
    return grid, R, binv


def test_matches_the_oracle_on_non_uniform_pore_volumes(oracle):
    grid, R, binv = _small()
    assert np.ptp(grid.pv) > 0.5 * grid.pv.min()
    prm = capi.default_params()
    dt = 3 * decks.DAY
    want = oracle.convergence(grid, prm, dt, R.ravel(), binv.ravel())
    got = ref.convergence_scalars(R, binv, grid.pv, dt, prm)
    assert want[0] == got.status == capi.OK and want[5] == got.converged
    for a, b in zip(want[1:5], (got.B, got.CNV, got.MB, got.linf)):
        assert np.allclose(a, b, rtol=1e-13, atol=0.0)
    assert np.array_equal(got.linf, np.abs(R).max(1))
    # with uniform pore volumes the row of max |R| / pv is the row of max |R|: here it is not, for at least one phase
    assert (got.argmaxRpv != np.abs(R).argmax(1)).any()
    # a residual small enough converges, on both sides
    small = R * 1e-12
    assert oracle.convergence(grid, prm, dt, small.ravel(), binv.ravel())[5] and ref.convergence_scalars(small, binv, grid.pv, dt, prm).converged


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("phase", [0, 1, 2])
def test_non_finite_residual_is_a_numerical_issue(oracle, value, phase):
    grid, R, binv = _small()
    prm = capi.default_params()
    R[phase, 11] = value
    assert oracle.convergence(grid, prm, decks.DAY, R.ravel(), binv.ravel())[0] == capi.ENUMERICAL
    assert ref.convergence_scalars(R, binv, grid.pv, decks.DAY, prm).status == capi.ENUMERICAL


def test_max_residual_allowed_is_a_numerical_issue(oracle):
    grid, R, binv = _small()
    dt = decks.DAY
    got = ref.convergence_scalars(R, binv, grid.pv, dt, capi.default_params())
    worst = max(got.CNV.max(), got.MB.max())
    for factor, status in ((2.0, capi.OK), (0.5, capi.ENUMERICAL)):
        prm = capi.default_params(max_residual_allowed=factor * worst)
        assert oracle.convergence(grid, prm, dt, R.ravel(), binv.ravel())[0] == status
        assert ref.convergence_scalars(R, binv, grid.pv, dt, prm).status == status


def test_relative_change_restatement():
    grid = decks.cartesian_grid(9, 1, 1)
    tab = decks.satfunc_standard_tables()
    a, b = decks.random_state(grid, tab, seed=1), decks.random_state(grid, tab, seed=2)
    value, num, den = ref.relative_change(a, b)
    plain = (((a.p - b.p) ** 2).sum() + ((a.sat - b.sat) ** 2).sum()) / ((b.p ** 2).sum() + (b.sat ** 2).sum())
    assert value == pytest.approx(plain, rel=1e-14) and num > 0 and den > 0
    assert ref.relative_change(a, a)[0] == 0.0
    zero = decks.State(np.zeros(9), np.zeros((9, 3)), a.rs, a.rv, a.hc)
    assert ref.relative_change(a, zero) == (0.0, pytest.approx(ref.relative_change(zero, a)[2]), 0.0)      # new norm 0: 0, not a division


def test_error_bounds():
    assert ref.gamma(0) == 0.0 and ref.gamma(1) == pytest.approx(ref.U) and ref.gamma(524288) == pytest.approx(524288 * ref.U, rel=1e-9)
    # a sum in an adversarial order stays inside the bound, and the bound is not slack by orders of magnitude
    rng = np.random.default_rng(0)
    x = rng.standard_normal(4097) * 10.0 ** rng.uniform(-6, 6, 4097)
    exact = math.fsum(x.tolist())
    worst = 0.0
    for order in (np.argsort(np.abs(x)), np.argsort(-np.abs(x)), np.arange(x.size)):
        s = 0.0
        for v in x[order]:
            s += v
        worst = max(worst, abs(s - exact))
    bound = ref.gamma(x.size - 1) * np.abs(x).sum()
    assert worst <= bound and worst > 1e-6 * bound
    grid, R, binv = _small()
    r = ref.convergence_scalars(R, binv, grid.pv, decks.DAY, capi.default_params())
    t = ref.tolerances(r)
    assert t.B_rtol == ref.gamma(36) + 8 * ref.U and np.array_equal(t.Rsum_atol, ref.gamma(36) * r.sumabsR)
    assert np.all(t.MB_atol > (r.B * r.dt / r.pvsum) * t.Rsum_atol) and np.all(t.MB_atol < 1e-13 * (r.B * r.dt / r.pvsum) * r.sumabsR)
    assert np.all(t.absRsum_atol >= t.Rsum_atol)


def test_target_rows_and_plans():
    assert ref.SECOND_FINAL_TRIP == 65537 and ref.PAST_GRID_CAP == 524289
    assert ref.target_rows(1).tolist() == [0] and ref.target_rows(2).tolist() == [0, 1] and ref.target_rows(64).tolist() == [0, 63]
    assert ref.target_rows(513).tolist() == [0, 63, 64, 255, 256, 512]
    assert ref.target_rows(65537).tolist() == [0, 63, 64, 255, 256, 65535, 65536]
    assert ref.target_rows(524289).tolist() == [0, 63, 64, 255, 256, 262144, 524287, 524288]
    for ordering in (capi.ORDER_NATURAL, capi.ORDER_MULTICOLOR):
        for nc in (1, 2, 65, 513):
            cell_of_row, pos = ref.plan_rows(nc, ordering)
            assert np.array_equal(pos[cell_of_row], np.arange(nc))          # pos[cell] = row, cell_of_row its inverse
            if ordering == capi.ORDER_NATURAL:
                assert np.array_equal(pos, np.arange(nc))
    # red-black on a column: the even cells, then the odd ones -- the last ROW is not the last cell
    cell_of_row, _ = ref.plan_rows(513, capi.ORDER_MULTICOLOR)
    assert cell_of_row[0] == 0 and cell_of_row[256] == 512 and cell_of_row[257] == 1 and cell_of_row[512] == 511


@pytest.mark.parametrize("nc", [2, 257, ref.SECOND_FINAL_TRIP, ref.PAST_GRID_CAP])
def test_the_device_decks_are_well_conditioned(oracle, nc):
    """Detectability, from reference data alone: on the decks of the device tests every single 1/b term and every planted residual
    stands more than 1000 tolerances above the sum it belongs to, and the planted maxima sit where plants() says."""
    case = ref.column_case(nc, capi.ORDER_MULTICOLOR)
    grid = case.grid
    assert grid.pv.min() >= 0.5 * 0.2 * 200.0 and grid.pv.max() <= 2.0 * 0.2 * 200.0 and len(set(grid.pv[case.cells])) == case.cells.size
    tab = decks.satfunc_standard_tables()
    st = decks.random_state(grid, tab, seed=11)
    oracle.set_threads(16)
    props = oracle.cell_props(grid, tab, st)
    binv = np.stack([1.0 / props[:, oracle.PROP_NAMES.index("b_" + c), 0] for c in "wog"])
    g = ref.gamma(nc - 1)
    for a in range(3):
        assert binv[a].min() > ref.DETECTABLE * (g + ref.SCALAR) * math.fsum(binv[a].tolist()), a
    # a residual of the size the assembly produces is not needed for the plants' conditioning: any R works, the plants scale with it
    rng = np.random.default_rng(nc)
    R = rng.standard_normal((3, nc)) * np.array([[1e-3], [2e-2], [5.0]])
    prm = capi.default_params()
    before = ref.convergence_scalars(R, binv, grid.pv, decks.DAY, prm)
    seen_linf, seen_cnv = set(), set()
    ipv = 1.0 / grid.pv
    for a, k, j, delta in ref.plants(case, R):
        Rp = R[a].copy()
        Rp[case.cells] += delta[:, a]
        absR = np.abs(Rp)
        assert int(absR.argmax()) == case.cells[k] and int((absR * ipv).argmax()) == case.cells[j]
        assert absR[case.cells[k]] > np.delete(absR, case.cells[k]).max()                     # strict
        after = ref.with_replaced(before, a, R[a, case.cells], Rp[case.cells])
        if nc <= 257:                                                                          # the shortcut against the sums themselves
            full = ref.convergence_scalars(np.where(np.arange(3)[:, None] == a, Rp, R), binv, grid.pv, decks.DAY, prm)
            assert after.Rsum[a] == pytest.approx(full.Rsum[a], rel=1e-14) and after.sumabsR[a] == pytest.approx(full.sumabsR[a], rel=1e-14)
            assert full.argmaxRpv[a] == case.cells[j] and full.linf[a] == absR.max()
        planted = delta[:, a].sum()
        tol = ref.tolerances(before).absRsum_atol[a] + ref.tolerances(after).absRsum_atol[a] + 2 * ref.U * absR.max()
        assert abs(planted) > ref.DETECTABLE * tol
        assert abs(after.Rsum[a]) - abs(before.Rsum[a]) == pytest.approx(abs(planted), abs=tol)
        seen_linf.add(k); seen_cnv.add(j)
    K = case.cells.size
    assert seen_linf == set(range(K)) and len(seen_cnv) == max(K - 1, 1)                      # every target carries max |R| once
