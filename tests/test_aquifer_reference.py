"""The aquifer restatement (aquifer_reference.py) against closed forms and hand values: what makes it a yardstick for the device tests."""
import math

import numpy as np
import pytest

import aquifer_reference as AQ

EPS = 2.0 ** -52


def fetkovich(p_a0=250.0e5, CtV0=0.05, J=5.8e-9, n=3):
    alpha = np.arange(1.0, n + 1.0)
    return AQ.Aquifer(AQ.FETKOVICH, p_a0, 2000.0, CtV0=CtV0, J=J, cells=np.arange(n), alpha=alpha / alpha.sum())


@pytest.mark.parametrize("nsteps", [1, 2, 37])
@pytest.mark.parametrize("p_cell", [230.0e5, 262.0e5])
def test_fetkovich_tank_is_exact_for_any_substepping(nsteps, p_cell):
    """Against a constant cell pressure p, W_e(T) = CtV0 (p_a0 - p)(1 - exp(-T / tau)) after ANY sub-stepping of [0, T]: with u = p_a - p,
    one step gives u' = u - dt J E u / CtV0 = u (1 - x E) = u exp(-x), the exact decay.
    Bound: a step does fewer than 16 roundings (the quotients and products of the scalars, expm1, A_j, B_j p, their difference, dt Q,
    the sums), each at most eps relative to a quantity no larger than S = CtV0 max(|p_a0|, |p|) -- the size of A_j dt and B_j p dt BEFORE they
    cancel to the influx --, and the map u -> u exp(-x) is a contraction, so the errors of earlier steps do not grow: 16 N eps S, plus
    the same once for the closed form's own evaluation."""
    T = 300.0 * 86400.0
    a = fetkovich()
    tau = a.CtV0 / a.J
    rng = np.random.default_rng(nsteps)
    w = rng.uniform(0.2, 3.0, nsteps)
    dts = T * w / w.sum()
    for dt in dts:
        AQ.tank_step(a, dt, p_cell)
    exact = a.CtV0 * (a.p_a0 - p_cell) * -math.expm1(-T / tau)
    S = a.CtV0 * max(abs(a.p_a0), abs(p_cell))
    bound = 16 * (nsteps + 1) * EPS * S
    print("N = %d: W_e = %.17g, closed form %.17g, difference %.3g, bound %.3g" % (nsteps, a.We, exact, a.We - exact, bound))
    assert abs(a.We - exact) <= bound
    assert abs(a.t - T) <= nsteps * EPS * T
    assert a.Ws == pytest.approx(a.We, rel=1e-15)          # b_w = 1 in the tank


def test_fetkovich_small_x_keeps_its_digits():
    """E = -expm1(-x) / x at x = 1e-12: 1 - x / 2 to the last digit, where (1 - exp(-x)) / x has lost four"""
    a = fetkovich(CtV0=1.0e3, J=1.0e-9)
    sc = AQ.scalars(a, 1.0)
    assert sc["x"] == pytest.approx(1.0e-12, rel=1e-15)
    assert abs(sc["E"] - (1.0 - sc["x"] / 2.0)) <= 2 * EPS


def test_carter_tracy_tank_by_hand():
    """With the table P_D = t_D: P' = 1, den = t_D+ - t_D = dt / T_c, T_c den = dt, b = beta / dt, a_j = (beta dp - W_e) / dt.  All numbers
    below are exact in binary, so the comparison is exact too."""
    a = AQ.Aquifer(AQ.CARTER_TRACY, 100.0, 0.0, beta=2.0, Tc=4.0, td=[0.0, 1.0, 10.0], pd=[0.0, 1.0, 10.0], cells=[0, 1], alpha=[0.25, 0.75])
    sc, A, B, q = AQ.tank_step(a, 8.0, 90.0, bw=0.5)
    assert (sc["tD"], sc["tDp"], sc["Pp"], sc["P"], sc["den"], sc["Tden"], sc["b"]) == (0.0, 2.0, 1.0, 2.0, 2.0, 8.0, 0.25)
    assert np.array_equal(B, [0.0625, 0.1875])
    assert np.array_equal(A, [0.25 * 25.0, 0.75 * 25.0])            # alpha (a_j + b p0), a_j = (2 * 10 - 0) / 8 = 2.5
    assert np.array_equal(q, [0.625, 1.875])
    assert (a.We, a.Ws, a.t) == (20.0, 10.0, 8.0)
    assert a.p_a() == 90.0                                          # W_e = beta dp: this table fills the aquifer's deficit in one step
    sc, A, B, q = AQ.tank_step(a, 8.0, 90.0, bw=0.5)
    assert (sc["tD"], sc["tDp"], sc["den"], sc["Tden"]) == (2.0, 4.0, 2.0, 8.0)
    assert np.array_equal(q, [0.0, 0.0])                            # a_j = (2 * 10 - 20 * 1) / 8 = 0
    assert (a.We, a.t) == (20.0, 16.0)
    # a cell pressure that differs from the frozen one: q_j = alpha (a_j + b (p0 - pw))
    a.We = 4.0
    sc = AQ.scalars(a, 8.0)
    A, B = AQ.coefficients(a, sc, [0.0, 0.0], [90.0, 90.0], [0.0, 0.0], 0.0)
    assert np.array_equal(AQ.rates(A, B, [86.0, 90.0]), [0.25 * (2.0 + 0.25 * 4.0), 0.75 * 2.0])


def test_hydrostatic_head_and_datum():
    """h_j = (rho0 g)(z - d_a) enters p_a + h_j (Fetkovich) and p_a0 + h_j - p0_j (Carter-Tracy)"""
    f = AQ.Aquifer(AQ.FETKOVICH, 100.0, 10.0, CtV0=1.0, J=1.0, cells=[0], alpha=[1.0])
    sc = AQ.scalars(f, 1.0)
    A, B = AQ.coefficients(f, sc, [2.0], [0.0], [14.0], 0.5)
    assert A[0] == B[0] * (100.0 + 4.0)
    c = AQ.Aquifer(AQ.CARTER_TRACY, 100.0, 10.0, beta=2.0, Tc=4.0, td=[0.0, 1.0], pd=[0.0, 1.0], cells=[0], alpha=[1.0])
    sc = AQ.scalars(c, 8.0)
    A, B = AQ.coefficients(c, sc, [2.0], [90.0], [14.0], 0.5)
    assert AQ.rates(A, B, [90.0])[0] == 2.0 * 14.0 / 8.0


def test_table_rule_and_bad_den():
    td = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    assert [AQ.table_segment(td, x) for x in (0.0, 1.0, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 9.0)] == [0, 0, 0, 1, 2, 2, 3, 3, 3, 3]
    assert AQ.table_segment(np.array([1.0, 2.0]), 7.0) == 0
    # a convex table: P - t_D P' turns negative once t_D is large enough
    c = AQ.Aquifer(AQ.CARTER_TRACY, 100.0, 0.0, beta=2.0, Tc=1.0, td=[0.0, 1.0, 2.0], pd=[0.0, 1.0, 4.0], cells=[0], alpha=[1.0])
    c.t = 1.5
    with pytest.raises(ValueError, match="den"):
        AQ.scalars(c, 0.25)


def test_tree_sum_follows_the_documented_tree():
    """1, 63, 64, 65, 257 and 600 terms: equal to the plain sum for integers (exact in any order), and for terms whose order matters equal
    to the tree written out by hand"""
    for n in (1, 63, 64, 65, 257, 600):
        assert AQ.tree_sum(np.arange(1.0, n + 1.0)) == n * (n + 1) / 2
    v = np.zeros(300)
    v[0], v[256], v[32], v[64] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53
    # slot 0 = 1 + 2^-53 -> 1 (ties to even); + slot 32 (2^-53) -> 1; wave 1 = 2^-53; (1 + 2^-53) -> 1: every small term is lost one by one
    assert AQ.tree_sum(v) == 1.0
    assert math.fsum(v) > 1.0
