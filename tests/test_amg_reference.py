"""The float64 restatement of the CPR pressure stage (tests/amg_reference.py) checked on its own, before any kernel is checked against
it: on a small hand-built matrix with a given aggregation its V-cycle equals the explicit product of the two-grid operators."""
import numpy as np
import scipy.sparse as sp

import amg_reference as ar


def _matrix(n=14, seed=3):
    """a non-symmetric, diagonally dominant M-matrix-like pressure operator (1-D chain plus a few long couplings)"""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for i in range(n - 1):
        t = rng.uniform(0.5, 2.0)
        A[i, i + 1] -= t
        A[i + 1, i] -= t * rng.uniform(0.8, 1.2)
    for i, j in ((0, 7), (3, 11), (5, 13)):
        A[i, j] -= 0.3
        A[j, i] -= 0.25
    A[np.diag_indices(n)] = -A.sum(axis=1) + rng.uniform(0.05, 0.2, n)
    return sp.csr_matrix(A)


def test_two_level_cycle_is_the_explicit_operator():
    A = _matrix()
    n = A.shape[0]
    agg = np.array([0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 4, 4])
    H = ar.Hierarchy(A, [agg])
    assert len(H.A) == 2 and H.inv is not None
    P = ar.prolongation(agg).toarray()
    Ad = A.toarray()
    Ac = P.T @ Ad @ P
    assert np.allclose(H.A[1].toarray(), Ac, rtol=0, atol=1e-14 * np.abs(Ad).sum())
    I = np.eye(n)
    rng = np.random.default_rng(7)
    for omega, pd, npre, npost in ((0.9, 1.9, 1, 2), (0.7, 1.0, 2, 1), (0.9, 2.2, 1, 0)):
        S = I - omega * np.diag(1.0 / np.diag(Ad)) @ Ad
        E = np.linalg.matrix_power(S, npost) @ (I - pd * P @ np.linalg.inv(Ac) @ P.T @ Ad) @ np.linalg.matrix_power(S, npre)
        V = (I - E) @ np.linalg.inv(Ad)          # the cycle from a zero start: x = (I - E) A^-1 b
        for _ in range(3):
            b = rng.standard_normal(n)
            x = H.vcycle(b, omega=omega, pdamp0=pd, pdamp=pd, npre=npre, npost=npost)
            assert np.linalg.norm(x - V @ b) <= 1e-13 * np.linalg.norm(V @ b)
        # linear in b
        b1, b2 = rng.standard_normal(n), rng.standard_normal(n)
        lhs = H.vcycle(2.0 * b1 - 3.0 * b2, omega=omega, pdamp0=pd, pdamp=pd, npre=npre, npost=npost)
        rhs = 2.0 * H.vcycle(b1, omega=omega, pdamp0=pd, pdamp=pd, npre=npre, npost=npost) - 3.0 * H.vcycle(b2, omega=omega, pdamp0=pd, pdamp=pd, npre=npre, npost=npost)
        assert np.linalg.norm(lhs - rhs) <= 1e-13 * np.linalg.norm(lhs)


def test_gauss_seidel_by_colour_is_the_explicit_operator():
    """level-0 Gauss-Seidel by colour: rows of one colour do not couple, so a colour's update is one block of a block Gauss-Seidel sweep"""
    n = 12
    A = np.zeros((n, n))
    for i in range(n - 1):
        A[i, i + 1] = A[i + 1, i] = -1.0 - 0.1 * i
    A[np.diag_indices(n)] = -A.sum(axis=1) + 0.1
    first = np.arange(n) % 2 == 0
    agg = np.arange(n) // 3
    H = ar.Hierarchy(sp.csr_matrix(A), [agg])
    P = ar.prolongation(agg).toarray()
    Ac = P.T @ A @ P
    I = np.eye(n)
    D = np.diag(np.diag(A))

    def colour_sweep(c):          # error propagation of x[c] += D_c^-1 (b - A x)[c]
        M = np.zeros((n, n))
        M[np.ix_(c, c)] = np.linalg.inv(D[np.ix_(c, c)])
        return I - M @ A
    S1, S2 = colour_sweep(first), colour_sweep(~first)
    pd = 1.9
    E = (S1 @ S2) @ (S1 @ S2) @ (I - pd * P @ np.linalg.inv(Ac) @ P.T @ A) @ (S2 @ S1)
    V = (I - E) @ np.linalg.inv(A)
    b = np.random.default_rng(1).standard_normal(n)
    x = H.vcycle(b, pdamp0=pd, pdamp=pd, npost0=2, gs_first=first)
    assert np.linalg.norm(x - V @ b) <= 1e-13 * np.linalg.norm(V @ b)


def test_sensitivity_controls_move_the_cycle():
    """the perturbations the GPU tests use as controls change the restated cycle by far more than any tolerance there"""
    A = _matrix(40, seed=5)
    agg = np.arange(40) // 4
    b = np.random.default_rng(2).standard_normal(40)
    H = ar.Hierarchy(A, [agg])
    x = H.vcycle(b)
    for y in (H.vcycle(b, omega=0.905), H.vcycle(b, pdamp0=1.9 * 1.01, pdamp=1.9 * 1.01), ar.Hierarchy(A, [agg], drop=(0, 0)).vcycle(b)):
        assert np.linalg.norm(y - x) >= 1e-4 * np.linalg.norm(x)


def test_point_ilu0_is_exact_on_a_triangular_pattern_and_matches_lu_without_fill():
    """the restated point ILU0: on a tridiagonal matrix (no fill in any order that keeps the chain) it is the exact LU solve; in a
    permuted order its factors reproduce A on A's pattern"""
    n = 9
    A = np.diag(np.full(n, 4.0)) + np.diag(np.full(n - 1, -1.0), 1) + np.diag(np.full(n - 1, -1.5), -1)
    b = np.arange(1.0, n + 1)
    x = ar.point_ilu0_apply(sp.csr_matrix(A), np.arange(n), b, relax=0.5)
    assert np.allclose(x, 0.5 * np.linalg.solve(A, b), rtol=1e-13, atol=0)
    # red-black order of the chain: fill would land outside the pattern; (L U)(i, j) == A(i, j) on the pattern
    order = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
    pos = np.empty(n, int); pos[order] = np.arange(n)
    y = np.array([ar.point_ilu0_apply(sp.csr_matrix(A), pos, e) for e in np.eye(n)]).T          # (L U)^-1 in the original numbering
    M = np.linalg.inv(y)
    assert np.allclose(M[A != 0], A[A != 0], rtol=1e-13, atol=1e-13)
