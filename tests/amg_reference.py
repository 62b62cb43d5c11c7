"""float64 restatement of the CPR pressure stage, numpy / scipy only.

It takes level 0 and the aggregates as the library reports them (opmgpu_cpr_level_get: the aggregation is host code and is checked for
its invariants, not restated) and builds from them, in float64:
  * the piecewise-constant prolongation P_l of every level and the Galerkin operators A_{l+1} = P_l^T A_l P_l;
  * the coarsest solve: the explicit inverse (n <= 96), else `coarse_sweeps` pairs of damped-Jacobi sweeps;
  * one V-cycle from a zero start: damped Jacobi (omega) with `npre` sweeps before and `npost` after the coarse-grid correction
    (`npost0` on level 0), the correction scaled by `pdamp0` into level 0 and by `pdamp` below, or Gauss-Seidel by colour on level 0;
  * the two-stage CPR application: pressure right-hand side, optional global-constant correction, the cycle, the full-system residual,
    stage 2 through a caller-supplied block ILU0 application, and the relaxed pressure correction.
The smoother constants are the documented ones unless a case overrides them; nothing is read back from the device but the correction
factors the run-time policy chose.
"""
import numpy as np
import scipy.sparse as sp

OMEGA = 0.9           # damped-Jacobi weight
NPRE, NPOST = 1, 2    # sweeps before / after the coarse-grid correction
COARSE_SWEEPS = 4     # pairs of Jacobi sweeps standing in for a coarsest level above DENSE_MAX
DENSE_MAX = 96        # largest coarsest level with an explicit inverse


def csr(rowptr, col, val, n):
    """CSR of an exported level (entries at the same position are summed)"""
    A = sp.csr_matrix((np.asarray(val, float), np.asarray(col), np.asarray(rowptr)), shape=(n, n))
    A.sum_duplicates()
    return A


def prolongation(agg, nc=None):
    agg = np.asarray(agg)
    n = agg.size
    nc = int(agg.max()) + 1 if nc is None else nc
    return sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, nc))


def inv_diag(A):
    d = A.diagonal()
    out = np.zeros_like(d)
    nz = d != 0
    out[nz] = 1.0 / d[nz]
    return out


class Hierarchy:
    """Levels A_0 .. A_L from A_0 and the aggregates of levels 0 .. L-1.

    drop = (i, j): the fine entry (i, j) of level 0 is left out of the level-1 sum (a sensitivity control: a Galerkin kernel that lost one
    contribution)."""

    def __init__(self, A0, aggs, drop=None):
        self.A = [sp.csr_matrix(A0, dtype=float)]
        self.P = []
        for l, agg in enumerate(aggs):
            P = prolongation(agg)
            Ac = (P.T @ self.A[-1] @ P).tocsr()
            if l == 0 and drop is not None:
                i, j = drop
                Ac = Ac.tolil()
                Ac[agg[i], agg[j]] -= self.A[0][i, j]
                Ac = Ac.tocsr()
            self.P.append(P)
            self.A.append(Ac)
        self.dinv = [inv_diag(A) for A in self.A]
        nc = self.A[-1].shape[0]
        self.inv = np.linalg.inv(self.A[-1].toarray()) if nc <= DENSE_MAX else None

    def vcycle(self, b, omega=OMEGA, pdamp0=1.9, pdamp=1.9, npre=NPRE, npost=NPOST, npost0=None, coarse_sweeps=COARSE_SWEEPS, gs_first=None):
        """x = V(b) from a zero start.  gs_first: boolean mask of level 0's first colour -> Gauss-Seidel by colour on level 0 (the
        library's OPMGPU_AMG_GS; its second colour is updated first on the way down, both in reverse order on the way up)."""
        npost0 = npost if npost0 is None else npost0
        nl = len(self.A)
        bs, xs = [np.asarray(b, float)], [None] * nl
        for l in range(nl - 1):
            A, Di, bl = self.A[l], self.dinv[l], bs[l]
            if l == 0 and gs_first is not None:
                c2 = ~gs_first
                x = Di * bl
                x[c2] += Di[c2] * (bl - A @ x)[c2]
                r = bl - A @ x
                r[c2] = 0.0
            else:
                x = omega * Di * bl
                for _ in range(npre - 1):
                    x = x + omega * Di * (bl - A @ x)
                r = bl - A @ x
            xs[l] = x
            bs.append(self.P[l].T @ r)
        A, Di, bl = self.A[-1], self.dinv[-1], bs[-1]
        if self.inv is not None:
            x = self.inv @ bl
        else:
            x = omega * Di * bl
            for _ in range(2 * coarse_sweeps):
                x = x + omega * Di * (bl - A @ x)
        xs[-1] = x
        for l in range(nl - 2, -1, -1):
            A, Di, bl = self.A[l], self.dinv[l], bs[l]
            x = xs[l] + (pdamp0 if l == 0 else pdamp) * (self.P[l] @ xs[l + 1])
            for _ in range(npost0 if l == 0 else npost):
                if l == 0 and gs_first is not None:
                    for c in (~gs_first, gs_first):
                        x[c] += Di[c] * (bl - A @ x)[c]
                else:
                    x = x + omega * Di * (bl - A @ x)
            xs[l] = x
        return xs[0]


def pressure_matrix(rowptr, col, val9, w):
    """A_p(i, j) = sum_eq w_eq(i) J_ij[eq][0]: the pressure column of the (scaled) equations combined with the CPR weights w[3][nb]"""
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    nb = rowptr.size - 1
    rows = np.repeat(np.arange(nb), np.diff(rowptr))
    v = np.asarray(val9, float).reshape(-1, 9)
    ap = w[0][rows] * v[:, 0] + w[1][rows] * v[:, 3] + w[2][rows] * v[:, 6]
    return sp.csr_matrix((ap, (rows, col)), shape=(nb, nb))


def cpr_apply(d3, J, w, Ap, cycle, stage2, cpr_relax=1.0, global_constant=False, nw=0):
    """The two-stage preconditioner on a block-interleaved d3: b = sum_eq w_eq d_eq; (global constant: b -= A_p 1 e with
    e = (1^T A_p 1)^-1 1^T b, and e is added back to the cycle's result); x_p = cycle(b); z = d - J [x_p; 0; 0]; v = stage2(z);
    v_p += cpr_relax x_p.  J: scipy BSR/CSR of the 3x3 system (caller numbering), Ap: level 0 without border rows, cycle: level-0
    vector (nw border rows behind the cells, right-hand side zero there) -> its V-cycle, stage2: z3 -> ILU0^-1 z3 (relaxed as the solve
    relaxes it)."""
    d = np.asarray(d3, float).reshape(-1, 3)
    nb = d.shape[0]
    b = w[0] * d[:, 0] + w[1] * d[:, 1] + w[2] * d[:, 2]
    e = 0.0
    if global_constant:
        one = np.ones(nb)
        e = one @ b / (one @ (Ap @ one))
        b = b - e * (Ap @ one)
    xp = cycle(np.concatenate([b, np.zeros(nw)]))[:nb] + e
    xfull = np.zeros(3 * nb)
    xfull[0::3] = xp
    z = np.asarray(d3, float) - J @ xfull
    v = np.array(stage2(z), float)
    v[0::3] += cpr_relax * xp
    return v


def point_ilu0_apply(A, order, b, relax=1.0):
    """relax (L U)^-1 b with the point ILU0 of the scalar matrix A (its own pattern, no fill), eliminated in `order` (order[i] = the
    position of row i; IKJ: row i's lower entries in increasing position, each L_ik = a_ik / u_kk then row i -= L_ik (row k's upper part))"""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    order = np.asarray(order)
    perm = np.argsort(order)                 # perm[p] = row at position p
    Ap = A[perm][:, perm].tocsr()
    Ap.sort_indices()
    rows = []
    for i in range(n):
        cols = Ap.indices[Ap.indptr[i]:Ap.indptr[i + 1]]
        row = dict(zip(cols.tolist(), Ap.data[Ap.indptr[i]:Ap.indptr[i + 1]].tolist()))
        for k in sorted(c for c in row if c < i):
            L = row[k] / rows[k][k]
            row[k] = L
            for j, u in rows[k].items():
                if j > k and j in row:
                    row[j] -= L * u
        rows.append(row)
    bp = np.asarray(b, float)[perm]
    y = np.zeros(n)
    for i in range(n):
        y[i] = bp[i] - sum(v * y[k] for k, v in rows[i].items() if k < i)
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - sum(v * x[j] for j, v in rows[i].items() if j > i)) / rows[i][i]
    out = np.zeros(n)
    out[perm] = relax * x
    return out
