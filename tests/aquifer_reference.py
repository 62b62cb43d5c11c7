"""The analytic-aquifer rule (Fetkovich, Carter-Tracy) restated in float64 NumPy from the text of include/opmgpu.h at opmgpu_set_aquifers
-- NOT from the kernels of csrc/aquifer.hip.  Every product and sum is one NumPy operation in the order the header's parentheses give, so
no fused multiply-add can hide in it.  What the rule needs of a cell (p_w, rho_w, b_w and their derivatives) is an INPUT here: the tests
take it from tests/cell_reference.py (cell(), 50 digits) or, to check the aquifer arithmetic alone, from the device's own read-out.

    a = Aquifer(kind, p_a0, datum, CtV0=, J= | beta=, Tc=, td=, pd=, cells=, alpha=)      state: a.We, a.Ws, a.t
    sc = scalars(a, dt)                           per aquifer, begin of a step (raises ValueError for a bad den)
    A, B = coefficients(a, sc, rho0, p0, z, g)    per connection
    q = rates(A, B, pw)                           q_j = A_j - B_j pw_j
    s, d = cell_terms(A, B, bw, pw)               one connected cell: what is subtracted from R_water and (times the scale) from D[water][:]
    Q = tree_sum(q)                               the commit's documented summation tree
    commit(a, dt, q, qs)
"""
import math

import numpy as np

FETKOVICH, CARTER_TRACY = 0, 1
BLOCK, WAVE = 256, 64


class Aquifer:
    def __init__(self, kind, p_a0, datum, CtV0=0.0, J=0.0, beta=0.0, Tc=0.0, td=(), pd=(), cells=(), alpha=()):
        self.kind, self.p_a0, self.datum = int(kind), float(p_a0), float(datum)
        self.CtV0, self.J, self.beta, self.Tc = float(CtV0), float(J), float(beta), float(Tc)
        self.td, self.pd = np.asarray(td, np.float64), np.asarray(pd, np.float64)
        self.cells, self.alpha = np.asarray(cells, np.int64), np.asarray(alpha, np.float64)
        self.We = self.Ws = self.t = 0.0

    def p_a(self):
        """the derived output: p_a0 - W_e / CtV0 (Fetkovich), p_a0 - W_e / beta (Carter-Tracy)"""
        return self.p_a0 - self.We / (self.CtV0 if self.kind == FETKOVICH else self.beta)


def table_segment(td, x):
    """the segment rule of the PVT tables: i = [t_D[1] < x] + sum_{k=2}^{n-2} [t_D[k] <= x] (0 for a table of two rows)"""
    n = len(td)
    i = 1 if (n > 2 and td[1] < x) else 0
    for k in range(2, n - 1):
        i += 1 if td[k] <= x else 0
    return i


def scalars(a, dt):
    """the per-aquifer scalars of a step of length dt from the committed state"""
    dt = np.float64(dt)
    We, t = np.float64(a.We), np.float64(a.t)
    if a.kind == FETKOVICH:
        pa = np.float64(a.p_a0) - We / np.float64(a.CtV0)
        tau = np.float64(a.CtV0) / np.float64(a.J)
        x = dt / tau
        E = np.float64(-math.expm1(-x)) / x
        return dict(E=E, JE=np.float64(a.J) * E, pa=pa, x=x)
    Tc = np.float64(a.Tc)
    tD, tDp = t / Tc, (t + dt) / Tc
    i = table_segment(a.td, tDp)
    Pp = (a.pd[i + 1] - a.pd[i]) / (a.td[i + 1] - a.td[i])
    P = a.pd[i] + Pp * (tDp - a.td[i])
    den = P - tD * Pp
    if not (den > 0.0 and np.isfinite(den)):
        raise ValueError("den = P - t_D P' = %r is not positive and finite" % float(den))
    Tden = Tc * den
    return dict(tD=tD, tDp=tDp, seg=i, Pp=Pp, P=P, den=den, Tden=Tden, b=np.float64(a.beta) / Tden)


def coefficients(a, sc, rho0, p0, z, gravity):
    """(A_j, B_j) of the aquifer's connections from their cells' frozen water density rho0 and water pressure p0 and the cell depths z"""
    rho0, p0, z = (np.asarray(v, np.float64) for v in (rho0, p0, z))
    h = (rho0 * np.float64(gravity)) * (z - np.float64(a.datum))
    if a.kind == FETKOVICH:
        B = a.alpha * sc["JE"]
        A = B * (sc["pa"] + h)
        return A, B
    aj = (np.float64(a.beta) * ((np.float64(a.p_a0) + h) - p0) - np.float64(a.We) * sc["Pp"]) / sc["Tden"]
    B = a.alpha * sc["b"]
    A = a.alpha * (aj + sc["b"] * p0)
    return A, B


def rates(A, B, pw):
    return np.asarray(A, np.float64) - np.asarray(B, np.float64) * np.asarray(pw, np.float64)


def cell_terms(A, B, bw, pw):
    """One connected cell with the connections (A[k], B[k]) in the listing order; bw, pw: [4] = value, d/dp, d/dSw, d/dX of the cell's b_w
    and p_w (d p_w / d v is taken as (1, pw[2], 0), as the rule says).  Returns (s, d[3]): R_water -= s, D[water][v] -= scale_water d[v]."""
    bw, pw = np.asarray(bw, np.float64), np.asarray(pw, np.float64)
    s, d = np.float64(0.0), np.zeros(3)
    for Aj, Bj in zip(np.asarray(A, np.float64), np.asarray(B, np.float64)):
        q = Aj - Bj * pw[0]
        bB = bw[0] * Bj
        s = s + bw[0] * q
        d[0] = d[0] + (bw[1] * q - bB)
        d[1] = d[1] + (bw[2] * q - bB * pw[2])
        d[2] = d[2] + bw[3] * q
    return s, d


def tree_sum(v):
    """the commit's tree: slot T sums v[T], v[T + 256], ... in ascending order from 0.0; each wave of 64 slots is folded with the offsets
    32, 16, 8, 4, 2, 1; the four wave sums are added in order"""
    v = np.asarray(v, np.float64)
    slots = np.zeros(BLOCK)
    for k0 in range(0, v.size, BLOCK):
        part = v[k0:k0 + BLOCK]
        slots[:part.size] = slots[:part.size] + part
    waves = []
    for w in range(BLOCK // WAVE):
        x = slots[w * WAVE:(w + 1) * WAVE].copy()
        off = WAVE // 2
        while off >= 1:
            x[:off] = x[:off] + x[off:2 * off]
            off //= 2
        waves.append(x[0])
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def commit(a, dt, q, qs):
    """W_e += dt Q, W_s += dt Qs, t += dt with Q, Qs by the tree; returns (Q, Qs)"""
    dt = np.float64(dt)
    Q, Qs = tree_sum(q), tree_sum(qs)
    a.We = float(np.float64(a.We) + dt * Q)
    a.Ws = float(np.float64(a.Ws) + dt * Qs)
    a.t = float(np.float64(a.t) + dt)
    return Q, Qs


def tank_step(a, dt, pw, bw=1.0, rho0=0.0, z=0.0, gravity=0.0):
    """one committed step of an aquifer against cells held at the water pressure pw (a scalar or one value per connection): the whole rule
    with the cell evaluator replaced by constants"""
    n = a.alpha.size
    pw = np.broadcast_to(np.asarray(pw, np.float64), (n,))
    sc = scalars(a, dt)
    A, B = coefficients(a, sc, np.broadcast_to(np.float64(rho0), (n,)), pw, np.broadcast_to(np.float64(z), (n,)), gravity)
    q = rates(A, B, pw)
    commit(a, dt, q, np.float64(bw) * q)
    return sc, A, B, q
