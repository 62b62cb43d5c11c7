"""Float64 restatements of the Newton loop's three cell-side reductions, host only: getConvergence with its convergenceReduction
(BlackoilModelBase_impl.hpp:1633-1857) and relativeChange (:1595-1631), written from the reference and not from the kernels.  Every sum
is math.fsum -- the exactly rounded sum of its terms --, so a device sum taken in ANY order differs from it by at most the textbook bound
gamma_{n-1} * sum |x_i| and nothing here has to be tuned: `tolerances` and `relative_change_rtol` state the bounds the device tests use.

Below the restatements: the column decks of tests/test_gpu_reductions.py and the internal rows they aim at, shared with the host test
(tests/test_reductions_reference.py) that checks the conditioning of those decks before a device ever sees them."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

from opmgpu import capi, decks

U = 2.0 ** -53                       # unit roundoff of float64
SCALAR = 8 * U                       # the few scalar roundings behind a sum: divisions, products, the test's own arithmetic
DETECTABLE = 1000.0                  # a planted change must exceed this many tolerances of the quantity it is meant to move


def gamma(k):
    """gamma_k = k u / (1 - k u): |fl-sum in any order - exact sum| <= gamma_{n-1} sum |x_i| for n terms (Higham, Accuracy and Stability
    of Numerical Algorithms, eq. 4.4)"""
    k = max(int(k), 0)
    return k * U / (1.0 - k * U)


def _fsum(x):
    x = np.asarray(x, np.float64).ravel()
    if not np.isfinite(x).all():
        with np.errstate(invalid="ignore"):
            return float(x.sum())            # NaN / Inf arithmetic: what any floating-point sum of these terms gives
    return math.fsum(x.tolist())


def convergence_scalars(R, binv, pv, dt, prm):
    """getConvergence for the reservoir equations.  R [3, nc] residual, binv [3, nc] = 1 / b, pv [nc], prm the opmgpu_params.
    B = sum(1/b) / nc (:1699), Rsum = sum R (:1701), maxRpv = max |R| / pv (:1751, :1700 -- as |R| * (1 / pv), the device's form of the
    same quotient), linf = max |R| (computeResidualNorms, :1551-1589), CNV = B dt maxRpv (:1768), MB = |B Rsum| dt / sum(pv) (:1769),
    converged (:1770-1771), status ENUMERICAL for a non-finite residual (:1562-1566), a NaN MB / CNV (:1828-1836) or one above
    max_residual_allowed (:1837-1845).  sumabsR, sumbinv, pvsum: what the error bounds of `tolerances` are made of."""
    R = np.asarray(R, np.float64).reshape(3, -1)
    binv = np.asarray(binv, np.float64).reshape(3, -1)
    pv = np.asarray(pv, np.float64)
    nc = R.shape[1]
    assert binv.shape == (3, nc) and pv.shape == (nc,)
    ipv = 1.0 / pv
    out = SimpleNamespace(nc=nc, dt=float(dt))
    out.sumbinv = np.array([_fsum(binv[a]) for a in range(3)])
    out.B = out.sumbinv / nc
    out.Rsum = np.array([_fsum(R[a]) for a in range(3)])
    out.sumabsR = np.array([_fsum(np.abs(R[a])) for a in range(3)])
    out.pvsum = _fsum(pv)
    with np.errstate(invalid="ignore", over="ignore"):
        out.maxRpv = np.array([(np.abs(R[a]) * ipv).max() for a in range(3)])
        out.argmaxRpv = np.array([int(np.argmax(np.abs(R[a]) * ipv)) for a in range(3)])
        out.linf = np.array([np.abs(R[a]).max() for a in range(3)])
        out.CNV = out.B * dt * out.maxRpv
        out.MB = np.abs(out.B * out.Rsum) * dt / out.pvsum
        out.converged = bool(np.all(out.MB < prm.tolerance_mb) and np.all(out.CNV < prm.tolerance_cnv))
        bad = (not np.isfinite(R).all()) or np.isnan(out.MB).any() or np.isnan(out.CNV).any()
        bad = bad or bool((out.MB > prm.max_residual_allowed).any() or (out.CNV > prm.max_residual_allowed).any())
    out.status = capi.ENUMERICAL if bad else capi.OK
    return out


def with_replaced(ref, a, old, new):
    """The sums of `ref` after the residual entries `old` of phase a became `new` (a handful of rows): the two sums the error bounds are
    made of are updated by the differences -- a few roundings on numbers that only scale a bound -- instead of summing a large deck again
    for every planted row.  Maxima and derived scalars are not carried over."""
    old, new = np.asarray(old, np.float64), np.asarray(new, np.float64)
    out = SimpleNamespace(nc=ref.nc, dt=ref.dt, B=ref.B, pvsum=ref.pvsum, Rsum=ref.Rsum.copy(), sumabsR=ref.sumabsR.copy())
    out.Rsum[a] = math.fsum([ref.Rsum[a]] + new.tolist() + (-old).tolist())
    out.sumabsR[a] = math.fsum([ref.sumabsR[a]] + np.abs(new).tolist() + (-np.abs(old)).tolist())
    return out


def tolerances(ref):
    """Error bounds of a device evaluation of convergence_scalars' quantities that sums in any order (u, gamma_k above; n = nc):
      sum 1/b : positive terms, so |dev - fsum| <= gamma_{n-1} fsum;  B = sum / nc adds one division  ->  B_rtol = gamma_{n-1} + 8u
      sum R   : |dev - fsum| <= gamma_{n-1} sum |R|                                                   ->  Rsum_atol
      sum pv  : positive terms, gamma_{n-1} relative (the device's own pore-volume sum is a plain loop)
      MB = |B Rsum| dt / pvsum: with B (1 + eb), Rsum + es, pvsum (1 + ep) and three roundings of its own,
            |MB_dev - MB| <= (B dt / pvsum) (Rsum_atol + (|Rsum| + Rsum_atol) (2 gamma_{n-1} + 8u))   ->  MB_atol
            (second-order terms are below gamma^2 = 4e-21 at n = 524289: inside the slack between the <= 5 roundings and 8u)
      |Rsum| read back out of the device's numbers as MB pvsum / (B dt): B cancels, pvsum's error and seven roundings stay
            |q - |Rsum|| <= Rsum_atol + (|Rsum| + Rsum_atol) (gamma_{n-1} + 8u)                       ->  absRsum_atol
    CNV = B dt max is compared with the DEVICE's B (CNV_rtol = 8u); the maxima themselves are exact."""
    g = gamma(ref.nc - 1)
    t = SimpleNamespace()
    t.B_rtol = g + SCALAR
    t.Rsum_atol = g * ref.sumabsR
    t.MB_atol = (ref.B * ref.dt / ref.pvsum) * (t.Rsum_atol + (np.abs(ref.Rsum) + t.Rsum_atol) * (2 * g + SCALAR))
    t.absRsum_atol = t.Rsum_atol + (np.abs(ref.Rsum) + t.Rsum_atol) * (g + SCALAR)
    t.CNV_rtol = SCALAR
    return t


def relative_change(prev, cur):
    """relativeChange(previous, current) (:1595-1631): (|p0 - p|^2 + |s0 - s|^2) / (|p|^2 + |s|^2) over all cells and phases, 0 when the
    new norm is 0.  Returns (value, numerator, denominator)."""
    dp = np.asarray(prev.p, np.float64) - np.asarray(cur.p, np.float64)
    ds = np.asarray(prev.sat, np.float64) - np.asarray(cur.sat, np.float64)
    num = _fsum(np.concatenate([dp * dp, (ds * ds).ravel()]))
    den = _fsum(np.concatenate([np.asarray(cur.p, np.float64) ** 2, (np.asarray(cur.sat, np.float64) ** 2).ravel()]))
    return (num / den if den > 0.0 else 0.0), num, den


def relative_change_rtol(nc):
    """Both sums have non-negative terms, one per cell on the device (four squares added up: <= 4 roundings, against one per square
    here): each is within gamma_{n-1} + 8u of its fsum, relatively; the quotient adds one rounding (inside the second 8u)."""
    return 2.0 * (gamma(nc - 1) + SCALAR) + SCALAR


# ------------------------------------------------------------------------------------------------------------------------------------------
# the column decks of the device tests
# ------------------------------------------------------------------------------------------------------------------------------------------
BLOCK, FINAL_STRIDE, MAX_BLOCKS = 256, 256, 2048         # csrc/common.hpp: kBlock, the final kernels' stride, kMaxRedBlocks
SMALL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513)
SECOND_FINAL_TRIP = BLOCK * FINAL_STRIDE + 1              # 65537 cells: 257 partials, one element for the final kernels' second trip
PAST_GRID_CAP = BLOCK * MAX_BLOCKS + 1                    # 524289 cells: 2049 blocks of cells against 2048 launched
EXTRA_ROWS = {SECOND_FINAL_TRIP: (65535, 65536), PAST_GRID_CAP: (262144, 524287, 524288)}


def target_rows(nc):
    """internal rows at the edges of a wave, a block, the final kernels' stride and the grid-stride loop"""
    rows = [0, 63, 64, 255, 256, nc - 1] + list(EXTRA_ROWS.get(nc, ()))
    return np.array(sorted({r for r in rows if 0 <= r < nc}), np.int64)


def column_pattern(nc):
    """BSR pattern of an nc x 1 x 1 column: every cell and its one or two neighbours"""
    i = np.arange(nc, dtype=np.int64)
    cols = np.stack([i - 1, i, i + 1], 1)
    keep = (cols >= 0) & (cols < nc)
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int32)
    return rowptr, cols[keep].astype(np.int32)


def plan_rows(nc, ordering):
    """cell_of_row [nc] for the column's pattern through the library's host-only planner (opmgpu_plan_ordering reports perm[cell] = row,
    include/opmgpu.h; single-perforation wells add no fill, so a model with them has the same rows -- the device test asserts it)"""
    rowptr, col = column_pattern(nc)
    pos, lev = np.zeros(nc, np.int32), np.zeros(nc, np.int32)
    nl = C.c_int32(0)
    st = capi.load().opmgpu_plan_ordering(nc, capi.iptr(rowptr), capi.iptr(col), int(ordering), capi.iptr(pos), capi.iptr(lev), C.byref(nl))
    assert st == capi.OK, st
    cell_of_row = np.empty(nc, np.int64)
    cell_of_row[pos] = np.arange(nc)
    return cell_of_row, pos


def column_case(nc, ordering, seed=0):
    """The deck of one device test: decks.cartesian_grid(nc, 1, 1, lognormal_sigma=0.5) with every pore volume multiplied by a random
    factor in [0.5, 2]; the target rows' factors are distinct, a ratio 4^(1/K) apart inside the same range and in random order, so that
    for every target but the lightest a LIGHTER target exists (plants()).  Returns grid, the target rows, their cells, (connpos, cells) of
    one single-perforation well per target, and the planner's perm."""
    base = decks.cartesian_grid(nc, 1, 1, lognormal_sigma=0.5)
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    factor = 0.5 * 4.0 ** rng.random(nc)
    cell_of_row, pos = plan_rows(nc, ordering)
    rows = target_rows(nc)
    cells = cell_of_row[rows]
    K = rows.size
    factor[cells] = 0.5 * 4.0 ** ((rng.permutation(K) + 0.5) / K)
    grid = decks.GridData(nc, base.conn_cells, base.trans, base.pv * factor, base.z, gravity=base.gravity, dims=base.dims)
    wells = (np.arange(K + 1, dtype=np.int32), cells.astype(np.int32))
    return SimpleNamespace(grid=grid, rows=rows, cells=cells, wells=wells, pos=pos)


def plants(case, R, phases=(0, 1, 2)):
    """For every target row and phase one planted pair, as (phase, k, j, delta [K, 3]) with delta in the wells' perforation order:
    the residual of target k is raised to M, the strict maximum of |R_a| (16 times the largest quotient |R_a| / pv of the deck, times
    the largest pore volume: no untouched row comes near it by either measure), and -- where a lighter target exists -- the residual of the next lighter target j to about
    M sqrt(pv_j / pv_k) < M, whose quotient by ITS pore volume is the larger one: max |R| sits on row k, max |R| / pv on row j.  The
    lightest target has no such partner (j = k: both maxima on it).  Both additions carry the sign of sum R_a, so |sum R_a| moves by
    exactly their sum."""
    R = np.asarray(R).reshape(3, -1)
    pv = case.grid.pv
    order = np.argsort(pv[case.cells])                      # targets, lightest first
    out = []
    for a in phases:
        sign = -1.0 if math.fsum(R[a].tolist()) < 0.0 else 1.0
        M = 16.0 * float((np.abs(R[a]) / pv).max()) * float(pv.max())
        for q, k in enumerate(order):
            delta = np.zeros((case.cells.size, 3))
            delta[k, a] = sign * M - R[a, case.cells[k]]
            j = k
            if q > 0:
                j = order[q - 1]
                delta[j, a] = sign * M * math.sqrt(pv[case.cells[j]] / pv[case.cells[k]]) - R[a, case.cells[j]]
            out.append((a, int(k), int(j), delta))
    return out
