"""The Newton loop's three device reductions -- opmgpu_convergence (k_conv_partial / k_conv_final over the bpart partials of k_cell_values),
opmgpu_average_b and opmgpu_relative_change (k_relchange_partial / k_sum2_final) -- against their float64 restatement
(tests/reductions_reference.py) at the sizes where each tier of the scheme can go wrong: around one wave (63, 64, 65 cells), one block
(255, 256, 257), several blocks (513), one element past the final kernels' 256-partial stride (65537) and one block past the grid cap
of 2048 (524289).  Columns of cells with non-uniform pore volume, so that the row of max |R| / pv is not the row of max |R|; one
single-perforation host well on every targeted INTERNAL row (first / last lane of a wave, of a block, of a stride trip), through which
opmgpu_add_well_terms plants residuals: a maximum, a known change of the sum, a NaN or an infinity that only that row carries.

Tolerances are the derived bounds of reductions_reference.tolerances: maxima bit for bit, sums within gamma_{n-1} sum |x|."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from opmgpu import capi, decks
from opmgpu.model import GpuBlackoilModel, NumericalIssue

import reductions_reference as ref
import twophase

pytestmark = pytest.mark.gpu

DT = 3 * decks.DAY
DP = 1.0 * decks.BAR                 # the pressure step of the single-row relative change


def _convergence(m):
    """(status, converged, B, CNV, MB, linf) of getConvergence; the numbers are valid whatever the status"""
    try:
        conv, status = m.getConvergence(), capi.OK
    except NumericalIssue:
        conv, status = None, capi.ENUMERICAL
    return SimpleNamespace(status=status, converged=conv, B=m.B_avg.copy(), CNV=m.CNV.copy(), MB=m.MB.copy(), linf=m.linf.copy())


def _same(a, b):
    return a.status == b.status and a.converged == b.converged and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("B", "CNV", "MB", "linf"))


def _open(nc, ordering, oil_water=False):
    """model on the column deck after prepareStep, assemble(True), a second state and assemble(False): accumulation and flux in R"""
    case = ref.column_case(nc, ordering)
    if oil_water:
        tab = twophase.tables(regions=1)
        st1, st2, st3 = (twophase.state(case.grid, seed=s) for s in (11, 21, 31))
    else:
        tab = decks.satfunc_standard_tables()
        st1, st2, st3 = (decks.random_state(case.grid, tab, seed=s) for s in (1, 11, 21))
        st2.hc[:] = st1.hc
    prm = capi.default_params(ilu_ordering=ordering)
    m = GpuBlackoilModel(case.grid, tab, prm, wells=case.wells)
    assert np.array_equal(m.ordering()[0], case.pos)                  # the wells' cells ARE the targeted internal rows
    m.prepareStep(DT, st1)
    m.assemble(True)
    m.setState(st2)
    m.assemble(False)
    return SimpleNamespace(m=m, case=case, prm=prm, nc=nc, st2=st2, st3=st3, oil_water=oil_water, phases=(0, 1) if oil_water else (0, 1, 2))


def _check_scalars(x):
    """check 1: B_avg, CNV, MB, linf, converged, status and averageB against the restatement of the read-back residual"""
    m, nc = x.m, x.nc
    R = m.residual().reshape(3, nc)
    sd = m.simulatorData()
    binv = np.stack([1.0 / sd["1OVERBW"], 1.0 / sd["1OVERBO"], np.ones(nc) if x.oil_water else 1.0 / sd["1OVERBG"]])
    r = ref.convergence_scalars(R, binv, x.case.grid.pv, DT, x.prm)
    t = ref.tolerances(r)
    for a in range(3):          # detectability: one dropped cell moves sum 1/b by far more than its bound
        assert binv[a].min() > ref.DETECTABLE * t.B_rtol * r.sumbinv[a]
    assert np.all(r.sumabsR[list(x.phases)] > 0.0) and np.all(np.abs(r.Rsum[list(x.phases)]) > 0.0)      # the accumulation term is in R
    got = _convergence(m)
    print("nc %d  B err/tol %s  MB err/tol %s  CNV rel err %s" % (nc, np.abs(got.B - r.B) / (t.B_rtol * r.B),
                                                                  np.abs(got.MB - r.MB) / np.maximum(t.MB_atol, 1e-300),
                                                                  np.abs(got.CNV - got.B * DT * r.maxRpv) / np.maximum(got.CNV, 1e-300)))
    assert np.all(np.abs(got.B - r.B) <= t.B_rtol * r.B), (got.B, r.B)
    assert np.array_equal(got.linf, r.linf), (got.linf, r.linf)
    want_cnv = got.B * DT * r.maxRpv
    assert np.all(np.abs(got.CNV - want_cnv) <= t.CNV_rtol * want_cnv), (got.CNV, want_cnv)
    assert np.all(np.abs(got.MB - r.MB) <= t.MB_atol), (got.MB, r.MB, t.MB_atol)
    assert got.status == r.status and (got.converged is None or got.converged == r.converged)
    assert np.array_equal(m.averageB(), got.B)                          # the same kernels on the same data
    if x.oil_water:
        assert got.B[2] == 1.0 and got.linf[2] == 0.0 and got.MB[2] == 0.0 and got.CNV[2] == 0.0        # n ones, summed in any order
    assert _same(_convergence(m), got)                                  # check 6: bitwise repeatable
    return R, r, t, got


def _check_plants(x, R0, r0, t0, got0):
    """checks 2 and 3: per target row and phase, max |R| on that row, max |R| / pv on a lighter target row, and |sum R| moved by what
    was planted"""
    m, case, nc = x.m, x.case, x.nc
    pv = case.grid.pv
    ipv = 1.0 / pv
    others = np.ones(nc, bool)
    others[case.cells] = False
    for a, k, j, delta in ref.plants(case, R0, x.phases):
        m.assemble(False)
        m.addWellTerms(delta, [], [])
        got = _convergence(m)
        Rp = m.residual().reshape(3, nc)
        for b in range(3):
            assert np.array_equal(Rp[b, others], R0[b, others])
            assert np.array_equal(Rp[b, case.cells], R0[b, case.cells] + delta[:, b])
        absR = np.abs(Rp[a])
        assert int(absR.argmax()) == case.cells[k] and (nc == 1 or absR[case.cells[k]] > np.delete(absR, case.cells[k]).max())
        assert int((absR * ipv).argmax()) == case.cells[j] and (j != k or case.cells[k] == case.cells[np.argmin(pv[case.cells])])
        assert np.array_equal(got.linf, np.abs(Rp).max(1)), (a, k, got.linf)
        want_cnv = got.B * DT * (np.abs(Rp) * ipv).max(1)
        assert np.all(np.abs(got.CNV - want_cnv) <= t0.CNV_rtol * want_cnv), (a, k, j, got.CNV, want_cnv)
        assert np.array_equal(got.B, got0.B)
        # |sum R_a| as the device has it, before and after
        after = ref.with_replaced(r0, a, R0[a, case.cells], Rp[a, case.cells])
        planted = after.Rsum[a] - r0.Rsum[a]
        tol = t0.absRsum_atol[a] + ref.tolerances(after).absRsum_atol[a]
        assert abs(planted) > ref.DETECTABLE * tol and planted * r0.Rsum[a] > 0.0
        q0, q1 = (g.MB[a] * r0.pvsum / (g.B[a] * DT) for g in (got0, got))
        assert abs((q1 - q0) - abs(planted)) <= tol, (a, k, j, q1 - q0, planted, tol)
        bad = max(want_cnv.max(), abs(r0.B[a] * after.Rsum[a]) * DT / r0.pvsum) > x.prm.max_residual_allowed
        assert got.status == (capi.ENUMERICAL if bad else capi.OK)
        for b in set(range(3)) - {a}:
            assert got.MB[b] == got0.MB[b] and got.CNV[b] == got0.CNV[b]


def _check_non_finite(x, got0, every_row):
    """check 4: a NaN or an infinity in one row of one phase is a NumericalIssue (a status, not a fault); the next assembly is clean"""
    m, case = x.m, x.case
    K = case.cells.size
    last = int(np.argmax(case.rows))
    for value in ((np.nan, np.inf, -np.inf) if every_row else (np.nan,)):
        for k in (range(K) if every_row else (last,)):
            for a in range(3):
                delta = np.zeros((K, 3))
                delta[k, a] = value
                m.assemble(False)
                m.addWellTerms(delta, [], [])
                with pytest.raises(NumericalIssue):
                    m.getConvergence()
    m.assemble(False)
    again = _convergence(m)
    assert np.isfinite(np.concatenate([again.B, again.CNV, again.MB, again.linf])).all() and _same(again, got0)


def _check_relative_change(x):
    """check 5: one row's pressure raised by DP -- every other term of the numerator is exactly 0 --, then every cell changed, then
    restoreState"""
    m, case, nc, st2 = x.m, x.case, x.nc, x.st2
    rtol = ref.relative_change_rtol(nc)
    assert ref.DETECTABLE * rtol < 1.0
    m.saveState()
    assert m.relativeChange() == 0.0
    _, _, den0 = ref.relative_change(st2, st2)
    for c in case.cells:
        st = st2.copy()
        st.p[c] = st2.p[c] + DP
        d = st2.p[c] - st.p[c]
        den = math.fsum([den0, -st2.p[c] * st2.p[c], st.p[c] * st.p[c]])
        m.setState(st)
        got = m.relativeChange()
        assert abs(got - d * d / den) <= rtol * (d * d / den), (int(c), got, d * d / den)
    if x.oil_water:                                   # (the device keeps Sg = 0 of an oil-water deck: so does this state)
        assert not x.st3.sat[:, 2].any()
    m.setState(x.st3)
    want, num, den = ref.relative_change(st2, x.st3)
    got = m.relativeChange()
    print("nc %d  relative change err/tol %.3g" % (nc, abs(got - want) / (rtol * want)))
    assert num > 0.0 and abs(got - want) <= rtol * want, (got, want)
    assert m.relativeChange() == got                  # check 6
    m.restoreState()
    back = m.getState()
    assert np.array_equal(back.p, st2.p) and np.array_equal(back.sat, st2.sat)
    if not x.oil_water:
        assert np.array_equal(back.rs, st2.rs) and np.array_equal(back.rv, st2.rv) and np.array_equal(back.hc, st2.hc)
    assert m.relativeChange() == 0.0


def _run(nc, ordering, oil_water=False, every_row=True):
    x = _open(nc, ordering, oil_water)
    try:
        R0, r0, t0, got0 = _check_scalars(x)
        _check_plants(x, R0, r0, t0, got0)
        _check_non_finite(x, got0, every_row)
        _check_relative_change(x)
    finally:
        x.m.close()


@pytest.mark.parametrize("ordering", [capi.ORDER_NATURAL, capi.ORDER_MULTICOLOR])
@pytest.mark.parametrize("nc", ref.SMALL_SIZES)
def test_around_one_wave_and_one_block(gpu_lib, nc, ordering):
    """1 cell (no connection at all) to 513 cells (three blocks), rows in the caller's order and in red-black order"""
    _run(nc, ordering)


def test_second_trip_of_the_final_kernels(gpu_lib):
    """65537 cells = 257 partials: k_conv_final and k_sum2_final stride a second time, for one element"""
    _run(ref.SECOND_FINAL_TRIP, capi.default_params().ilu_ordering, every_row=False)


def test_one_block_past_the_grid_cap(gpu_lib):
    """524289 cells = 2049 blocks of cells against kMaxRedBlocks = 2048: one grid-stride second trip of the partial kernels, and 2049
    bpart partials of sum 1/b"""
    _run(ref.PAST_GRID_CAP, capi.default_params().ilu_ordering, every_row=False)


@pytest.mark.parametrize("nc", [257, ref.SECOND_FINAL_TRIP])
def test_oil_water(gpu_lib, nc):
    """no gas phase: k_cell_values adds 1 per cell to the third sum of 1/b, so B_avg[2] is exactly 1 whatever the order"""
    _run(nc, capi.default_params().ilu_ordering, oil_water=True, every_row=nc < 1000)
