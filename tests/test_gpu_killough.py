"""GPU: Killough's relative-permeability hysteresis (opmgpu_set_hysteresis_model; the rule is stated in include/opmgpu.h) -- the history
kernel's scanning parameters and the evaluator's scanning curves against the numpy restatement tests/killough_reference.py, the assembly
against the UNCHANGED oracle on the twin deck (Carlson with zero shift on one twin imbibition region per cell), the table paths, the
contexts that must agree bit for bit, the refusals, and the golden deck from the reader to the restart file.

Two twins: without end-point scaling the twin TABLE carries the affine form (abscissae (x - A0) / m, ordinates R y); with imbibition end
points and SCALECRS the twin END POINTS carry it ((s_j - A0) / m) and the twin table only the ordinates R y.  With vertical scaling
neither is enough -- the oracle multiplies a curve by (cell maximum / table maximum) and the maximum is a node of the curve, so a factor R
on the ordinates cancels -- and no twin was built for it: that case pins krg and kro through the output record and
their DERIVATIVES through the perforation properties against the numpy rule."""
import os

import numpy as np
import pytest

import killough_cases as kc
import killough_reference as kref
import test_gpu_assembly_shapes as shapes
from opmgpu import capi, decks, eclio
from opmgpu.model import GpuBlackoilModel
from util import rel_err, slot_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = os.path.join(ROOT, "tests", "golden", "decks", "KILLOUGH_SMALL.DATA")
RTOL_JAC = 1e-11          # tests/test_gpu_assembly.py: Jacobian blocks / residual in f64
DT = 2 * decks.DAY
SEEDS = (1, 3)            # the numpy rule alone finds >= 30 % of the cells scanning and >= 5 % each on drainage and in a guard, per system
EPS = np.finfo(float).eps


def _model(grid, tab, model=capi.HYST_KILLOUGH, a=kc.A, **prm):
    m = GpuBlackoilModel(grid, tab, capi.default_params(**prm))
    if model is not None:
        m.setHysteresisModel(model, a)
    return m


_REF = {}


def _reference(case):
    """per seed of a case: the history the states leave (running minima, as the device forms them) and the numpy rule's planes at it;
    computed once and shared, read-only"""
    if case not in _REF:
        tab, grid = kc.tables(), kc.grid_of(case)
        out, mow, mgo = [], None, None
        for seed in SEEDS:
            mow, mgo = kc.history_of(kc.history_state(grid, tab, seed), mow, mgo)
            planes = kref.scanning_planes(tab, grid, mow, mgo, kc.A)
            for a in list(planes.values()) + [mow, mgo]:
                a.setflags(write=False)
            out.append((mow, mgo, planes))
        _REF[case] = (tab, grid, out)
    return _REF[case]


@pytest.mark.parametrize("case", kc.CASES)
def test_scanning_parameters_follow_the_rule(gpu_lib, case):
    """after updateHysteresis on random states: Sncrt, m, R of both systems against the numpy rule at rtol 1e-13 / atol 1e-15 (the Carlson
    shifts' tolerance in tests/test_gpu_assembly.py) in the cells with Shy - Sncrd >= 0.02 -- m divides by Shy - Sncrt, which amplifies
    rounding as Shy -> Sncrd --, exact zeros of m and R in the guard cells, m = R = 1 without a history"""
    tab, grid, ref = _reference(case)
    m = _model(grid, tab)
    for seed, (mow, mgo, pl) in zip(SEEDS, ref):
        m.prepareStep(DT, kc.history_state(grid, tab, seed))
        m.updateHysteresis()
        h = m.getHysteresis()
        assert np.array_equal(h[0], mow) and np.array_equal(h[1], mgo)
        got = dict(zip(("sncrt_ow", "m_ow", "r_ow", "sncrt_go", "m_go", "r_go"), m.getHysteresisScanning()))
        new = decks.random_state(grid, tab, seed=10 + seed)
        frac = kc.branch_fractions(tab, grid, mow, mgo, new)
        for s, mdc, d in (("ow", mow, h[2]), ("go", mgo, h[3])):
            guard, hist = pl["guard_" + s], mdc < 2.0
            ok = hist & ~guard & (pl["shy_" + s] - pl["sncrd_" + s] >= 0.02)
            for k in ("sncrt_", "m_", "r_"):
                a, b = got[k + s][ok], pl[k + s][ok]
                print("%s seed %d %s: %d cells, max rel err %.3e, m up to %.1f" % (case, seed, k + s, ok.sum(), (np.abs(a - b) / np.abs(b)).max(), pl["m_" + s][ok].max()))
            for k in ("sncrt_", "m_", "r_"):
                assert np.allclose(got[k + s][ok], pl[k + s][ok], rtol=1e-13, atol=1e-15), (case, seed, k + s)
            assert guard.any() and np.all(got["m_" + s][guard] == 0.0) and np.all(got["r_" + s][guard] == 0.0)
            assert np.all(got["m_" + s][~hist] == 1.0) and np.all(got["r_" + s][~hist] == 1.0) and np.all(got["sncrt_" + s][~hist] == 0.0)
            # the shift planes hold the offsets of the affine form (the device's own m and Sncrt through the header's two formulas)
            t, mm, sncri = got["sncrt_" + s], got["m_" + s], pl["sncri_" + s]
            want = (1.0 - sncri - mm * (1.0 - t)) if s == "ow" else (mm * t - sncri)
            assert np.all(np.abs(d - want)[hist] <= 8 * EPS * (1.0 + np.abs(mm[hist]))) and np.all(d[~hist] == 0.0)
            scan, drain, grd = frac[s]
            assert scan >= 0.30 and drain >= 0.05 and grd >= 0.05, (case, seed, s, frac[s])
        assert (pl["sncrt_go"] > pl["sncrd_go"]).mean() > 0.2 and (pl["sncrt_ow"] > pl["sncrd_ow"]).mean() > 0.2
    m.close()


@pytest.mark.parametrize("case", kc.CASES)
def test_kr_of_the_output_record_is_the_rule(gpu_lib, case):
    """krg and kro of a NEW state at the frozen history, through the output record, against the numpy rule to 1e-12 in every cell.
    The bound: m = (Snmax - Sncri) / (Shy - Sncrt) carries a relative rounding of k eps Shy / (Shy - Sncrt) on either side (k ~ 8: the
    operations behind Sncrt), and the two sides form the curve's argument differently (A0 + m S against Sncri + m (S - Sncrt)); on the
    scanning side S - Sncrt <= Shy - Sncrt, so the arguments differ by <= k eps Shy m, and kr = R krni(.) by that times R krni'.  Where m
    is large R is small -- R m = (kd / ki) (Snmax - Sncri) / (Shy - Sncrt) is bounded by the curves, its largest value is taken from the
    numpy planes below -- so the error is <= 2 k eps max(R m) max(krni'), which the test asserts to lie below 1e-12."""
    tab, grid, ref = _reference(case)
    mow, mgo, pl = ref[0]
    slope = max(np.abs(np.diff(tab.sgof_krg[tab.sgof_ptr[1]:tab.sgof_ptr[2]]) / np.diff(tab.sgof_sg[tab.sgof_ptr[1]:tab.sgof_ptr[2]])).max(),
                np.abs(np.diff(tab.swof_krow[tab.swof_ptr[1]:tab.swof_ptr[2]]) / np.diff(tab.swof_sw[tab.swof_ptr[1]:tab.swof_ptr[2]])).max())
    rm = max((pl["r_ow"] * pl["m_ow"]).max(), (pl["r_go"] * pl["m_go"]).max())
    print("%s: max R m %.2f, max imbibition slope %.2f (times the scaling's, <= 2): derived bound %.2e" % (case, rm, slope, 16 * EPS * rm * 2 * slope))
    assert 16 * EPS * rm * 2 * slope <= 1e-12
    m = _model(grid, tab)
    m.prepareStep(DT, kc.history_state(grid, tab, SEEDS[0]))
    m.setHysteresis(mow, mgo)
    for seed in (11, 12):
        st = decks.random_state(grid, tab, seed=seed)
        m.prepareStep(DT, st)
        sd = m.simulatorData()
        want = np.array([kref.kr_cell(tab, grid, c, mow[c], mgo[c], kc.A, st.sat[c, 0], st.sat[c, 2]) for c in range(grid.nc)])
        e_g, e_o = np.abs(sd["GASKR"] - want[:, 0]).max(), np.abs(sd["OILKR"] - want[:, 1]).max()
        print("%s seed %d: max |krg - rule| %.3e, max |kro - rule| %.3e" % (case, seed, e_g, e_o))
        assert np.abs(sd["GASKR"] - want[:, 0]).max() <= 1e-12 and np.abs(sd["OILKR"] - want[:, 1]).max() <= 1e-12
    m.setHysteresisModel(capi.HYST_CARLSON)                # the model matters: Carlson's curves at the same history differ
    sd = m.simulatorData()
    assert np.abs(sd["GASKR"] - want[:, 0]).max() > 1e-3 and np.abs(sd["OILKR"] - want[:, 1]).max() > 1e-3
    m.close()


@pytest.mark.parametrize("case", ["hysteresis", "scaled"])
def test_assembly_against_the_unchanged_oracle_on_the_twin(gpu_lib, oracle, case):
    """hysteresis alone, and with imbibition end points + SCALECRS: residual and Jacobian of a NEW state at the frozen history against the oracle on the twin deck, at
    tests/test_gpu_assembly.py's RTOL_JAC plus the twin's own rounding.  The twin's abscissae (x - A0) / m are O(1) numbers with ~2
    roundings each; the oracle forms a segment's slope from their difference, (x1 - x0) / m >= dx_min / m_max, so a slope -- a Jacobian
    entry's d kr / d S -- carries up to 4 eps m_max / dx_min relative error, m_max over the cells the state finds on the non-zero part of a
    scanning curve (below it the twin's ordinates are both zero: the slope is exactly 0).  Values carry 4 eps times the slope: far less.
    The scaled twin's fixed points (s_j - A0) / m behave alike: a map slope (u1 - u0) / (s1' - s0') carries 4 eps m / ds, ds the smallest
    distance of the cell's imbibition fixed points."""
    tab, grid, ref = _reference(case)
    mow, mgo, pl = ref[0]
    m = _model(grid, tab)
    m.prepareStep(DT, kc.history_state(grid, tab, SEEDS[0]))
    m.updateHysteresis()
    twin_tab, twin_grid = (kc.twin_deck if case == "hysteresis" else kc.twin_deck_scaled)(tab, grid, mow, mgo)
    dx_min = min(np.diff(tab.swof_sw[tab.swof_ptr[1]:tab.swof_ptr[2]]).min(), np.diff(tab.sgof_sg[tab.sgof_ptr[1]:tab.sgof_ptr[2]]).min())
    swco = tab.swof_sw[0] if grid.eps is None else grid.eps[0]
    if case == "scaled":
        sys_ = [kref.cell_systems(tab, grid, c) for c in range(grid.nc)]
        dx_min = min(np.diff(sy[s].table_i.s_pts).min() for sy in sys_ for s in ("ow", "go"))
        assert dx_min > 0.02

    def m_in_play(st):
        """the largest m among the cells st finds on the non-zero part of a scanning curve (numpy rule): only their slopes are the twin's"""
        sn_ow = 1.0 - (st.sat[:, 2] + np.maximum(st.sat[:, 0], swco))
        out = 1.0
        for s, mdc, sn in (("ow", mow, sn_ow), ("go", mgo, st.sat[:, 2])):
            on = (mdc < 2.0) & (1.0 - sn > mdc) & (sn > pl["sncrt_" + s]) & (pl["m_" + s] > 0.0)
            out = max(out, pl["m_" + s][on].max())
        return out
    hist = oracle.Hysteresis(grid.nc)
    hist.mdc_ow[:], hist.mdc_go[:] = mow, mgo                     # the shifts stay zero
    oracle.set_hysteresis(hist)
    try:
        rowptr, col = oracle.pattern(twin_grid)
        scale = tuple(capi.default_params().matbalscale)
        for seed in (11, 12):
            st = decks.random_state(grid, tab, seed=seed)
            twin_rounding = 4 * EPS * m_in_play(st) / dx_min
            assert twin_rounding < RTOL_JAC
            m.prepareStep(DT, st)
            m.assemble(True)
            r0, v0, _, _ = oracle.assemble(twin_grid, twin_tab, DT, st, rowptr, col, scale=scale)
            v, r = m.jacobian()[2], m.residual()
            print(case + " seed %d: residual %.3e, Jacobian %.3e / by slot %.3e (twin rounding %.2e)" % (seed, rel_err(r, r0), rel_err(v, v0), slot_err(v, v0), twin_rounding))
            assert rel_err(r, r0) < RTOL_JAC + twin_rounding
            assert rel_err(v, v0) < RTOL_JAC + twin_rounding and slot_err(v, v0) < RTOL_JAC + twin_rounding
        # Killough matters: the oracle's Carlson on the deck itself assembles another matrix
        hc = oracle.Hysteresis(grid.nc)
        oracle.set_hysteresis(hc)
        hc.update(grid, tab, kc.history_state(grid, tab, SEEDS[0]).sat)
        _, v_c, _, _ = oracle.assemble(grid, tab, DT, st, rowptr, col, scale=scale)
        assert rel_err(v_c, v0) > 1e-4
    finally:
        oracle.set_hysteresis(None)
    m.close()


def test_kr_derivatives_under_vertical_scaling_are_the_rule(gpu_lib):
    """imbibition end points + SCALECRS + vertical scaling, for which no twin was built: the evaluator's DERIVATIVES of kro and krg -- R m
    (vertical factor) (slope of the 2- or 3-point map) (table slope), formed by the same eval_cell the assembly instantiates -- through the
    perforation properties (every cell a perforation: mob and its d/dSw, d/dXvar) against central differences of the numpy rule.
    mob_o = kro / mu_o with mu_o(p_o, rs) free of the saturations: d kro = mu_o d mob_o.  mu_g moves with Sg through p_g = p_o + pcgo(Sg):
    d krg / d Sg = mu_g d mob_g + mob_g d mu_g, d mu_g / d Sg from central differences of the device's own GAS_VISC (values, not the
    derivative under test).  Cells where the one-sided differences of the rule disagree (a kink of a piecewise-linear curve within h) are
    left out; at least 80 % remain.  The bound: a central difference of O(1) values with step h carries 2 eps / h rounding per value;
    the rule's curves are linear between kinks and kro's blend of them has third derivatives of O(10), h^2 of that is far less:
    16 eps / h (1 + |d|) = 3.6e-8 (1 + |d|) at h = 1e-7.  A wrong factor would show at O(0.1 - 10)."""
    tab, grid, ref = _reference("all")
    mow, mgo, pl = ref[0]
    nc, h = grid.nc, 1e-7
    m = _model(grid, tab)
    m.setWells([0, nc], np.arange(nc))                     # one well, every cell a perforation, perforation i = cell i
    st = decks.random_state(grid, tab, seed=11)
    st.sat[:, 0] = np.clip(st.sat[:, 0], 0.02, 0.98)       # (room for the differences)
    both = (st.hc == capi.HC_GAS_AND_OIL) & (st.sat[:, 2] > 2 * h) & (st.sat[:, 1] > 2 * h)
    st.sat[:, 1] = 1.0 - st.sat[:, 0] - st.sat[:, 2]
    m.prepareStep(DT, st)
    m.setHysteresis(mow, mgo)
    sd, pp = m.simulatorData(), m.perfProps(nc)

    def gas_visc(dsg):
        s2 = st.copy()
        s2.sat[:, 2] += dsg; s2.sat[:, 1] -= dsg
        m.setState(s2)
        return m.simulatorData()["GAS_VISC"]
    dmu_g = (gas_visc(h) - gas_visc(-h)) / (2 * h)
    m.close()
    mu_o, mu_g = sd["OIL_VISC"], sd["GAS_VISC"]
    dev_o_w, dev_o_g = pp[:, 30] * mu_o, pp[:, 31] * mu_o
    dev_g_g = pp[:, 35] * mu_g + pp[:, 32] * dmu_g

    def rule(c, dsw, dsg):
        return np.array(kref.kr_cell(tab, grid, c, mow[c], mgo[c], kc.A, st.sat[c, 0] + dsw, st.sat[c, 2] + dsg))
    used = {"kro/sw": 0, "kro/sg": 0, "krg/sg": 0}
    worst = dict.fromkeys(used, 0.0)
    scanning = 0
    for c in np.flatnonzero(both):
        k0 = rule(c, 0.0, 0.0)
        for name, (dsw, dsg), dev, col in (("kro/sw", (h, 0.0), dev_o_w[c], 1), ("kro/sg", (0.0, h), dev_o_g[c], 1), ("krg/sg", (0.0, h), dev_g_g[c], 0)):
            fwd, bwd = (rule(c, dsw, dsg)[col] - k0[col]) / h, (k0[col] - rule(c, -dsw, -dsg)[col]) / h
            if abs(fwd - bwd) > 1e-6 * (1.0 + abs(fwd)):
                continue                                   # a kink within h
            d = 0.5 * (fwd + bwd)
            used[name] += 1
            worst[name] = max(worst[name], abs(dev - d) / (1.0 + abs(d)))
            assert abs(dev - d) <= 16 * EPS / h * (1.0 + abs(d)), (name, c, dev, d)
        scanning += (1.0 - st.sat[c, 2] > mgo[c]) and st.sat[c, 2] > pl["sncrt_go"][c] and pl["m_go"][c] > 0.0
    print("derivatives against the rule, worst |dev - d| / (1 + |d|):", worst, "cells used:", used, "of", both.sum(), "; on a gas scanning curve:", scanning)
    assert min(used.values()) >= 0.8 * both.sum() and both.sum() > 60 and scanning > 10


def _shape_run(large, precision, model=capi.HYST_KILLOUGH):
    """tests/test_gpu_assembly_shapes.py's hysteresis deck, states and histories through one shape with Killough's model"""
    grid, tab = shapes._deck("hysteresis", large)
    m = _model(grid, tab, model, preconditioner_single=int(precision == "mixed"), linear_solver_reduction=1e-10, linear_solver_maxiter=400)
    out = []
    for seed, st in zip(shapes.SEEDS, shapes._states("hysteresis")):
        m.prepareStep(shapes.DT, st)
        m.setHysteresis(*shapes._history(grid.nc, seed))
        m.assemble(True)
        out.append((m.residual(), m.jacobian()[2], np.stack([v for _, v in sorted(m.simulatorData().items())]), np.stack(m.getHysteresisScanning())))
    m.close()
    return out


def test_killough_through_the_blob_path_and_mixed_precision(gpu_lib):
    """tables read from the blob, the float copy written alongside, against (LDS, double): the same system at RTOL_JAC, the scanning
    planes bit for bit (the history kernel reads the same tables whatever the region numbers)"""
    base = _shape_run(False, "double")
    for (r0, v0, rec0, sc0), (r, v, rec, sc) in zip(base, _shape_run(True, "mixed")):
        e_r, e_v, e_rec = rel_err(r, r0), rel_err(v, v0), max(rel_err(a, b) for a, b in zip(rec, rec0))
        print("blob + mixed against LDS + double: residual %.3e Jacobian %.3e output record %.3e" % (e_r, e_v, e_rec))
        assert e_r < RTOL_JAC and e_v < RTOL_JAC and e_rec < RTOL_JAC
        assert np.array_equal(sc, sc0)
    carlson = _shape_run(False, "double", model=None)
    assert rel_err(carlson[0][1], base[0][1]) > 1e-4 and np.all(carlson[0][3][[1, 2, 4, 5]] == 1.0)


def _system(m, st):
    """(residual, Jacobian, increment) of one assembly and solve"""
    m.prepareStep(DT, st)
    m.assemble(True)
    m.getConvergence()
    dx = m.solveJacobianSystem(want_dx=True, single_precision=False)
    return m.residual(), m.jacobian()[2], dx


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_contexts_that_agree_bit_for_bit(gpu_lib):
    tab, grid, ref = _reference("all")
    mow, mgo, _ = ref[0]
    hst, new = kc.history_state(grid, tab, SEEDS[0]), decks.random_state(grid, tab, seed=11)
    prm = dict(linear_solver_reduction=1e-10, linear_solver_maxiter=400)

    def carlson(touch):
        m = _model(grid, tab, None, **prm)
        if touch == "setter":
            m.setHysteresisModel(capi.HYST_CARLSON)
        m.prepareStep(DT, hst)
        if touch == "there and back":
            m.setHysteresisModel(capi.HYST_KILLOUGH, 0.3)
        m.updateHysteresis()
        if touch == "there and back":
            m.setHysteresisModel(capi.HYST_CARLSON, 0.3)
        out = _system(m, new) + tuple(m.getHysteresis())
        m.close()
        return out
    never = carlson("never")
    assert _same(never, carlson("setter")) and _same(never, carlson("there and back"))

    wells = (np.array([0, 3], np.int32), np.array([2, 44, 86], np.int32))

    def killough(order):
        m = _model(grid, tab, None, **prm)
        m.prepareStep(DT, hst)
        if order == "model first":
            m.setHysteresisModel(capi.HYST_KILLOUGH, kc.A)
            m.updateHysteresis()
            m.setWells(*wells)                            # a re-plan with a resident history
        elif order == "wells first":
            m.setWells(*wells)
            m.updateHysteresis()                          # (Carlson's shifts, replaced by the setter)
            m.setHysteresisModel(capi.HYST_KILLOUGH, kc.A)
        else:                                             # restart: the history is set, the parameters follow
            m.setHysteresisModel(capi.HYST_KILLOUGH, kc.A)
            m.setWells(*wells)
            m.setHysteresis(mow, mgo)
        out = _system(m, new) + tuple(m.getHysteresis()) + tuple(m.getHysteresisScanning())
        # the model lasts through a saved and restored state and a change of the solve's precision
        m.saveState()
        m.setState(hst)
        m.restoreState()
        m.setSolvePrecision(True); m.setSolvePrecision(False)
        assert _same(_system(m, new), out[:3])
        m.close()
        return out
    # (Carlson's shifts too are carried through a re-plan in the cells' own order: history first, wells second == wells first)
    def carlson_replan(wells_first):
        m = _model(grid, tab, None, **prm)
        m.prepareStep(DT, hst)
        if wells_first:
            m.setWells(*wells)
        m.updateHysteresis()
        if not wells_first:
            m.setWells(*wells)
        m.prepareStep(DT, new)
        m.assemble(True)
        out = (m.residual(), m.jacobian()[2]) + tuple(m.getHysteresis())
        m.close()
        return out
    assert _same(carlson_replan(True), carlson_replan(False))
    first = killough("model first")
    assert _same(first, killough("wells first")) and _same(first, killough("restart"))
    assert np.abs(first[8] - 1.0).max() > 0.1 and np.abs(first[11] - 1.0).max() > 0.1        # (m_ow, m_go are not Carlson's 1)
    assert np.abs(first[2]).max() > 0.0


def test_refusals_carry_their_text(gpu_lib):
    tab, grid, _ = _reference("hysteresis")
    plain = decks.GridData(grid.nc, grid.conn_cells, grid.trans, grid.pv, grid.z, dims=grid.dims)
    m = GpuBlackoilModel(plain, tab, capi.default_params())
    with pytest.raises(ValueError, match="no hysteresis"):
        m.setHysteresisModel(capi.HYST_KILLOUGH, 0.1)
    with pytest.raises(ValueError, match="no hysteresis"):
        m.getHysteresisScanning()
    m.close()
    m = _model(grid, tab, capi.HYST_KILLOUGH, 0.25)
    m.prepareStep(DT, kc.history_state(grid, tab, 1))
    m.updateHysteresis()
    before = np.stack(m.getHysteresisScanning())
    for model, a, text in ((1, 0.1, "neither OPMGPU_HYST_CARLSON"), (3, 0.1, "neither OPMGPU_HYST_CARLSON"), (-1, 0.1, "neither OPMGPU_HYST_CARLSON"),
                           (capi.HYST_KILLOUGH, float("nan"), "not finite"), (capi.HYST_KILLOUGH, float("inf"), "not finite"),
                           (capi.HYST_KILLOUGH, -0.1, "negative"), (capi.HYST_CARLSON, -1.0, "negative")):
        with pytest.raises(ValueError, match=text):
            m.setHysteresisModel(model, a)
        assert np.array_equal(np.stack(m.getHysteresisScanning()), before)          # nothing changed
    m.setHysteresisModel(capi.HYST_KILLOUGH, 0.0)                                   # a = 0 is Land's trapping without Killough's term
    assert not np.array_equal(np.stack(m.getHysteresisScanning()), before)
    m.close()


def test_golden_deck_from_the_reader_to_the_restart_file(gpu_lib, tmp_path):
    """KILLOUGH_SMALL.DATA: gas injection, then water injection.  GASKR / OILKR of the last report step are the numpy rule on that step's
    own saturations and history planes to 1e-12 (the bound derived at test_kr_of_the_output_record_is_the_rule), and gas is trapped
    somewhere: Sncrt_go > Sncrd.  The restart file holds REAL (float32) arrays, as every restart file of this project does, so the
    comparison is made on the doubles the driver hands to the writer -- the model's state, history and output record at the end of the
    run -- and the file is checked to hold exactly their float32 roundings."""
    from opmgpu.simulator import Simulator
    base = str(tmp_path / "KILLOUGH")
    prm = capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, tolerance_mb=1e-9, tolerance_cnv=1e-5, tolerance_wells=1e-8,
                              linear_solver_reduction=1e-6, linear_solver_maxiter=200)
    sim = Simulator(DECK, params=prm, output_base=base)
    assert sim.deck.hysteresis_model() == (capi.HYST_KILLOUGH, 0.15)
    reps = sim.run()
    assert [r["days"] for r in reps] == [10.0, 30.0, 50.0, 80.0] and all(r["failed"] == 0 for r in reps)
    st, h, sd = sim.model.getState(), sim.model.getHysteresis(), sim.model.simulatorData()
    sw, sg, mow, mgo = st.sat[:, 0], st.sat[:, 2], h[0], h[1]
    rst = eclio.read_restart(base, len(reps) + 1)                  # (report 1 is the initial state)
    assert rst["DAYS"] == 80.0
    for name, arr in (("SWAT", sw), ("SGAS", sg), ("HMDC_OW", mow), ("HMDC_GO", mgo), ("GASKR", sd["GASKR"]), ("OILKR", sd["OILKR"])):
        assert np.array_equal(np.asarray(rst[name], np.float32), arr.astype(np.float32)), name
    tab, grid = sim.tables, sim.grid
    want = np.array([kref.kr_cell(tab, grid, c, mow[c], mgo[c], 0.15, sw[c], sg[c]) for c in range(grid.nc)])
    e_g, e_o = np.abs(sd["GASKR"] - want[:, 0]).max(), np.abs(sd["OILKR"] - want[:, 1]).max()
    pl = kref.scanning_planes(tab, grid, mow, mgo, 0.15)
    scanning = (mgo < 2.0) & (1.0 - sg > mgo) & ~pl["guard_go"] & (sg > pl["sncrt_go"])
    print("last report step: max |GASKR - rule| %.3e, max |OILKR - rule| %.3e; %d cells on the non-zero part of a gas scanning curve, "
          "Sncrt_go up to %.4f, krg up to %.3f" % (e_g, e_o, scanning.sum(), pl["sncrt_go"].max(), sd["GASKR"].max()))
    assert e_g <= 1e-12 and e_o <= 1e-12
    assert np.any(pl["sncrt_go"] > pl["sncrd_go"]) and scanning.any() and sd["GASKR"][scanning].max() > 0.01
    # the device's own planes are the rule's, and the model is what the deck says: Carlson's curves give other numbers
    got = sim.model.getHysteresisScanning()
    ok = ~pl["guard_go"] & (mgo < 2.0) & (pl["shy_go"] - pl["sncrd_go"] >= 0.02)
    assert ok.any() and np.allclose(got[3][ok], pl["sncrt_go"][ok], rtol=1e-13, atol=1e-15)
    sim.model.setHysteresisModel(capi.HYST_CARLSON)
    assert np.abs(sim.model.simulatorData()["GASKR"] - sd["GASKR"]).max() > 1e-4
