"""The VFP tables on the device (csrc/vfp.hpp through csrc/wells.hip) against the host restatement opmgpu/vfp.py.

  (a) opmgpu_vfp_evaluate -- the evaluators the well kernels call -- on the tables, points and derived bounds of tests/vfp_cases.py (the ones
      tests/test_vfp_twin.py runs through the host build of the same header), all eight tables set at once; with two sensitivity controls.
  (b) lockstep of DeviceWellModel against WellCoupledModel / StandardWellsHost on the oracle, as test_gpu_wells.py::
      test_device_well_controls_match_host does it and with its tolerances: a producer on THP control through a 5-axis FLO_LIQ / WFR_WCT /
      GFR_GLR table, a water injector on THP control through an injector table, a BHP-controlled producer that breaks its THP limit.
  (c) (the 5-axis producer case in test_gpu_wells.py::test_well_presolve_forms_agree)

Worst errors measured on an MI355X over the eight tables, in units of the derived bounds (each test prints its own): value 0.080, gradient in q
0.011, THP inversion 0.031.  Control margins: wfr <-> gfr at least 3.0e9 bounds, flo sign at least 1.1e10 bounds, at every random point.
"""
import numpy as np
import pytest

from opmgpu import capi, decks, wells as W
from opmgpu.model import GpuBlackoilModel
from util import OracleBackend

import vfp_cases as vc
from test_vfp_twin import _worst

pytestmark = pytest.mark.gpu

NAMES = list(vc.tables())


@pytest.fixture(scope="module")
def probe_model(gpu_lib):
    """the 300-cell deck with its two wells (no THP control) and all tables of vfp_cases set, in their order"""
    from test_wells_host import _limits_setup
    grid, tab, st, wl, _ = _limits_setup()
    gm = GpuBlackoilModel(grid, tab, capi.default_params())
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p), vfp_tables=list(vc.tables().values()))
    yield gm
    del md
    gm.close()


@pytest.mark.parametrize("name", NAMES)
def test_device_evaluators_match_host_restatement(probe_model, name):
    index = NAMES.index(name)                   # every table but the first lies behind others: VM_AXIS / VM_DATA offsets that are not 0
    t, pts, h = vc.tables()[name], vc.points(name), vc.host_values(name)
    bhp, dq, thp = probe_model.vfp_evaluate(index, pts["q"], pts["thp"], pts["alq"], pts["bhp_in"])
    worst = {"value": _worst(bhp - h.bhp, h.bhp_bound), "gradient": _worst(dq - h.dq, h.dq_bound), "thp": _worst(thp - h.thp, h.thp_bound)}
    print("%s on the device: worst error / bound %s; decisions of the THP inversion at >= %.3g bounds" % (name, worst, h.knot_margin))
    assert worst["value"] <= 1.0 and worst["gradient"] <= 1.0 and worst["thp"] <= 1.0, worst
    if t.thp.size == 1:
        assert np.all(thp == t.thp[0])
    if name == "dip":
        assert h.unsorted.all()
    # the same evaluation again: the probe leaves nothing behind
    again = probe_model.vfp_evaluate(index, pts["q"], pts["thp"], pts["alq"], pts["bhp_in"])
    assert np.array_equal(again[0], bhp) and np.array_equal(again[1], dq) and np.array_equal(again[2], thp)


@pytest.mark.parametrize("name", ["prod5_liq", "prod5_gas"])
def test_device_evaluators_sensitivity_controls(probe_model, name):
    """so that the comparison could fail: the host value with wfr and gfr looked up on each other's axis, and with flo looked up under the
    opposite sign, each lies at least 100 bounds away from what the device returns -- at every random point"""
    index = NAMES.index(name)
    t, pts, h = vc.tables()[name], vc.points(name), vc.host_values(name)
    sel = np.flatnonzero(pts["kind"] == "random")
    bhp, _, _ = probe_model.vfp_evaluate(index, pts["q"][sel], pts["thp"][sel], pts["alq"][sel], pts["bhp_in"][sel])
    swapped = np.array([vc.host_lookup(t, pts["q"][i], pts["thp"][i], pts["alq"][i], swap_ratios=True)[0] for i in sel])
    flipped = np.array([vc.host_lookup(t, pts["q"][i], pts["thp"][i], pts["alq"][i], flip_flo=True)[0] for i in sel])
    m_swap, m_flip = np.abs(swapped - bhp) / h.bhp_bound[sel], np.abs(flipped - bhp) / h.bhp_bound[sel]
    print("%s: control margins [bounds]: wfr <-> gfr min %.3g median %.3g; flo sign min %.3g median %.3g"
          % (name, m_swap.min(), np.median(m_swap), m_flip.min(), np.median(m_flip)))
    assert m_swap.min() >= 100.0 and m_flip.min() >= 100.0


def test_probe_is_refused_without_tables_and_for_an_unknown_table(gpu_lib, probe_model):
    from test_wells_host import _limits_setup
    grid, tab, st, wl, _ = _limits_setup()
    z = np.zeros(1)
    gm = GpuBlackoilModel(grid, tab, capi.default_params())
    with pytest.raises(ValueError):
        gm.vfp_evaluate(0, np.zeros(3), z, z, z)
    gm.close()
    for index in (-1, len(NAMES)):
        with pytest.raises(ValueError):
            probe_model.vfp_evaluate(index, np.zeros(3), z, z, z)


@pytest.mark.parametrize("case", ["prod_thp5", "inj_thp", "bhp_to_thp"])
@pytest.mark.parametrize("cpr", [0, 1])
def test_device_thp_control_matches_host(gpu_lib, oracle, case, cpr):
    """test_gpu_wells.py::test_device_well_controls_match_host for wells whose THP control runs through tables that exercise every axis:
      prod_thp5   a producer on THP through the 5-axis FLO_LIQ / WFR_WCT / GFR_GLR table, ALQ between nodes;
      inj_thp     a water injector on THP through an injector table;
      bhp_to_thp  a BHP-controlled producer whose THP limit is broken after the first update, so that it switches to THP control.
    The used table is the second one set: its blob offsets are not zero."""
    name = case
    kw = dict(thp_limit_bar=vc.host_thp_limit(oracle)) if name == "bhp_to_thp" else {}
    c = vc.lockstep_case(name, **kw)
    hws, hconv, hhist = vc.host_run(oracle, c)
    assert hconv
    vc.assert_case_claims(name, c, hws, hhist)          # the case tests what it claims: shown on the host before anything is compared
    grid, tab, st, wl, tables = c["grid"], c["tab"], c["st"], c["wells"], c["tables"]
    prm = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500, cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=cpr)
    prm_o = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500)
    dt = vc.LOCKSTEP_DT
    gm = GpuBlackoilModel(grid, tab, prm)
    ob = OracleBackend(oracle, grid, tab, prm_o, wells=wl.arrays())
    md = W.DeviceWellModel(gm, wl, c["well_state"](), vfp_tables=tables)
    mo = W.WellCoupledModel(ob, W.StandardWellsHost(wl, grid.z, tab.surface_density[0], vfp_tables=tables), c["well_state"]())
    md.prepareStep(dt, st); mo.prepareStep(dt, st)
    history = []
    it = 0
    while True:
        cd, _ = md.nonlinearIteration(it, single_precision=False)
        co, _ = mo.nonlinearIteration(it, single_precision=False)
        ws = md.pull_well_state()
        if it == 0:
            assert md.presolve_converged and md.presolve_iterations == mo.wh.well_iterations, (md.presolve_iterations, mo.wh.well_iterations)
        assert cd == co, it
        assert np.array_equal(ws.current, mo.ws.current), (it, ws.current, mo.ws.current)
        assert np.allclose(md.well_flux_residual, mo.wh.well_flux_residual, rtol=1e-5, atol=1e-12), it
        assert md.well_ctrl_residual == pytest.approx(mo.wh.well_ctrl_residual, rel=1e-5, abs=1e-9), it
        a, b = gm.getState(), ob.getState()
        assert np.array_equal(a.hc, b.hc), it
        assert np.abs(a.p - b.p).max() <= 1e-6 * np.abs(b.p).max() and np.abs(a.sat - b.sat).max() <= 1e-6, it
        assert np.allclose(ws.bhp, mo.ws.bhp, rtol=1e-7), (it, ws.bhp, mo.ws.bhp)
        assert np.allclose(ws.qs, mo.ws.qs, rtol=1e-6, atol=1e-9 * np.abs(mo.ws.qs).max()), it
        assert np.allclose(ws.thp, mo.ws.thp, rtol=1e-6, atol=1.0), (it, ws.thp, mo.ws.thp)
        history.append(ws.current.copy())
        it += 1
        if (cd and it > 1) or it > 12:
            break
    assert cd and it <= 12
    assert all(np.array_equal(x, y) for x, y in zip(history, hhist)) and len(history) == len(hhist)
    gm.close()


def test_probe_changes_nothing_a_later_solve_sees(gpu_lib):
    """the same two Newton iterations of the THP-controlled producer with and without probe calls in between: the same bits"""
    c = vc.lockstep_case("prod_thp5")
    pts = vc.points("prod5_oil")            # the decoy table of the case, set first
    out = []
    for probe in (False, True):
        gm = GpuBlackoilModel(c["grid"], c["tab"], capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500))
        md = W.DeviceWellModel(gm, c["wells"], c["well_state"](), vfp_tables=c["tables"])
        md.prepareStep(5 * decks.DAY, c["st"])
        for it in range(2):
            if probe:
                gm.vfp_evaluate(0, pts["q"], pts["thp"], pts["alq"], pts["bhp_in"])
                gm.vfp_evaluate(1, pts["q"], pts["thp"], pts["alq"][:] * 0.25, pts["bhp_in"])
            md.nonlinearIteration(it, single_precision=False)
        ws = md.pull_well_state()
        s = gm.getState()
        out.append((ws.bhp.copy(), ws.qs.copy(), ws.thp.copy(), s.p.copy(), s.sat.copy()))
        gm.close()
    assert all(np.array_equal(x, y) for x, y in zip(*out))
