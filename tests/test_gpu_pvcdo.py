"""GPU: the dead oil of constant compressibility and viscosibility (PVCDO, opmgpu_set_pvcdo) -- the output record against the numpy
restatement of the rule (tests/pvcdo_reference.py), Newton iterations in lockstep with the unchanged CPU oracle on the dense-PVDO twin
(tests/pvcdo_cases.py), the setter's discipline, and the golden deck through the report-step driver.

Tolerances.  Where the device is compared with the restatement, both evaluate the same closed form: 1e-12 relative.  Where it is compared
with the twin, the twin's own derived error is ADDED to the tolerance the corresponding existing test uses for a tabulated oil:
cases.tol_value() = 10 x (H c)^2 / 8 where values are compared (residual, convergence scalars), cases.tol_slope() = 2 x the slope bound
where slopes enter (Jacobian blocks, the updated state).  Existing figures: residual and Jacobian 1e-11 (tests/test_gpu_assembly.py,
tests/test_gpu_twophase.py), CNV 1e-9, MB 1e-7, B_avg 1e-12, state 1e-6 (tests/test_gpu_twophase.py, tests/util.py lockstep_parity).

Stone II: the CPU oracle has no Stone law (tests/test_gpu_stone.py compares with a restatement of kro, not with the oracle), so the twin of
that form is evaluated by the DEVICE through its tabulated-oil path, which this feature leaves as it was; the tolerances are the same."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from opmgpu import capi, decks, eclio, wells as W
from opmgpu import deck as deckmod
from opmgpu.model import GpuBlackoilModel
from opmgpu.simulator import Simulator
from util import OracleBackend, perforated_diag_mask, rel_err

import pvcdo_cases as cases
import pvcdo_reference as ref
import twophase as tp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = os.path.join(ROOT, "tests", "golden", "decks", "PVCDO_SMALL.DATA")
WORKER = os.path.join(ROOT, "tests", "_pvcdo_dist_worker.py")
DT = 5 * decks.DAY
RTOL = 1e-12


def _plain(t):
    """the same tables without the analytic oil: the constant stand-in alone"""
    p = copy.copy(t)
    p.pvcdo = None
    return p


# ---------------------------------------------------------------------------------------------------------------------------------------
# the output record and the other value-only evaluators
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", cases.FORMS)
def test_values_are_the_rule(gpu_lib, form):
    g = cases.grid()
    own, _ = cases.tables(form)
    st = cases.state(g, form)
    cells = np.arange(0, g.nc, 3, dtype=np.int32)
    m = GpuBlackoilModel(g, own, wells=(np.array([0, cells.size], np.int32), cells))
    m.setState(st)
    sd = m.simulatorData()
    pp = m.perfProps(cells.size).reshape(cells.size, 9, 4)
    press = np.minimum(st.p[cells] * 1.03, cases.P_HI * decks.BAR)
    b_perf, rsmax, _ = m.perfPvtAt(press)
    n = 8
    pv = np.linspace(cases.P_LO, cases.P_HI, n) * decks.BAR
    reg = (np.arange(n) % 2).astype(np.int32)
    coeff = np.zeros((n, 3))
    m._chk(m.lib.opmgpu_voidage_coefficients(m.ctx, n, capi.dptr(pv), capi.dptr(np.zeros(n)), capi.dptr(np.zeros(n)), capi.iptr(reg), capi.dptr(coeff)))
    fipnum = (1 + np.arange(g.nc) % 3).astype(np.int32)
    vals, fip = m.computeFluidInPlace(fipnum, cells=True)
    m.close()
    rows = ref.rows_of(cases.rows_si(), g.pvtnum)
    ib, dib = ref.inv_b(rows, st.p)
    mu, _ = ref.viscosity(rows, st.p)
    close = lambda a, b: np.allclose(a, b, rtol=RTOL, atol=0.0)        # noqa: E731
    print("1/Bo %.2e  mu_o %.2e" % (np.abs(sd["1OVERBO"] / ib - 1).max(), np.abs(sd["OIL_VISC"] / mu - 1).max()))
    assert close(sd["1OVERBO"], ib) and close(sd["OIL_VISC"], mu)
    assert close(sd["OIL_DEN"], own.surface_density[g.pvtnum, 1] * ib)
    # the oil is dead: no saturated solution ratio, no bubble point -- exactly
    assert np.all(sd["RSSAT"] == 0.0) and np.all(sd["PBUB"] == 0.0) and np.all(rsmax == 0.0)
    # perforation properties (value and d / dp of b_o), the perforation PVT at other pressures, the voidage coefficient
    assert close(pp[:, 4, 0], ib[cells]) and close(pp[:, 4, 1], dib[cells]) and np.all(pp[:, 4, 2:] == 0.0)
    assert close(b_perf[:, 1], ref.inv_b(rows[cells], press)[0])
    assert close(coeff[:, 1], 1.0 / ref.inv_b(cases.rows_si()[reg], pv)[0])
    # fluid in place, the oil row: pore-volume multiplier x b_o x S_o x pore volume
    cp = own.rock_comp * (st.p - own.rock_pref)
    oil = ((1.0 + cp + 0.5 * cp * cp) * ib) * st.sat[:, 1] * g.pv
    assert close(fip[1], oil)
    assert np.allclose(vals[:, 1], [oil[fipnum == r + 1].sum() for r in range(3)], rtol=RTOL, atol=0.0)
    # and none of this is the constant stand-in the context was created with
    assert np.abs(sd["1OVERBO"] * rows[:, 1] - 1.0).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------------
# two Newton iterations in lockstep with the twin
# ---------------------------------------------------------------------------------------------------------------------------------------
class _DeviceTwin:
    """the few calls the lockstep makes, on a device model with the twin's tabulated oil (the Stone form: the oracle has no Stone law)"""

    def __init__(self, g, twin, prm):
        self.m = GpuBlackoilModel(g, twin, prm)
        self.position = None

    def prepareStep(self, dt, st):
        self.m.prepareStep(dt, st)

    def assemble(self, initial):
        self.m.assemble(initial)
        self.r, self.val = self.m.residual(), self.m.jacobian()[2]

    def getConvergence(self):
        conv = self.m.getConvergence()
        self.CNV, self.MB, self.B_avg = self.m.CNV, self.m.MB, self.m.B_avg
        return conv

    def solveJacobianSystem(self):
        self.m.solveJacobianSystem(want_dx=False, single_precision=False)

    def updateState(self):
        self.m.updateState()

    def getState(self):
        return self.m.getState()

    def continue_from(self, st):
        self.m.setState(st)

    def close(self):
        self.m.close()


class _OracleTwin(OracleBackend):
    def continue_from(self, st):
        self.st = st.copy()

    def close(self):
        pass


@pytest.mark.parametrize("form", cases.FORMS)
def test_newton_lockstep_with_the_twin(gpu_lib, oracle, form):
    g = cases.grid()
    own, twin = cases.tables(form)
    st = cases.smooth_state(g, form)
    nc = g.nc
    tv, ts = cases.tol_value(), cases.tol_slope()
    prm = capi.default_params(linear_solver_reduction=1e-10, linear_solver_maxiter=2000)
    gm = GpuBlackoilModel(g, own, prm)
    ob = _DeviceTwin(g, twin, prm) if form == "stone2" else _OracleTwin(oracle, g, twin, capi.default_params(linear_solver_reduction=1e-10, linear_solver_maxiter=8000))
    ob.position = gm.ordering()[0]
    rowptr, col = oracle.pattern(g)
    ne = 2 if form == "ow" else 3                   # an oil-water deck's pinned gas unknown is not the twin's gas equation
    gm.prepareStep(DT, st); ob.prepareStep(DT, st)
    for it in range(2):
        gm.assemble(it == 0); ob.assemble(it == 0)
        gr, gc, gv = gm.jacobian()
        assert np.array_equal(gr, rowptr) and np.array_equal(gc, col)
        res = gm.residual()
        gv, val = gv.reshape(-1, 3, 3), np.asarray(ob.val).reshape(-1, 3, 3)
        e_r, e_j = rel_err(res[:ne * nc], ob.r[:ne * nc]), rel_err(gv[:, :ne, :ne], val[:, :ne, :ne])
        cg, co = gm.getConvergence(), ob.getConvergence()
        print("%s it %d: residual %.2e (tol %.2e)  Jacobian %.2e (tol %.2e)  CNV %s  MB %s" %
              (form, it, e_r, 1e-11 + tv, e_j, 1e-11 + ts, np.abs(gm.CNV[:ne] / ob.CNV[:ne] - 1), np.abs(gm.MB[:ne] / ob.MB[:ne] - 1)))
        assert e_r < 1e-11 + tv, (it, e_r)
        assert e_j < 1e-11 + ts, (it, e_j)
        # MB = |B_avg sum(R)| dt / sum(pv).  Without wells the fluxes of a closed grid cancel in that sum (at the first iteration the whole of
        # it is rounding), so next to the relative figure stands what the residual's own tolerance allows the sum to move: nc entries, each
        # by (1e-11 + tv) of the largest
        atol_mb = ob.B_avg[:ne] * nc * (1e-11 + tv) * np.abs(ob.r).max() * DT / g.pv.sum()
        assert np.allclose(gm.CNV[:ne], ob.CNV[:ne], rtol=1e-9 + tv)
        assert np.all(np.abs(gm.MB[:ne] - ob.MB[:ne]) <= (1e-7 + tv) * np.abs(ob.MB[:ne]) + atol_mb), (gm.MB, ob.MB, atol_mb)
        assert np.allclose(gm.B_avg[:ne], ob.B_avg[:ne], rtol=1e-12 + tv)
        assert cg == co, it                          # the same iterations are taken: neither side stops before the other
        gm.solveJacobianSystem(want_dx=False, single_precision=False)
        gm.updateState()
        ob.solveJacobianSystem()
        ob.updateState()
        a, b = gm.getState(), ob.getState()
        e_p, e_s = np.abs(a.p - b.p).max() / np.abs(b.p).max(), np.abs(a.sat[:, :ne] - b.sat[:, :ne]).max()
        print("   updated state: pressure %.2e  saturation %.2e (tol %.2e)" % (e_p, e_s, 1e-6 + ts))
        assert e_p <= 1e-6 + ts and e_s <= 1e-6 + ts, (it, e_p, e_s)
        if form == "ow":        # the oil-water twin's range of validity (tests/twophase.py): a cell the update took closer to connate water
            a.sat[:, 0] = np.maximum(a.sat[:, 0], tp.connate(g) + 1e-3); a.sat[:, 1] = 1.0 - a.sat[:, 0]       # than 1e-3 is put back there
            gm.setState(a)
        else:
            assert np.array_equal(a.hc, b.hc)
        ob.continue_from(a)
    gm.close(); ob.close()


def _wells(g):
    nx, ny, nz = g.dims
    colm = lambda i, j: [i + nx * j + nx * ny * k for k in range(nz)]      # noqa: E731
    WI = 5.0 * float(np.median(g.trans))
    wl = W.Wells()
    wl.add_well("INJ", W.INJECTOR, g.z[colm(0, 0)[0]], colm(0, 0), WI, (1.0, 0.0, 0.0), (W.SURFACE_RATE, 30.0 / 86400.0, (1.0, 0.0, 0.0)),
                limits=[(W.BHP, 600 * decks.BAR)])
    wl.add_well("P1", W.PRODUCER, g.z[colm(nx - 1, ny - 1)[0]], colm(nx - 1, ny - 1)[:4], WI, (0.0, 1.0, 0.0), (W.BHP, 150 * decks.BAR), limits=[])
    return wl


def test_newton_lockstep_with_device_wells(gpu_lib, oracle):
    """the default three-phase form with one injector and one BHP producer on the device, the oracle with the host well model on the twin;
    every cell in the first PVT region (the host well model of the oracle side takes ONE set of surface densities), so the bounds are those
    of that region's row"""
    g = cases.grid(pvt_regions=1)
    own, twin = cases.tables("default")
    st = cases.smooth_state(g, "default")
    nc = g.nc
    tv, ts = cases.tol_value(1), cases.tol_slope(1)
    wl = _wells(g)
    prm_g = capi.default_params(linear_solver_reduction=1e-10, linear_solver_maxiter=2000, cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=0)
    prm_o = capi.default_params(linear_solver_reduction=1e-10, linear_solver_maxiter=8000)
    gm = GpuBlackoilModel(g, own, prm_g)
    rowptr0, col0 = oracle.pattern(g)
    scale = np.asarray(prm_g.matbalscale[:])
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    ob = OracleBackend(oracle, g, twin, prm_o, wells=wl.arrays())
    mo = W.WellCoupledModel(ob, W.StandardWellsHost(wl, g.z, twin.surface_density[0]), W.WellState(wl, st.p))
    keep = ~perforated_diag_mask(rowptr0, col0, wl.cells)
    dt = 2 * decks.DAY
    md.prepareStep(dt, st); mo.prepareStep(dt, st)
    for it in range(2):
        gm.setSolvePrecision(False)
        gm.assemble(it == 0)
        mo.assemble(it == 0)
        _, val_res, _, _ = oracle.assemble(g, twin, dt, ob.st, rowptr0, col0, scale=tuple(scale), accum0=ob.acc0)
        if it == 0:
            md.pull_well_state()
            assert md.presolve_converged
        gr, gc, gv = gm.jacobian()
        assert np.array_equal(gr, rowptr0) and np.array_equal(gc, col0)
        e_r = rel_err(gm.residual(), ob.r)
        e_j = rel_err(gv.reshape(-1, 3, 3)[keep], val_res.reshape(-1, 3, 3)[keep])
        print("wells it %d: residual %.2e (tol %.2e)  Jacobian %.2e (tol %.2e)" % (it, e_r, 1e-11 + tv, e_j, 1e-11 + ts))
        assert e_r < 1e-11 + tv and e_j < 1e-11 + ts, (it, e_r, e_j)
        cg = gm.getConvergence(); co = ob.getConvergence()
        assert np.allclose(gm.CNV, ob.CNV, rtol=1e-9 + tv) and np.allclose(gm.MB, ob.MB, rtol=1e-7 + tv, atol=1e-18)
        assert np.allclose(gm.B_avg, ob.B_avg, rtol=1e-12 + tv)
        cg = md.wellConvergence() and cg; co = mo.wh.converged(ob.B_avg) and co
        assert np.allclose(md.well_flux_residual, mo.wh.well_flux_residual, rtol=1e-7 + ts, atol=1e-14)
        assert cg == co, it
        gm.solveJacobianSystem(want_dx=False, single_precision=False)
        gm.updateState()
        ob.solveJacobianSystem(single_precision=False)
        mo.wh.recover_and_update(ob.perfDx(wl.nperf), mo.ws)
        ob.updateState()
        a, b = gm.getState(), ob.getState()
        e_p, e_s = np.abs(a.p - b.p).max() / np.abs(b.p).max(), np.abs(a.sat - b.sat).max()
        print("   updated state: pressure %.2e  saturation %.2e (tol %.2e)" % (e_p, e_s, 1e-6 + ts))
        assert e_p <= 1e-6 + ts and e_s <= 1e-6 + ts, (it, e_p, e_s)
        ob.st = a.copy()
        ws = md.pull_well_state()
        assert np.allclose(ws.bhp, mo.ws.bhp, rtol=1e-6 + ts), (it, ws.bhp, mo.ws.bhp)
        assert np.allclose(ws.qs, mo.ws.qs, rtol=1e-5 + ts, atol=(1e-8 + ts) * np.abs(mo.ws.qs).max()), it
        assert np.array_equal(ws.current, mo.ws.current), it
        mo.ws.assign(ws)
    gm.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the setter
# ---------------------------------------------------------------------------------------------------------------------------------------
WELLS = (np.array([0, 3, 5], np.int32), np.array([7, 7 + 35, 7 + 70, 200, 235], np.int32))


def _assembled(g, t, st, steps, single=False):
    """create on tables t (FluidTables(pvcdo=...) sets the form right after creation), run the steps (("pvcdo", rows or None) /
    ("wells", wells)) in order, assemble once -> (residual, Jacobian values)"""
    m = GpuBlackoilModel(g, t, capi.default_params())
    for what, arg in steps:
        if what == "pvcdo":
            m.setPvcdo(arg)
        else:
            m.setWells(*arg)
    m.prepareStep(DT, st)
    m.setSolvePrecision(single)
    m.assemble(True)
    out = m.residual(), m.jacobian()[2]
    m.close()
    return out


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("form", ["default", "ow"])
def test_setter_discipline(gpu_lib, form):
    g = cases.grid()
    own, _ = cases.tables(form)
    plain = _plain(own)
    st = cases.state(g, form)
    rows = cases.rows_si()
    with_form, without = _assembled(g, own, st, []), _assembled(g, plain, st, [])
    assert not _same(with_form, without)                                                  # the form acts on this state
    assert _same(_assembled(g, plain, st, [("pvcdo", rows)]), with_form)                  # set by hand = set by the model at creation
    assert _same(_assembled(g, own, st, [("pvcdo", None)]), without)                      # NULL: a context that never set it
    assert _same(_assembled(g, plain, st, [("pvcdo", rows[::-1].copy()), ("pvcdo", rows)]), with_form)      # replaced
    # a re-plan (new well pattern) after the setter = the setter after the re-plan, and the form is still there
    replanned = _assembled(g, own, st, [("wells", WELLS)])
    assert _same(replanned, _assembled(g, plain, st, [("wells", WELLS), ("pvcdo", rows)]))
    assert not _same(replanned, _assembled(g, plain, st, [("wells", WELLS)]))
    # a change of the solve's precision: the residual (always double) is the form's, the float Jacobian its rounding
    f32 = _assembled(g, own, st, [], single=True)
    assert np.array_equal(f32[0], with_form[0]) and rel_err(f32[1], with_form[1]) < 2e-6 and not np.array_equal(f32[0], without[0])


def test_setter_refusals(gpu_lib):
    g = cases.grid()
    own, _ = cases.tables("default")
    st = cases.state(g, "default")
    rows = cases.rows_si()
    m = GpuBlackoilModel(g, own, capi.default_params())
    for k, bad, word in ((2, np.nan, "not finite"), (0, np.inf, "not finite"), (1, 0.0, "B_ref"), (1, -1.0, "B_ref"), (3, 0.0, "viscosity"), (3, -2e-3, "viscosity")):
        v = rows.copy(); v[1, k] = bad
        assert m.lib.opmgpu_set_pvcdo(m.ctx, capi.dptr(v)) == capi.EINVAL
        why = m.lib.opmgpu_last_error(m.ctx).decode()
        assert word in why and "region 1" in why, why
        with pytest.raises(ValueError, match=word):
            m.setPvcdo(v)
    with pytest.raises(ValueError, match="PVT region"):
        m.setPvcdo(rows[:1])
    m.prepareStep(DT, st)                             # a refused call changed nothing
    m.assemble(True)
    got = m.residual(), m.jacobian()[2]
    m.close()
    assert _same(got, _assembled(g, own, st, []))
    # a context with dissolved gas: the analytic oil is dead
    live = decks.satfunc_standard_tables(regions=2)
    assert live.has_disgas == 1
    m = GpuBlackoilModel(g, live, capi.default_params())
    assert m.lib.opmgpu_set_pvcdo(m.ctx, capi.dptr(rows)) == capi.EINVAL
    assert "has_disgas" in m.lib.opmgpu_last_error(m.ctx).decode()
    with pytest.raises(ValueError, match="has_disgas"):
        m.setPvcdo(rows)
    m.setPvcdo(None)                                  # going back to the tabulated oil is always allowed
    m.close()
    # wet gas over the dead oil (has_vapoil) is allowed
    wet = decks.FluidTables(density_wog=[[1000.0, 700.0, 1.0]] * 2, pvtw=[[1.0, 1.0, 4.0e-5, 0.96, 0.0]] * 2, pvto=None, pvcdo=cases.ROWS,
                            pvtg=[[(100, [(0.0001, 0.010, 0.1), (0.0, 0.0104, 0.1)]), (200, [(0.0004, 0.005, 0.2), (0.0, 0.0054, 0.2)])]] * 2,
                            swof=[cases.SWOF3] * 2, sgof=[cases.SGOF3] * 2, rock=(1.0, 5.0e-5), disgas=False, vapoil=True)
    m = GpuBlackoilModel(g, wet, capi.default_params())
    m.setState(st)
    ib = m.simulatorData()["1OVERBO"]
    m.close()
    assert np.allclose(ib, ref.inv_b(ref.rows_of(rows, g.pvtnum), st.p)[0], rtol=RTOL, atol=0.0)


def test_saved_state_keeps_the_form(gpu_lib):
    g = cases.grid()
    own, _ = cases.tables("ow")
    st = cases.smooth_state(g, "ow")
    m = GpuBlackoilModel(g, own, capi.default_params(linear_solver_reduction=1e-8, linear_solver_maxiter=400))
    m.prepareStep(DT, st)
    m.saveState()
    m.assemble(True)
    first = m.residual(), m.jacobian()[2]
    m.getConvergence()
    m.solveJacobianSystem(want_dx=False, single_precision=False)
    m.updateState()
    assert np.abs(m.getState().p - st.p).max() > 0.0
    m.restoreState()
    m.assemble(True)
    again = m.residual(), m.jacobian()[2]
    m.close()
    assert _same(first, again) and not _same(first, _assembled(g, _plain(own), st, []))


# ---------------------------------------------------------------------------------------------------------------------------------------
# two ranks over the shared-memory test transport: every rank sets its own copy
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_assemble_the_single_domain_residual(gpu_lib, tmp_path):
    """The owned cells' residual of a 2-rank run against the single-domain one.  tests/test_gpu_thpres_dist.py compares maxima, which do not
    depend on an order, exactly; a residual is a SUM over the row's connections taken in the order of the rank's own plan, so two plans
    may differ in the last bits: 1e-13 of the largest residual entry (a row has at most 6 connections x 3 phases of terms near that size,
    each rounded at 1.1e-16), and the figure is printed."""
    g = cases.grid()
    own, _ = cases.tables("default")
    st = cases.smooth_state(g, "default")
    single = _assembled(g, own, st, [])[0].reshape(3, g.nc)
    plain = _assembled(g, _plain(own), st, [])[0].reshape(3, g.nc)
    env = dict(os.environ, OPMGPU_COMM_TRANSPORT="shm")
    env["PYTHONPATH"] = os.path.join(ROOT, "opm-simulators-legacy_amd") + os.pathsep + env.get("PYTHONPATH", "")
    code = "from opmgpu import partition; print(partition.make_unique_id().hex())"
    uid = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
    world = 2
    outs = [str(tmp_path / ("r%d.npz" % r)) for r in range(world)]
    procs = [subprocess.Popen([sys.executable, WORKER, "0", str(r), str(world), uid, outs[r]], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, logs[r][-6000:])
    seen = np.zeros(g.nc, bool)
    scale = np.abs(single).max()
    for o in outs:
        q = np.load(o)
        ids, res = q["ids"], q["residual"]
        err = np.abs(res - single[:, ids]).max()
        print("owned residual against the single domain: %.3e of the largest entry (exact: %s)" % (err / scale, np.array_equal(res, single[:, ids])))
        assert err <= 1e-13 * scale
        assert np.abs(res - plain[:, ids]).max() > 1e-6 * scale                           # the rank did set its copy
        seen[ids] = True
    assert seen.all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the golden deck through the report-step driver, device wells
# ---------------------------------------------------------------------------------------------------------------------------------------
def _twin_deck_text():
    """the golden deck with its PVCDO records replaced by PVDO tables sampling them every H: an ordinary tabulated dead oil"""
    text = open(DECK).read()
    a, b = text.index("PVCDO\n"), text.index("PVTW\n")
    rows = deckmod.read_deck(DECK).records("PVCDO")
    pvdo = "PVDO\n"
    for r in rows:
        pvdo += "\n".join(" %.17g %.17g %.17g" % row for row in cases.dense_pvdo(tuple(r[:5]))) + " /\n"
    return text[:a] + pvdo + text[b:]


def test_golden_deck_runs_and_matches_its_twin(gpu_lib, tmp_path):
    tight = dict(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, tolerance_mb=1e-9, tolerance_cnv=1e-5, tolerance_wells=1e-8, linear_solver_reduction=1e-9,
                 linear_solver_maxiter=400)
    base, base_twin = str(tmp_path / "PVCDO"), str(tmp_path / "TWIN")
    sim = Simulator(DECK, params=capi.default_params(**tight), output_base=base)
    sim.model.max_single_precision_days = 0.0
    assert sim.tables.pvcdo is not None and sim.tables.phases == "wo"
    rows = ref.rows_of(sim.tables.pvcdo, sim.grid.pvtnum)
    rho_s = sim.tables.surface_density[sim.grid.pvtnum]

    def in_place(state):          # water and oil in place by the rule (water: PVTW's own closed form) -- mass per cell summed
        t = sim.tables
        w = t.pvtw[sim.grid.pvtnum]
        x = w[:, 2] * (state.p - w[:, 0])              # (the water pressure differs by pcow: immaterial to a sign check)
        bw = (1.0 + x * (1.0 + x / 2.0)) / w[:, 1]
        cp = t.rock_comp * (state.p - t.rock_pref)
        pvm = (1.0 + cp + 0.5 * cp * cp) * sim.grid.pv
        return np.array([(pvm * bw * state.sat[:, 0]).sum(), (pvm * ref.inv_b(rows, state.p)[0] * state.sat[:, 1]).sum()])
    v0 = in_place(sim.model.getState())
    reps = sim.run()
    assert [r["days"] for r in reps] == [10.0, 20.0, 40.0] and all(r["substeps"] >= 1 and r["failed"] == 0 for r in reps)
    final = sim.model.getState()
    sd = sim.model.simulatorData()
    assert np.allclose(sd["1OVERBO"], ref.inv_b(rows, final.p)[0], rtol=RTOL, atol=0.0)
    assert np.allclose(sd["OIL_DEN"], rho_s[:, 1] * ref.inv_b(rows, final.p)[0], rtol=RTOL, atol=0.0)
    # material balance as tests/test_gpu_twophase_deck.py bounds it: water came in, oil went out; and the driver's own oil in place is the rule's
    dv = in_place(final) - v0
    assert dv[0] > 0 and dv[1] < 0
    assert reps[-1]["fip"][:, 1].sum() == pytest.approx(in_place(final)[1], rel=1e-10)
    sp = {a[0]: a[2] for a in eclio.read_arrays(base + ".SMSPEC")}
    kw, wg = list(sp["KEYWORDS"]), list(sp["WGNAMES"])
    idx = lambda k, g_: next(i for i, (a, b) in enumerate(zip(kw, wg)) if a == k and b == g_)      # noqa: E731
    smry = [a[2] for a in eclio.read_arrays(base + ".UNSMRY") if a[0] == "PARAMS"]
    assert len(smry) == 3 and sum(r[idx("FWIR", ":+:+:+:+")] for r in smry) > 0
    for r in smry:
        assert r[idx("WBHP", "PROD")] == pytest.approx(235.0, rel=1e-5) and r[idx("WOPR", "PROD")] > 0.0
    sim.close()
    # the dense twin, an ordinary PVDO deck, through the same driver on the device: PRESSURE and SWAT within compare's defaults (2e-2 / 1e-5)
    twin_path = str(tmp_path / "TWIN.DATA")
    with open(twin_path, "w") as f:
        f.write(_twin_deck_text())
    sim2 = Simulator(twin_path, params=capi.default_params(**tight), output_base=base_twin)
    sim2.model.max_single_precision_days = 0.0
    assert sim2.tables.pvcdo is None and sim2.tables.oil_psat.size == 2 * 3201
    reps2 = sim2.run()
    sim2.close()
    assert [r["days"] for r in reps2] == [10.0, 20.0, 40.0]
    assert eclio.compare(base, base_twin, restart_keywords=("PRESSURE", "SWAT"), summary=False) == []
