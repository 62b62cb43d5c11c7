"""GPU: well efficiency factors (WEFAC; opmgpu_set_well_efficiency, WellArgs::eff of csrc/wells.hip).  The rule (include/opmgpu.h): the CELLS
see e_w times the well's rates and their derivatives -- residual, own-cell diagonal block, P and rhs_extra of the factored Schur form, the
bordered pressure level's well column -- the well equations and the well state do not see e_w.
  1 a context that never called the setter, one that passed NULL and one that passed ones compute the same bits
  2 at a fixed state the wells' contribution to residual and diagonal blocks is linear in e_w, well by well
  3 Newton parity with the reference subclass (tests/wefac_reference.py: one coupled system, direct solve) and with the host well model
  4 material balance of a waterflood: the fluid in place changes by the e-weighted well volumes
  5 the factors last through saved states, a change of precision and a re-plan, a new well list resets them; the refusals
  6 two ranks over the shared-memory test transport, one well each
  7 tests/golden/decks/WEFAC_SMALL.DATA through the report-step driver to the summary file"""
import os
import subprocess
import sys

import numpy as np
import pytest

from opmgpu import capi, decks, eclio, wells as W
from opmgpu.model import GpuBlackoilModel
from test_wefac import DECK, EFF, seeded_state, with_factors
from test_wells_host import _setup
from util import OracleBackend
from wefac_reference import WefacOracleModel, arrays
import well_size_decks as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_wefac_dist_worker.py")
EPS = np.finfo(float).eps


def _diag_blocks(gm):
    rowptr, col, val = gm.jacobian()
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    d = rows == col
    out = np.zeros((rowptr.size - 1, 9))
    out[rows[d]] = val[d]
    return out, val[~d]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1: never set = NULL = ones, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cpr", [0, 1])
@pytest.mark.parametrize("single", [False, True])
def test_unit_factors_are_the_context_that_never_set_them(gpu_lib, single, cpr):
    grid, tab, st, wl = _setup()
    out = {}
    for how in ("never", "null", "ones"):
        gm = GpuBlackoilModel(grid, tab, capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=cpr))
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
        if how == "null":
            assert gpu_lib.opmgpu_set_well_efficiency(gm.ctx, None) == capi.OK
        elif how == "ones":
            gm.setWellEfficiency(np.ones(wl.nw))
        assert np.array_equal(gm.getWellEfficiency(), np.ones(wl.nw))
        md.prepareStep(2 * decks.DAY, st)
        gm.setSolvePrecision(single)
        gm.assemble(True)
        gm.getConvergence()
        res, jac = gm.residual(), gm.jacobian()[2]
        dx = gm.solveJacobianSystem(want_dx=True, single_precision=single)
        gm.updateState()
        ws = md.pull_well_state()
        out[how] = (res, jac, dx, ws.bhp.copy(), ws.qs.copy(), ws.perf_rates.copy(), ws.perf_press.copy(), gm.getState().p)
        gm.close()
    for how in ("null", "ones"):
        for k, (a, b) in enumerate(zip(out["never"], out[how])):
            assert np.array_equal(a, b), (how, k)
    assert np.abs(out["never"][2]).max() > 0 and np.abs(out["never"][4]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2: linearity, well by well
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_assemblies(gpu_lib):
    """residual and Jacobian blocks of tests/well_size_decks.long_deck() (nine wells of 1 to 320 perforations) at ONE state and well state,
    without the well pre-solve: no wells; factors 1; factors e_w = 0.3 + 0.07 w with 1.0 for well 4; e with well 6 alone changed"""
    deck = D.long_deck()
    wl = deck.wl
    e = 0.3 + 0.07 * np.arange(wl.nw)
    e[4] = 1.0
    e2 = e.copy(); e2[6] = 0.61
    out = {}
    for name, eff in (("none", None), ("one", np.ones(wl.nw)), ("e", e), ("e2", e2)):
        gm = GpuBlackoilModel(deck.grid, deck.tab, capi.default_params(solve_welleq_initially=0))
        md = gm
        if eff is not None:
            md = W.DeviceWellModel(gm, with_factors(D.long_deck().wl, eff), W.WellState(wl, deck.st.p))
        md.prepareStep(deck.dt, deck.st)
        gm.setSolvePrecision(False)
        gm.assemble(True)
        diag, off = _diag_blocks(gm)
        ws = md.pull_well_state().copy() if eff is not None else None
        out[name] = (gm.residual().reshape(3, deck.grid.nc), diag, off, ws)
        gm.close()
    return deck, e, e2, out


def test_cell_rows_are_linear_in_the_wells_factor(long_assemblies):
    """R(e) - R(no wells) = e_w (R(1) - R(no wells)) in every perforated cell, and the same for its diagonal block.
    Bound, with u = eps / 2 and M = the largest of |X0|, |X1|, |Xe| of the entry (X = R or a block entry, X0 without wells):  the device
    forms X1 = fl(X0 - t) and Xe = fl(X0 - fl(e t)) (a fused multiply-add drops the inner rounding; for a block entry t = s d with the
    scaling s and e s rounded once more): errors u |X1|, u |Xe|, 2 u |e t|;  the test forms D1 = fl(X1 - X0), De = fl(Xe - X0) and
    fl(e D1): u |D1|, u |De|, u |e D1|.  With |t|, |D1|, |De| <= 2 M and e <= 1 the sum is <= (1 + 1 + 4 + 2 + 2 + 2) u M = 6 eps M."""
    deck, e, e2, out = long_assemblies
    wl = deck.wl
    cells = np.asarray(wl.cells)
    e_perf = np.repeat(e, np.diff(wl.connpos))
    assert len(set(e.tolist())) == wl.nw and e[4] == 1.0 and e.max() <= 1.0 and np.diff(wl.connpos).max() == 320
    for k in (0, 1):                                            # residual [3, nc] -> [nperf, 3]; diagonal blocks [nc, 9] -> [nperf, 9]
        pick = (lambda x: x[:, cells].T) if k == 0 else (lambda x: x[cells])
        x0, x1, xe = (pick(out[n][k]) for n in ("none", "one", "e"))
        M = np.maximum(np.maximum(np.abs(x0), np.abs(x1)), np.abs(xe))
        err = np.abs((xe - x0) - e_perf[:, None] * (x1 - x0))
        touched = x1 != x0                     # (a perforation the cross-flow rule shuts -- wells 7 and 8 -- contributes exactly nothing)
        per_well = np.add.reduceat(touched.any(1).astype(int), wl.connpos[:-1])
        assert touched.any(0).all() and (per_well > 0).all() and touched.any(1).sum() >= 0.7 * wl.nperf, per_well
        worst = (err / np.where(M > 0, M, 1.0)).max() / EPS
        print("%s: worst deviation from linearity %.2f eps of the largest term" % (("residual", "diagonal blocks")[k], worst))
        assert np.all(err <= 6 * EPS * M), (k, worst)
        # the factor acts: where e_w < 1 the weighted entries differ from the unweighted ones (well 4, e = 1, gives the same bits)
        w4 = slice(wl.connpos[4], wl.connpos[5])
        assert np.array_equal(xe[w4], x1[w4])
        assert np.array_equal((xe != x1).any(1), touched.any(1) & (e_perf != 1.0))
    # unperforated cells and the off-diagonal blocks never see a well
    free = np.ones(deck.grid.nc, bool); free[cells] = False
    for n in ("one", "e", "e2"):
        assert np.array_equal(out[n][0][:, free], out["none"][0][:, free]) and np.array_equal(out[n][1][free], out["none"][1][free])
        assert np.array_equal(out[n][2], out["none"][2])
    # another factor for well 6 alone: the cells of every other well keep their bits, those of well 6 do not
    w6 = np.zeros(wl.nperf, bool); w6[wl.connpos[6]:wl.connpos[7]] = True
    assert np.array_equal(out["e2"][0][:, cells[~w6]], out["e"][0][:, cells[~w6]]) and np.array_equal(out["e2"][1][cells[~w6]], out["e"][1][cells[~w6]])
    assert np.all((out["e2"][0][:, cells[w6]] != out["e"][0][:, cells[w6]]).any(0))
    # the well equations do not see the factor: the well state the assembly leaves (perfPhaseRates, perfPress, rates, bhp) is the same
    for n in ("e", "e2"):
        a, b = out["one"][3], out[n][3]
        assert np.array_equal(a.perf_rates, b.perf_rates) and np.array_equal(a.perf_press, b.perf_press) and np.array_equal(a.qs, b.qs) and np.array_equal(a.bhp, b.bhp)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3: Newton parity with the reference subclass and the host well model
# ---------------------------------------------------------------------------------------------------------------------------------------
def _parity_deck(name):
    if name == "setup":
        grid, tab, st, wl = _setup()
        return grid, tab, st, (lambda: _setup()[3]), np.asarray(EFF), 2 * decks.DAY
    deck = D.many_deck(65)
    e = 0.3 + 0.07 * (np.arange(65) % 10)
    e[64] = 1.0
    return deck.grid, deck.tab, deck.st, (lambda: D.many_deck(65).wl), e, deck.dt


@pytest.mark.parametrize("cpr", [0, 1])
@pytest.mark.parametrize("name", ["setup", "many65"])
def test_newton_parity_with_the_reference_and_the_host_model(gpu_lib, oracle, name, cpr):
    """Device wells with factors against (a) the reference subclass of the independent oracle model and (b) the host well model with factors on
    the CPU oracle: two Newton iterations, the tolerances of tests/test_gpu_wells.py::test_device_wells_match_host_wells_on_the_oracle.
    many65: 65 wells, one past the 64-lane stride of the loops over wells, a distinct factor per lane position."""
    grid, tab, st, make, e, dt = _parity_deck(name)
    prm = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500, cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=cpr)
    prm_o = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=8000)
    wl_d, wl_h, wl_r = (with_factors(make(), e) for _ in range(3))
    gm = GpuBlackoilModel(grid, tab, prm)
    md = W.DeviceWellModel(gm, wl_d, seeded_state(wl_d, st.p))
    assert np.array_equal(gm.getWellEfficiency(), e)
    ob = OracleBackend(oracle, grid, tab, prm_o, wells=wl_h.arrays())
    mo = W.WellCoupledModel(ob, W.StandardWellsHost(wl_h, grid.z, tab.surface_density[0]), seeded_state(wl_h, st.p))
    ref = WefacOracleModel(grid, tab, prm_o, wl_r, arrays(seeded_state(wl_r, st.p)), e)
    md.prepareStep(dt, st); mo.prepareStep(dt, st); ref.prepareStep(dt, st)
    for it in range(2):
        cd, _ = md.nonlinearIteration(it, single_precision=False)
        co, _ = mo.nonlinearIteration(it, single_precision=False)
        cr = ref.nonlinearIteration(it)
        assert cd == co == cr, it
        ws = md.pull_well_state()
        a = gm.getState()
        for tag, flux, ctrl, b, wsb, cnv in (("host", mo.wh.well_flux_residual, mo.wh.well_ctrl_residual, ob.getState(), mo.ws, ob.CNV),
                                             ("reference", ref.well_flux_residual, ref.well_ctrl_residual, ref.st, ref.ws, ref.CNV)):
            assert np.allclose(md.well_flux_residual, flux, rtol=1e-5, atol=1e-12), (tag, it)
            assert md.well_ctrl_residual == pytest.approx(ctrl, rel=1e-5, abs=1e-12), (tag, it)
            assert np.array_equal(a.hc, b.hc), (tag, it)
            assert np.abs(a.p - b.p).max() <= 1e-6 * np.abs(b.p).max(), (tag, it)
            assert np.abs(a.sat - b.sat).max() <= 1e-6, (tag, it)
            assert np.allclose(ws.bhp, wsb.bhp, rtol=1e-7), (tag, it)
            assert np.allclose(ws.qs, wsb.qs, rtol=1e-6, atol=1e-9 * np.abs(wsb.qs).max()), (tag, it)
            assert np.allclose(ws.perf_rates, wsb.perf_rates, rtol=1e-6, atol=1e-9 * np.abs(wsb.perf_rates).max()), (tag, it)
            assert np.allclose(gm.CNV, cnv, rtol=1e-5, atol=1e-9), (tag, it)
    assert (ws.qs[np.asarray(wl_d.type) == W.INJECTOR, 0] > 0).all()
    gm.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4: material balance
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_waterflood_material_balance_with_factors(gpu_lib, oracle):
    """The waterflood of tests/test_gpu_wells.py::test_waterflood_material_balance_through_adaptive_stepping with the injector on 80 % and the
    producer on 50 % uptime: over every converged sub-step the change of each component's surface volume in place equals dt times the
    e-weighted well rates, at that test's tolerance -- and misses the unweighted sum by the volume the wells did not move, dt times
    sum_w (1 - e_w) q_w: for oil and gas, which the producer alone moves, half its rate, asked to be 1000 times the tolerance (the first
    sub-step measured 9e4 and 5e4 times; water, 1e4 times there, is printed only: the injector's 0.2 and the producer's 0.5 of its water
    rate have opposite signs)."""
    from opmgpu import timestepping as ts
    from opmgpu.model import NonlinearSolver
    grid, tab, st, wl = _setup()
    e = np.array([0.8, 0.5])
    with_factors(wl, e)
    prm = capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, tolerance_mb=1e-10, tolerance_cnv=1e-6, linear_solver_reduction=1e-8, linear_solver_maxiter=300)
    gm = GpuBlackoilModel(grid, tab, prm)
    model = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p), tolerance_wells=1e-9, tolerance_well_control=1e-9)
    gm.setState(st)
    names = oracle.PROP_NAMES

    def in_place():
        props = oracle.cell_props(grid, tab, gm.getState())
        return np.array([(props[:, names.index("accum_" + c), 0] * grid.pv).sum() for c in "wog"])

    class Recorder:
        def __init__(self):
            self.inner, self.steps = NonlinearSolver(), []

        def step(self, m):
            before = in_place()
            out = self.inner.step(m, single_precision=False)
            ws = model.pull_well_state()
            self.steps.append((m.m.dt, before, in_place(), ws.qs.copy()))
            return out

    rec = Recorder()
    ats = ts.AdaptiveTimeStepping(initial_timestep_days=1.0)
    rep = ats.step(0.0, 30 * decks.DAY, rec, model)
    assert rep["converged"] and len(rep["substeps"]) >= 3 and sum(rep["substeps"]) == pytest.approx(30 * decks.DAY)
    inj_rate = 2000.0 / 86400.0
    for dt, before, after, qs in rec.steps[-len(rep["substeps"]):]:
        scale = inj_rate * dt
        tol = 1e-5 * np.array([scale, scale, 200 * scale])
        weighted = (e[:, None] * qs).sum(axis=0) * dt
        plain = qs.sum(axis=0) * dt
        assert np.all(np.abs((after - before) - weighted) <= tol), (dt / decks.DAY, after - before, weighted)
        assert abs(qs[0, 0] - inj_rate) <= 1e-9 and qs[1, 1] < 0             # the well's own rate is its target, unweighted
        miss = np.abs((after - before) - plain)
        print("dt %.2f d: the unweighted sum misses by %s tolerances (w, o, g)" % (dt / decks.DAY, np.round(miss / tol).tolist()))
        assert np.allclose(miss, np.abs(((1.0 - e)[:, None] * qs).sum(axis=0)) * dt, rtol=0, atol=tol)
        assert miss[1] >= 1e3 * tol[1] and miss[2] >= 1e3 * tol[2], (dt / decks.DAY, miss, tol)
    gm.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5: persistence and refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_factors_last_and_are_reset_by_a_new_well_list(gpu_lib):
    grid, tab, st, wl = _setup()
    e = np.asarray(EFF)

    def assembled(gm, md):
        md.push_well_state()            # an assembly rewrites perfPhaseRates, which the next one's connection pressures read: same start every time
        gm.assemble(True)
        return gm.residual(), gm.jacobian()[2]

    prm = lambda: capi.default_params(solve_welleq_initially=0)          # noqa: E731  (the pre-solve would move the well state between assemblies)

    def fresh(eff, single):
        gm = GpuBlackoilModel(grid, tab, prm())
        md = W.DeviceWellModel(gm, with_factors(_setup()[3], eff), W.WellState(wl, st.p))
        md.prepareStep(2 * decks.DAY, st)
        gm.setSolvePrecision(single)
        out = assembled(gm, md)
        gm.close()
        return out

    unit_d, want_d, want_f = fresh((1.0, 1.0), False), fresh(e, False), fresh(e, True)
    assert not np.array_equal(unit_d[0], want_d[0])
    gm = GpuBlackoilModel(grid, tab, prm())
    md = W.DeviceWellModel(gm, _setup()[3], W.WellState(wl, st.p))
    gm.setWellEfficiency(e)
    md.prepareStep(2 * decks.DAY, st)
    gm.setSolvePrecision(False)
    gm.saveState()
    first = assembled(gm, md)
    assert np.array_equal(first[0], want_d[0]) and np.array_equal(first[1], want_d[1])          # the setter = the factors DeviceWellModel sets
    # saved states: the factors are no part of them
    gm.setWellEfficiency(None)
    gm.saveState()
    gm.setWellEfficiency(e)
    gm.restoreState()
    assert np.array_equal(gm.getWellEfficiency(), e)
    again = assembled(gm, md)
    assert np.array_equal(again[0], want_d[0]) and np.array_equal(again[1], want_d[1])
    # a change of the solve's precision
    gm.setSolvePrecision(True)
    assert np.array_equal(gm.getWellEfficiency(), e)
    f32 = assembled(gm, md)
    assert np.array_equal(f32[0], want_f[0]) and np.array_equal(f32[1], want_f[1])
    gm.setSolvePrecision(False)
    # a re-plan: the same perforated cells registered as ONE group through opmgpu_set_wells rebuilds the structure under the device wells
    gm.setWells(np.array([0, wl.nperf], np.int32), wl.arrays()[1])
    assert np.array_equal(gm.getWellEfficiency(), e)
    replanned = assembled(gm, md)
    assert np.array_equal(replanned[0], want_d[0]) and np.array_equal(replanned[1], want_d[1])
    # a new well list: ones again
    md2 = W.DeviceWellModel(gm, _setup()[3], W.WellState(wl, st.p))
    assert np.array_equal(gm.getWellEfficiency(), np.ones(wl.nw))
    md2.prepareStep(2 * decks.DAY, st)
    reset = assembled(gm, md2)
    assert np.array_equal(reset[0], unit_d[0]) and np.array_equal(reset[1], unit_d[1])
    gm.close()


def test_setter_refusals(gpu_lib):
    grid, tab, st, wl = _setup()
    lib = gpu_lib
    gm = GpuBlackoilModel(grid, tab, capi.default_params())

    def refused(factors, text):
        f = None if factors is None else capi.f64(factors)
        assert lib.opmgpu_set_well_efficiency(gm.ctx, capi.dptr(f)) == capi.EINVAL, factors
        msg = lib.opmgpu_last_error(gm.ctx).decode()
        assert text in msg, (factors, msg)

    refused([0.5, 0.5], "no device wells")                     # before opmgpu_set_device_wells
    refused(None, "no device wells")
    out = np.zeros(2)
    assert lib.opmgpu_get_well_efficiency(gm.ctx, capi.dptr(out)) == capi.EINVAL and "no device wells" in lib.opmgpu_last_error(gm.ctx).decode()
    assert lib.opmgpu_set_well_efficiency(None, None) == capi.EINVAL
    with pytest.raises(ValueError, match="no device wells"):
        gm.setWellEfficiency([0.5, 0.5])
    W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    gm.setWellEfficiency([0.7, 0.6])
    refused([0.5, float("nan")], "not finite")
    refused([float("inf"), 0.5], "not finite")
    refused([0.0, 0.5], "outside (0, 1]")
    refused([0.5, -0.25], "outside (0, 1]")
    refused([1.0 + 2 ** -52, 0.5], "outside (0, 1]")
    assert lib.opmgpu_get_well_efficiency(gm.ctx, None) == capi.EINVAL
    with pytest.raises(ValueError, match="3 factors for 2 device wells"):
        gm.setWellEfficiency([0.5, 0.5, 0.5])
    assert np.array_equal(gm.getWellEfficiency(), [0.7, 0.6])              # a refused call changes nothing
    gm.setWellEfficiency([1.0, 2 ** -30])                                  # the ends of (0, 1] that are allowed
    assert np.array_equal(gm.getWellEfficiency(), [1.0, 2 ** -30])
    gm.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6: two ranks, one well each
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_assemble_the_single_domain_residual_with_factors(gpu_lib, tmp_path):
    """The owned cells' residual of a 2-rank run (injector with factor 0.5 on one rank, producer with 0.8 on the other) against the
    single-domain run, at the bound of tests/test_gpu_pvcdo.py::test_two_ranks_assemble_the_single_domain_residual: 1e-13 of the largest
    entry (two plans may sum a row's connections in different orders).  No well pre-solve: its stopping rule reads a global mean that the
    two runs sum in different orders."""
    import _wefac_dist_worker as wk
    from opmgpu import partition
    grid, tab, st = wk.base.deck(wk.CFG)

    def single(eff):
        gm = GpuBlackoilModel(grid, tab, wk.params())
        res = wk.owned_residual(gm, wk.wells(grid, eff), st, grid.nc)
        gm.close()
        return res

    want, unit = single(wk.EFF), single((1.0, 1.0))
    env = dict(os.environ, OPMGPU_COMM_TRANSPORT="shm")
    env["PYTHONPATH"] = os.path.join(ROOT, "opm-simulators-legacy_amd") + os.pathsep + env.get("PYTHONPATH", "")
    code = "from opmgpu import partition; print(partition.make_unique_id().hex())"
    uid = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
    world = 2
    outs = [str(tmp_path / ("r%d.npz" % r)) for r in range(world)]
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), uid, outs[r]], env=env, stdout=subprocess.PIPE,
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
    seen = np.zeros(grid.nc, bool)
    scale = np.abs(want).max()
    owners = {}
    wells_cells = np.asarray(wk.wells(grid).cells)
    for r, o in enumerate(outs):
        q = np.load(o)
        ids, res = q["ids"], q["residual"]
        for n, f in zip(q["names"].tolist(), q["eff"].tolist()):
            owners[n] = (r, f)
        err = np.abs(res - want[:, ids]).max()
        print("rank %d: owned residual against the single domain: %.3e of the largest entry" % (r, err / scale))
        assert err <= 1e-13 * scale
        mine = np.isin(ids, wells_cells)
        assert mine.any() and np.abs(res[:, mine] - unit[:, ids[mine]]).max() > 1e-6 * scale       # the rank did set its well's factor
        seen[ids] = True
    assert seen.all()
    assert owners["INJ"][1] == 0.5 and owners["PROD"][1] == 0.8 and owners["INJ"][0] != owners["PROD"][0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7: deck to file
# ---------------------------------------------------------------------------------------------------------------------------------------
def _summary(base):
    kws = wgn = None
    for k, _, v in eclio.read_arrays(base + ".SMSPEC"):
        if k.strip() == "KEYWORDS":
            kws = [str(x).strip() for x in v]
        if k.strip() == "WGNAMES":
            wgn = [str(x).strip() for x in v]
    rows = [np.asarray(v, float) for k, _, v in eclio.read_arrays(base + ".UNSMRY") if k.strip() == "PARAMS"]
    return [{(k, g): x for k, g, x in zip(kws, wgn, row)} for row in rows]


def test_deck_with_wefac_through_the_driver(gpu_lib, tmp_path):
    """WEFAC_SMALL.DATA (INJ 0.8 and PROD* 0.5 from the start, PROD1 0.9 from the second report step) through Simulator with device wells:
    at every report step FOPR = e WOPR(PROD1) and FWIR = e WWIR(INJ) with the step's factors -- to two float32 roundings, the file's
    precision: 2^-23 of the value -- and the W* vectors are the wells' own rates.  The same deck without WEFAC ends its first report step at
    other pressures: 20 % less water in and 50 % less oil out over ten days move a 90-cell model by bars; 0.1 bar is asked."""
    from opmgpu.simulator import Simulator
    prm = lambda: capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, tolerance_mb=1e-9, tolerance_cnv=1e-5, tolerance_wells=1e-8,      # noqa: E731
                                      linear_solver_reduction=1e-6, linear_solver_maxiter=200)
    base = str(tmp_path / "WEFAC")
    sim = Simulator(DECK, params=prm(), output_base=base)
    factors = [sim.schedule.wells(s).efficiency_factors().tolist() for s in range(3)]
    assert factors == [[0.8, 0.5], [0.8, 0.9], [0.8, 0.9]]
    sim.run(max_steps=1)
    p_with = sim.model.getState().p.copy()
    sim.close()
    sim = Simulator(DECK, params=prm(), output_base=base)
    reps = sim.run()
    sim.close()
    assert len(reps) == 3
    rows = _summary(base)
    assert len(rows) == 3
    f = ":+:+:+:+"
    for (e_inj, e_prod), row in zip(factors, rows):
        wopr, wwir = row[("WOPR", "PROD1")], row[("WWIR", "INJ")]
        assert wopr > 1.0 and wwir > 1.0
        assert abs(row[("FOPR", f)] - e_prod * wopr) <= 2.0 ** -23 * wopr, (row[("FOPR", f)], e_prod, wopr)
        assert abs(row[("FWPR", f)] - e_prod * row[("WWPR", "PROD1")]) <= 2.0 ** -23 * max(row[("WWPR", "PROD1")], 1e-30)
        assert abs(row[("FGPR", f)] - e_prod * row[("WGPR", "PROD1")]) <= 2.0 ** -23 * row[("WGPR", "PROD1")]
        assert abs(row[("FWIR", f)] - e_inj * wwir) <= 2.0 ** -23 * wwir
    assert rows[0][("WWIR", "INJ")] == pytest.approx(400.0, rel=1e-6)                # the injector's own rate is its target, whatever its uptime
    # the same deck without WEFAC
    src = open(DECK).read()
    plain = src.replace("WEFAC\n 'INJ'   0.8 /\n 'PROD*' 0.5 /\n/\n", "").replace("WEFAC\n 'PROD1' 0.9 /\n/\n", "")
    assert "WEFAC\n" not in plain.split("SCHEDULE\n")[1]
    path = str(tmp_path / "PLAIN.DATA")
    open(path, "w").write(plain)
    sim = Simulator(path, params=prm())
    sim.run(max_steps=1)
    p_plain = sim.model.getState().p
    sim.close()
    assert np.abs(p_with - p_plain).max() > 0.1 * decks.BAR, np.abs(p_with - p_plain).max() / decks.BAR
