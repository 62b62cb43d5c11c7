"""The device well model (csrc/wells.hip, the wells' parts of csrc/linsolver.hip and csrc/amg.hip) past its fixed sizes: more than 128 and
more than 256 perforations in a well (the LDS tile of k_well_cdp, the second trip of every `j += 256` loop), more than 48, 64 and 256 wells
(the bordered pressure level, the 64-lane loops over wells, the form of the pre-solve), and the opt-in Woodbury correction of stage 2.
The decks are those of tests/well_size_decks.py; the references are the host well model (opmgpu/wells.py) on the CPU oracle, the second
restatement oracle/wells.py, and the float64 restatement of the pressure stage (tests/amg_reference.py).

  A  connection pressures of wells with 1 .. 320 perforations against both restatements
  B  two Newton iterations in lockstep with the oracle (util.lockstep_parity) on every deck, ILU0 and CPR, BiCGStab and GMRES
  C  the three forms of the pre-solve agree bit for bit, also above 256 wells (where only the two-launch form applies)
  D  the pressure stage with 48 wells (bordered) and with 49 (not bordered) against its restatement
  E  OPMGPU_WELL_WOODBURY=1 changes the preconditioner, not the Newton increment
  F  (no GPU) the decks are what A-E and G rely on
  G  the wells' convergence maxima as a decomposed run packs them on the device (k_well_conv_pack), with 257 and 300 wells

Measured on MI355X: 24 s for the module -- the lockstep cases 0.1 .. 1.1 s each (LONG the longest), the two Woodbury cases 5 s each (two
processes per case), everything else below 1 s; the guard F takes 10 s on the CPU.

Found by these tests and fixed with them: k_well_cdp took the total of a well's perforation rates at the top and reduced it on the way down,
which leaves rounding residue (1e-20) instead of the reference's exact 0.0 in the segments below the lowest flowing perforation; their
mixture was then that of the residue instead of the well's comp_frac.  LONG's producer without cross-flow (flowing perforations 96-119 of
320) had connection pressures off by up to 1.0e5 Pa (7.9e-2 of max |cdp|) below perforation 119."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import well_size_decks as D
from opmgpu import capi, decks, partition, wells as W
from opmgpu.model import GpuBlackoilModel
from util import lockstep_parity

HERE = os.path.dirname(os.path.abspath(__file__))


def _deck(name):
    return D.long_deck() if name == "long" else D.many_deck(int(name[4:]))


def _perf_well(wl):
    return np.repeat(np.arange(wl.nw), np.diff(np.asarray(wl.connpos)))


def _second_restatement_presolve(oracle, deck):
    """oracle/wells.py through control switching, connection pressures and the pre-solve of the first assembly (CoupledOracleModel.assemble
    without the linearisation against the cells, which this check does not need)"""
    from oracle import wells as OW
    w0 = W.WellState(deck.wl, deck.st.p)
    cm = OW.CoupledOracleModel(deck.grid, deck.tab, capi.default_params(), deck.wl, OW.WellStateArrays(w0.bhp, w0.qs, w0.perf_press, w0.perf_rates, w0.current))
    cm.prepareStep(deck.dt, deck.st)
    cm.update_well_controls()
    _, _, _, binv = oracle.assemble(deck.grid, deck.tab, deck.dt, deck.st, cm.rowptr, cm.col, scale=(1.0, 1.0, 1.0))
    cm.compute_connection_pressures()
    vals, _ = cm.perf_props(cm.st)
    assert cm.solve_well_eq(vals, binv.reshape(3, deck.grid.nc).mean(1))
    return cm


def _host_first_assembly(oracle, deck):
    mo = D.host_model(oracle, deck)
    mo.prepareStep(deck.dt, deck.st)
    mo.assemble(True)
    return mo


# n * eps of a 320-term sum is 4e-14; the remaining factor covers the density quotient of every term
CDP_TOL = 1e-12


# ---------------------------------------------------------------- A
@pytest.mark.gpu
def test_connection_pressures_of_long_wells(gpu_lib, oracle):
    """k_well_cdp on wells of 1, 64, 127, 128, 129, 255, 256, 257 and 320 perforations (one, two and three LDS tiles; a partial first tile in
    the reverse pre-pass): perf_press - bhp after the first assembly against the host well model AND against oracle/wells.py, which all sum
    in the reference's order in double."""
    deck = D.long_deck()
    wl = deck.wl
    gm = GpuBlackoilModel(deck.grid, deck.tab, capi.default_params())
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, deck.st.p))
    md.prepareStep(deck.dt, deck.st)
    gm.assemble(True)
    ws = md.pull_well_state()
    its = md.presolve_iterations
    assert md.presolve_converged
    cdp = ws.perf_press - ws.bhp[_perf_well(wl)]
    gm.close()
    mo = _host_first_assembly(oracle, deck)
    cm = _second_restatement_presolve(oracle, deck)
    assert its == mo.wh.well_iterations == cm.well_iterations
    scale = np.abs(mo.wh.cdp).max()
    cp = wl.connpos
    for name, ref in (("host", mo.wh.cdp), ("oracle/wells.py", cm.cdp)):
        worst = [float(np.abs(cdp[cp[w]:cp[w + 1]] - ref[cp[w]:cp[w + 1]]).max() / scale) for w in range(wl.nw)]
        print("cdp against %s, per well, relative to max |cdp| = %.3e Pa: %s" % (name, scale, " ".join("%.1e" % e for e in worst)))
    for name, ref in (("host", mo.wh.cdp), ("oracle/wells.py", cm.cdp)):
        assert np.abs(cdp - ref).max() <= CDP_TOL * scale, (name, np.abs(cdp - ref).max() / scale)
    assert scale > 5 * decks.BAR          # 160 m of wellbore


# ---------------------------------------------------------------- B
LOCKSTEP = [("long", 0, 0), ("long", 1, 0), ("long", 1, 1)] + [("many%d" % n, c, 0) for n in D.MANY_SIZES for c in (0, 1)] + [("many300", 1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,cpr,gmres", LOCKSTEP, ids=["%s-cpr%d-gmres%d" % c for c in LOCKSTEP])
def test_lockstep_parity_past_the_fixed_sizes(gpu_lib, oracle, name, cpr, gmres):
    """Residual, Jacobian, coupled operator (k_lowrank_reduce + lowrank_add against the explicit clique matrix), convergence scalars
    (the maxima over all wells of well_convergence()), pre-solve iteration count, current controls, well and reservoir state after the
    update (k_well_recover, k_well_update) of two Newton iterations, at the walker's own tolerances.
    (k_well_conv_pack packs the same maxima on the device only in a decomposed run: check G below.)"""
    deck = _deck(name)
    lockstep_parity(gpu_lib, oracle, deck.grid, deck.tab, deck.st, deck.dt, deck.wl, niter=2, cpr=cpr, gmres=gmres)


@pytest.mark.gpu
def test_lockstep_parity_of_long_wells_in_float(gpu_lib, oracle):
    """LONG with the float Jacobian and the float CPR solve, at the tolerances of the cart100_f32 entry of test_gpu_fullsize.TIMED_KW"""
    from test_gpu_fullsize import TIMED_KW
    deck = D.long_deck()
    lockstep_parity(gpu_lib, oracle, deck.grid, deck.tab, deck.st, deck.dt, deck.wl, niter=2, **TIMED_KW["cart100_f32"][1])


# ---------------------------------------------------------------- C
def _presolve_run(deck, monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("OPMGPU_WELL_PRESOLVE_FUSED", raising=False)
    else:
        monkeypatch.setenv("OPMGPU_WELL_PRESOLVE_FUSED", mode)
    gm = GpuBlackoilModel(deck.grid, deck.tab, capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=2000))
    md = W.DeviceWellModel(gm, deck.wl, W.WellState(deck.wl, deck.st.p))
    md.prepareStep(deck.dt, deck.st)
    md.nonlinearIteration(0, single_precision=False)
    ws = md.pull_well_state()
    assert md.presolve_converged
    out = (md.presolve_iterations, ws.current.copy(), ws.bhp.copy(), ws.qs.copy(), ws.perf_rates.copy(), ws.perf_press.copy(), gm.getState())
    gm.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,modes", [("long", ("1", "0", "2")), ("many65", ("1", "0", "2")), ("many257", (None, "1", "0"))])
def test_presolve_forms_agree_past_the_fixed_sizes(gpu_lib, oracle, monkeypatch, name, modes):
    """One fused launch, two launches per iteration and the single-workgroup fallback (OPMGPU_WELL_PRESOLVE_FUSED = 1, 0, 2) give the host's
    iteration count and the same controls, well state and reservoir state bit for bit.  With 257 wells (kFusedWells = 256) the library is
    written to take the two-launch form whatever the variable says; what is checked there is that the default, "1" and "0" agree bit for bit
    and take the host's iteration count -- which form ran is not observable through the C ABI."""
    deck = _deck(name)
    host_its = _host_first_assembly(oracle, deck).wh.well_iterations
    assert host_its >= 2
    out = {m: _presolve_run(deck, monkeypatch, m) for m in modes}
    a = out[modes[0]]
    assert a[0] == host_its, (a[0], host_its)
    for m in modes[1:]:
        b = out[m]
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), (m, a[0], b[0])
        assert all(np.array_equal(x, y) for x, y in zip(a[2:6], b[2:6])), m
        assert np.array_equal(a[6].p, b[6].p) and np.array_equal(a[6].sat, b[6].sat), m


# ---------------------------------------------------------------- D
# amg.hpp: the wells' unknowns are singleton rows on every level down to the coarsest, whose dense inverse holds at most 96 rows; a border
# is built only if the wells take at most half of them
BORDER_MAX_WELLS = 48


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [48, 49])
def test_pressure_stage_either_side_of_the_border_limit(gpu_lib, nw):
    """MANY(48): level 0 carries 48 border rows; MANY(49): none, the wells reach the pressure stage through their cells' diagonal only.
    Both hierarchies and cycles against the float64 restatement, as test_gpu_cpr_stages.test_b2_bordered_level0 does."""
    import amg_reference as ar
    from test_gpu_cpr_stages import check_hierarchy
    assert BORDER_MAX_WELLS == ar.DENSE_MAX // 2
    deck = D.many_deck(nw)
    gm = GpuBlackoilModel(deck.grid, deck.tab, capi.default_params(**dict(capi.CPR_AMG_VCYCLE, linear_solver_reduction=1e-6, linear_solver_maxiter=300)))
    md = W.DeviceWellModel(gm, deck.wl, W.WellState(deck.wl, deck.st.p))
    md.prepareStep(deck.dt, deck.st)
    _, lin = md.nonlinearIteration(0, single_precision=False)
    rowptr, col, val = gm.jacobian()
    n, _, nwb = gm.cpr_levels()
    print("many%d: %d border wells, levels %s, %d linear iterations to 1e-6" % (nw, nwb, list(n), lin))
    assert nwb == (nw if nw <= BORDER_MAX_WELLS else 0)
    assert n[0] == deck.grid.nc + nwb
    check_hierarchy(gm, rowptr, col, val, False, "sizes_many%d" % nw, seen={})          # not a case of that module's coverage table
    gm.close()


# ---------------------------------------------------------------- E
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["long", "many65"])
def test_woodbury_correction_leaves_the_newton_increment(gpu_lib, tmp_path, name):
    """OPMGPU_WELL_WOODBURY=1 (k_wb_setup / k_wb_apply: the wells' low-rank terms inside the second CPR stage, under GMRES) is a
    preconditioner only: at a 1e-10 reduction the increment equals the one without it to 1e-7 relative, the bound test_bicgstab_parity holds
    a double solve to.  The variable is read when the solver is set up: one process per setting (tests/_well_sizes_worker.py)."""
    res = {}
    for on in ("0", "1"):
        env = dict(os.environ, OPMGPU_WELL_WOODBURY=on)
        out = str(tmp_path / ("dx%s.npy" % on))
        p = subprocess.run([sys.executable, os.path.join(HERE, "_well_sizes_worker.py"), name, out], env=env, cwd=os.path.dirname(HERE),
                           capture_output=True, text=True, timeout=240)
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139):          # the worker died: nothing more is started on that device
            pytest.exit("worker %s OPMGPU_WELL_WOODBURY=%s ended with %d: %s" % (name, on, p.returncode, p.stderr[-2000:]), returncode=3)
        assert p.returncode == 0, (name, on, p.returncode, p.stdout[-3000:], p.stderr[-3000:])
        res[on] = (json.loads(p.stdout.strip().splitlines()[-1]), np.load(out))
    (off, x_off), (on, x_on) = res["0"], res["1"]
    print("%s: linear iterations without / with the correction %d / %d, reductions %.1e / %.1e" % (name, off["iterations"], on["iterations"], off["reduction"], on["reduction"]))
    assert off["woodbury"] == 0 and on["woodbury"] == 1
    assert off["reduction"] <= 1e-10 and on["reduction"] <= 1e-10
    # the variable took effect: another preconditioner gives another Krylov path, so the two increments cannot be the same bit for bit
    assert not np.array_equal(x_on, x_off)
    nc = x_off.size // 3
    for a in range(3):
        blk = slice(a * nc, (a + 1) * nc)
        assert np.abs(x_on[blk] - x_off[blk]).max() <= 1e-7 * np.abs(x_off[blk]).max(), (a, np.abs(x_on[blk] - x_off[blk]).max() / np.abs(x_off[blk]).max())


# ---------------------------------------------------------------- G
def _displaced_start(deck):
    """MANY's start state with the LAST well on its liquid-rate control at rates that satisfy neither that control nor its flux equations
    (a two-phase rate control does not seed the rates): without the pre-solve the assembled system of iteration 0 then has its largest
    flux-equation AND a control-equation residual far from zero in that well"""
    ws = W.WellState(deck.wl, deck.st.p)
    last = deck.wl.nw - 1
    ws.current[last] = 1
    ws.qs[last] = [-2e-4, -3e-4, -1e-2]
    return ws


def _host_residuals(oracle, deck, presolve):
    """|flux equations| [nw, 3] weighted with B_avg, |control equations| [nw] and the model, of the host's first assembly"""
    from util import OracleBackend
    ob = OracleBackend(oracle, deck.grid, deck.tab, capi.default_params(), wells=deck.wl.arrays())
    wh = W.StandardWellsHost(deck.wl, deck.grid.z, deck.tab.surface_density[0], solve_welleq_initially=presolve)
    mo = W.WellCoupledModel(ob, wh, W.WellState(deck.wl, deck.st.p) if presolve else _displaced_start(deck))
    mo.prepareStep(deck.dt, deck.st)
    mo.assemble(True)
    ob.getConvergence()
    wh.converged(ob.B_avg)
    return np.abs(wh.flux_eq) * np.asarray(ob.B_avg), np.abs(wh.ctrl_eq), mo


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [257, 300])
def test_well_convergence_maxima_of_a_decomposed_run(gpu_lib, oracle, nw):
    """In a decomposed run the maxima of the well equations' residuals are packed on the device (k_well_conv_pack, one workgroup of 256
    threads striding over the wells) and ride on the convergence all-reduce; a single-domain run takes them in a host loop instead.  MANY(257)
    and MANY(300) as a ONE-rank decomposition (a communicator to itself and one isolated ghost copy of cell 0, which changes no owned
    equation): well_flux_residual and well_ctrl_residual of the first assembly against the host model on the oracle at the walker's
    tolerances (rtol 1e-7), with the pre-solve and -- for a control-equation residual that is not zero -- without it from a displaced state.
    In both the extreme residuals belong to the last well (index >= 256)."""
    deck = D.many_deck(nw)
    g, st, nc, last = deck.grid, deck.st, deck.grid.nc, nw - 1
    src = np.concatenate([np.arange(nc), [0]])
    grid_b = decks.GridData(nc + 1, g.conn_cells, g.trans, g.pv[src], g.z[src])
    st_b = decks.State(st.p[src], st.sat[src], st.rs[src], st.rv[src], st.hc[src])

    class Dom:
        n_owned, neigh_rank, send_ptr, send_cells = nc, capi.i32([0]), capi.i32([0, 1]), capi.i32([0])
        recv_ptr, recv_cells = capi.i32([0, 1]), capi.i32([nc])

    for presolve in (True, False):
        flux, ctrl, mo = _host_residuals(oracle, deck, presolve)
        assert int(np.argmax(flux.max(1))) == last >= 256 and flux.max() > 1e-6
        if not presolve:
            assert int(np.argmax(ctrl)) == last and ctrl[last] > 1e-5 and np.delete(ctrl, last).max() < 1e-12
        gm = GpuBlackoilModel(grid_b, deck.tab, capi.default_params(solve_welleq_initially=int(presolve)))
        partition.attach_comm(gm, Dom, 0, 1, partition.make_unique_id())
        md = W.DeviceWellModel(gm, deck.wl, W.WellState(deck.wl, st.p) if presolve else _displaced_start(deck))
        md.prepareStep(deck.dt, st_b)
        gm.setSolvePrecision(False)
        gm.assemble(True)
        gm.getConvergence()
        md.wellConvergence()
        got_flux, got_ctrl = np.array(md.well_flux_residual), md.well_ctrl_residual
        ws = md.pull_well_state()
        gm.close()
        print("many%d, pre-solve %d: flux residuals %s (host %s), control residual %.6e (host %.6e)" % (nw, presolve, got_flux, mo.wh.well_flux_residual, got_ctrl, mo.wh.well_ctrl_residual))
        if presolve:
            assert md.presolve_converged and md.presolve_iterations == mo.wh.well_iterations
        assert np.array_equal(ws.current, mo.ws.current)
        assert np.allclose(got_flux, mo.wh.well_flux_residual, rtol=1e-7, atol=1e-14), (presolve, got_flux, mo.wh.well_flux_residual)
        assert got_ctrl == pytest.approx(mo.wh.well_ctrl_residual, rel=1e-7, abs=1e-14), (presolve, got_ctrl, mo.wh.well_ctrl_residual)


# ---------------------------------------------------------------- F (no GPU)
def test_the_cases_are_what_they_claim(oracle):
    """Every deck on the CPU, with the host well model on the oracle backend: the perforation counts; the cross-flow pattern of the two wells
    without cross-flow; the LAST well of MANY(nw) has the largest flux-equation and control-equation residuals and is the one that switches
    control in the pre-solve; at least two pre-solve iterations; host model and oracle get through two Newton iterations by themselves; and
    the two restatements agree on the connection pressures of LONG at the bound of check A."""
    deck = D.long_deck()
    wl, cp = deck.wl, deck.wl.connpos
    tr = D.host_trace(oracle, deck, newton=True)
    assert tuple(tr["perforations"]) == D.LONG_COUNTS == (1, 64, 127, 128, 129, 255, 256, 257, 320)
    assert {wl.controls[w][0][0] for w in range(wl.nw)} == {W.BHP, W.SURFACE_RATE} and set(wl.type) == {W.INJECTOR, W.PRODUCER}
    assert [w for w in range(wl.nw) if not wl.allow_cf[w]] == [7, 8]
    neg7 = np.flatnonzero(tr["drawdown"][cp[7]:cp[8]] < 0)
    assert wl.type[7] == W.INJECTOR and neg7.tolist() == [256]                       # the minority sign at index >= 256 only
    pos8 = np.flatnonzero(tr["drawdown"][cp[8]:cp[9]] >= 0)
    assert wl.type[8] == W.PRODUCER and pos8.tolist() == list(D.CF_WELLS[8][1]) and pos8.max() < 128 and 0 < pos8.size < 160
    assert tr["presolve_iterations"] >= 2 and tr["presolve_switches"] and tr["newton_ok"]
    cm = _second_restatement_presolve(oracle, deck)
    mo = _host_first_assembly(oracle, deck)
    assert cm.well_iterations == mo.wh.well_iterations == tr["presolve_iterations"]
    assert np.abs(cm.cdp - mo.wh.cdp).max() <= CDP_TOL * np.abs(mo.wh.cdp).max()
    for nw in D.MANY_SIZES:
        tr = D.host_trace(oracle, D.many_deck(nw), newton=True)
        assert tr["nw"] == nw and set(tr["perforations"]) == {2}
        last = nw - 1
        assert last >= D.TAIL_START.get(nw, 0)
        assert tr["presolve_iterations"] >= 2 and tr["presolve_switches"] == [last], (nw, tr["presolve_switches"])
        assert tr["flux_argmax"] == last and tr["first_flux_argmax"] == last, (nw, tr["flux_argmax"], tr["first_flux_argmax"])
        assert tr["ctrl_argmax"] == last and tr["ctrl_max"] > 1e-3, (nw, tr["ctrl_argmax"], tr["ctrl_max"])
        assert max(tr["flux_max"]) > 1e-6          # far above the absolute floor of the walker's comparison (1e-14)
        assert tr["newton_ok"] and not tr["converged0"]
    assert D.TAIL_START == {65: 64, 257: 256, 300: 256}
    for nw in (257, 300):          # check G's second leg: no pre-solve, the last well displaced
        flux, ctrl, _ = _host_residuals(oracle, D.many_deck(nw), False)
        assert int(np.argmax(flux.max(1))) == nw - 1 and int(np.argmax(ctrl)) == nw - 1 and ctrl[nw - 1] > 1e-5 and np.delete(ctrl, nw - 1).max() < 1e-12
