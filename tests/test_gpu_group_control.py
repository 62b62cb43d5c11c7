"""GPU: group rate control shared by guide rates (opmgpu_set_well_groups, k_group_targets of csrc/wells.hip).  The sharing rule is stated in
include/opmgpu.h and restated in tests/group_reference.py.
  1 the kernel against the restatement on groups of 1, 63, 64, 65 and 257 wells; two calls give the same bits
  2 without groups nothing changes: never set = ngroups 0 = set and removed, bit for bit
  3 Newton parity with the reference subclass of the oracle's coupled model and with the host well model
  4 behaviour: the group meets its target, a well on its BHP limit leaves its share to the others, all wells BHP-bound
  5 the groups last through saved states, a change of precision and a re-plan; a new well list removes them; the refusals
  6 tests/golden/decks/GROUP_SMALL.DATA through the report-step driver, device wells and host wells"""
import types

import numpy as np
import pytest

from opmgpu import capi, decks, wells as W
from opmgpu.model import GpuBlackoilModel, NonlinearSolver
from group_reference import GroupOracleModel, arrays, slot_targets
from util import OracleBackend
import group_decks as G

pytestmark = pytest.mark.gpu

DAY = decks.DAY


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1: the kernel against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sizes(gpu_lib):
    """the 450-well case on the device: (case, reference targets, terms, reference group rates, [two reads of the device])"""
    case = G.sizes_case(0)
    grid, tab, wl, slot, current, qs, bhp, group_of_well = case
    gm = GpuBlackoilModel(grid, tab, capi.default_params())
    ws = W.WellState(wl, np.full(grid.nc, 250 * decks.BAR))
    md = W.DeviceWellModel(gm, wl, ws)
    assert gm.n_well_groups == len(G.SIZES) and md.shared_cells()[1] >= 3          # several wells per cell
    ws.current[:], ws.qs[:], ws.bhp[:] = current, qs, bhp
    md.push_well_state()
    reads = [gm.wellGroupTargets() for _ in range(2)]
    ref = slot_targets(wl.groups, slot, current, qs, wl.efficiency_factors())
    gm.close()
    return case, ref, reads


def test_kernel_matches_the_restatement_across_wave_and_block_sizes(sizes):
    """|device - restatement| <= 1e-12 * terms per target, terms = (gamma_w / Gamma_w) (T + sum |r_v|) / e_w: the device sums at most 257
    doubles per group (257 * 2^-53 = 3e-14 relative to the sum of the terms' magnitudes), the restatement sums exactly; what is left of
    the 1e-12 is a margin of about 30."""
    (grid, tab, wl, slot, current, qs, bhp, gow), (ref, terms, ref_rate), reads = sizes
    dev, rate = reads[0]
    assert [len(g.wells) for g in wl.groups] == list(G.SIZES)
    for g in wl.groups[3:]:                                 # members of one group with their slot at different indices
        assert {int(slot[w]) for w in g.wells} == {2, 3}
    on_slot = current == slot
    assert on_slot[gow == 0].all() and not on_slot[gow == 1].any()                  # I empty; C empty
    for g in (3, 4):
        assert on_slot[gow == g].any() and not on_slot[gow == g].all()
    e = wl.efficiency_factors()
    assert (e[gow == 4] < 1).sum() > 50 and (e[gow != 4] == 1).all()
    g2 = wl.groups[2]
    assert g2.sign == 1 and sum(qs[w, 0] for w in g2.wells if not on_slot[w]) > g2.target      # a negative remainder ...
    assert (ref[[w for w in g2.wells if on_slot[w]]] == 0).all() and on_slot[gow == 2].any()   # ... leaves the wells on the slot nothing
    assert np.isfinite(dev).all() and np.isfinite(ref).all()
    err = np.abs(dev - ref)
    worst = (err / terms).max()
    print("worst |device - restatement| / terms = %.2e; group rates %s" % (worst, np.abs(rate - ref_rate) / np.abs(ref_rate)))
    assert np.all(err <= 1e-12 * terms), worst
    assert (dev != 0).sum() > 300 and np.array_equal(np.sign(dev[dev != 0]), np.where(np.asarray(wl.type)[dev != 0] == W.PRODUCER, -1.0, 1.0))
    # the members' rate sum: the same bound against the sum of the magnitudes
    mags = np.asarray([sum(abs(e[w] * float(np.dot(g.distr, qs[w]))) for w in g.wells) for g in wl.groups])
    assert np.all(np.abs(rate - ref_rate) <= 1e-12 * mags)


def test_two_calls_give_the_same_bits(sizes):
    _, _, reads = sizes
    assert np.array_equal(reads[0][0], reads[1][0]) and np.array_equal(reads[0][1], reads[1][1])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2: nothing changes without groups
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("presolve", [1, 0])
def test_without_groups_every_path_keeps_its_bits(gpu_lib, presolve):
    """a wells deck whose producers carry a slot as last control: a context that never called the setter, one that called it with
    ngroups = 0, and one that set the group, let the kernel write the slots and removed the group again"""
    out = {}
    for how in ("never", "zero", "set and removed"):
        grid, tab, st, wl = G.field_deck()
        groups, wl.groups = wl.groups, []                    # DeviceWellModel installs no groups: the slots are plain rate limits
        gm = GpuBlackoilModel(grid, tab, capi.default_params(solve_welleq_initially=presolve))
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
        if how == "zero":
            assert gpu_lib.opmgpu_set_well_groups(gm.ctx, 0, None, None, None, None, None, None) == capi.OK
        elif how == "set and removed":
            gm.setWellGroups(groups)
            tg, _ = gm.wellGroupTargets()
            assert np.allclose(tg[:4] * DAY, [-40.0, -80.0, -120.0, -160.0], rtol=1e-13) and np.isnan(tg[4])
            gm.setWellGroups(None)
        md.prepareStep(2 * DAY, st)
        verdicts = []
        for it in range(2):
            gm.setSolvePrecision(False)
            gm.assemble(it == 0)
            verdicts.append((gm.getConvergence(), md.wellConvergence()))
            res, jac = gm.residual(), gm.jacobian()[2]
            dx = gm.solveJacobianSystem(want_dx=True, single_precision=False)
            gm.updateState()
        ws = md.pull_well_state()
        out[how] = (res, jac, dx, ws.bhp.copy(), ws.qs.copy(), ws.perf_rates.copy(), ws.perf_press.copy(), ws.current.copy(), gm.getState().p,
                    np.asarray(verdicts), np.asarray([md.presolve_iterations, md.presolve_converged]))
        gm.close()
    for how in ("zero", "set and removed"):
        for k, (a, b) in enumerate(zip(out["never"], out[how])):
            assert np.array_equal(a, b), (how, k)
    assert np.abs(out["never"][2]).max() > 0 and np.abs(out["never"][4]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3: Newton parity
# ---------------------------------------------------------------------------------------------------------------------------------------
PARITY = {
    # all four producers on their slot; well 3 cannot deliver its share above its BHP limit and hands it to the others
    "one_bhp": lambda: G.field_deck(bhp_limits_bar=(150, 150, 150, 248.5)),
    # one producer on GRUP, the others start on their own ORAT, which is below (well 3) or above their share; efficiency factors
    "mixed": lambda: G.field_deck(on_group=(0,), own_orat=150.0, eff=(1.0, 0.8, 1.0, 0.9)),
}


@pytest.mark.parametrize("cpr", [0, 1])
@pytest.mark.parametrize("presolve", [1, 0])
@pytest.mark.parametrize("name", sorted(PARITY))
def test_newton_parity_with_the_reference_and_the_host_model(gpu_lib, oracle, name, presolve, cpr):
    """Device wells under group control against (a) the group_reference subclass of the oracle's coupled model and (b) the host well model
    on the CPU oracle, Newton iteration by iteration until all three have converged; the tolerances are those of
    tests/test_gpu_wefac.py::test_newton_parity_with_the_reference_and_the_host_model.  The current controls agree at every iteration."""
    make = PARITY[name]
    grid, tab, st, wl_d = make()
    _, _, _, wl_h = make()
    _, _, _, wl_r = make()
    dt = 2 * DAY
    prm = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500, cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=cpr, solve_welleq_initially=presolve)
    prm_o = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=8000, solve_welleq_initially=presolve)
    gm = GpuBlackoilModel(grid, tab, prm)
    md = W.DeviceWellModel(gm, wl_d, W.WellState(wl_d, st.p))
    assert gm.n_well_groups == 1
    ob = OracleBackend(oracle, grid, tab, prm_o, wells=wl_h.arrays())
    mo = W.WellCoupledModel(ob, W.StandardWellsHost(wl_h, grid.z, tab.surface_density[0], solve_welleq_initially=bool(presolve)), W.WellState(wl_h, st.p))
    ref = GroupOracleModel(grid, tab, prm_o, wl_r, arrays(W.WellState(wl_r, st.p)), wl_r.groups, wl_r.efficiency_factors())
    md.prepareStep(dt, st); mo.prepareStep(dt, st); ref.prepareStep(dt, st)
    done = False
    for it in range(10):
        cd, _ = md.nonlinearIteration(it, single_precision=False)
        co, _ = mo.nonlinearIteration(it, single_precision=False)
        cr = ref.nonlinearIteration(it)
        assert cd == co == cr, it
        ws = md.pull_well_state()
        a = gm.getState()
        for tag, flux, ctrl, b, wsb, cnv in (("host", mo.wh.well_flux_residual, mo.wh.well_ctrl_residual, ob.getState(), mo.ws, ob.CNV),
                                             ("reference", ref.well_flux_residual, ref.well_ctrl_residual, ref.st, ref.ws, ref.CNV)):
            assert np.array_equal(ws.current, wsb.current), (tag, it, ws.current, wsb.current)
            assert np.allclose(md.well_flux_residual, flux, rtol=1e-5, atol=1e-12), (tag, it)
            assert md.well_ctrl_residual == pytest.approx(ctrl, rel=1e-5, abs=1e-12), (tag, it)
            assert np.array_equal(a.hc, b.hc), (tag, it)
            assert np.abs(a.p - b.p).max() <= 1e-6 * np.abs(b.p).max(), (tag, it)
            assert np.abs(a.sat - b.sat).max() <= 1e-6, (tag, it)
            assert np.allclose(ws.bhp, wsb.bhp, rtol=1e-7), (tag, it)
            assert np.allclose(ws.qs, wsb.qs, rtol=1e-6, atol=1e-9 * np.abs(wsb.qs).max()), (tag, it)
            assert np.allclose(ws.perf_rates, wsb.perf_rates, rtol=1e-6, atol=1e-9 * np.abs(wsb.perf_rates).max()), (tag, it)
            assert np.allclose(gm.CNV, cnv, rtol=1e-5, atol=1e-9), (tag, it)
        if cd and it >= 1:
            done = True
            break
    assert done
    slot = len(wl_d.controls[0]) - 1
    if name == "one_bhp":
        assert ws.current[:4].tolist() == [slot, slot, slot, 1]
    else:
        assert ws.current[:4].tolist() == [slot, slot, slot, 0]
    e = wl_d.efficiency_factors()
    assert abs((e[:4] * ws.qs[:4, 1]).sum() + wl_d.groups[0].target) <= prm.tolerance_well_control
    # the slot targets on the device are the restatement's for the state they were computed from
    tg, rate = gm.wellGroupTargets()
    want, terms, _ = slot_targets(wl_d.groups, [len(c) - 1 for c in wl_d.controls], ws.current, ws.qs, e)
    assert np.all(np.abs(tg[:4] - want[:4]) <= 1e-12 * terms[:4]) and np.isnan(tg[4])
    gm.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4: behaviour
# ---------------------------------------------------------------------------------------------------------------------------------------
def _converged(make, **prm_kw):
    grid, tab, st, wl = make()
    prm = capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, linear_solver_reduction=1e-8, linear_solver_maxiter=300, **prm_kw)
    gm = GpuBlackoilModel(grid, tab, prm)
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    md.prepareStep(2 * DAY, st)
    NonlinearSolver(max_iter=15).step(md, single_precision=False)
    ws = md.pull_well_state().copy()
    gm.close()
    g = wl.groups[0]
    e = wl.efficiency_factors()
    total = sum(e[w] * float(np.dot(g.distr, ws.qs[w])) for w in g.wells)
    slot = np.asarray([len(c) - 1 for c in wl.controls])
    return wl, g, ws, total, slot, prm.tolerance_well_control


def test_production_group_meets_its_target():
    wl, g, ws, total, slot, tol = _converged(lambda: G.field_deck(eff=(1.0, 0.7, 1.0, 0.9)))
    assert (ws.current[:4] == slot[:4]).all()
    assert abs(total + g.target) <= tol, (total * DAY, g.target * DAY)
    e = wl.efficiency_factors()
    share = np.asarray(g.guide) / sum(g.guide)
    assert np.allclose(e[:4] * ws.qs[:4, 1], -share * g.target, rtol=0, atol=tol)          # ... each well by its guide rate


def test_a_producer_on_its_bhp_limit_leaves_its_share_to_the_others():
    wl, g, ws, total, slot, tol = _converged(lambda: G.field_deck(bhp_limits_bar=(150, 150, 150, 248.5)))
    assert ws.current[:4].tolist() == [slot[0], slot[1], slot[2], 1] and ws.bhp[3] == 248.5 * decks.BAR
    assert abs(total + g.target) <= tol, (total * DAY, g.target * DAY)
    assert -ws.qs[3, 1] < 0.4 * g.target - 100 * tol                                        # less than its 4 / 10 ...
    rest = g.target + ws.qs[3, 1]
    assert np.allclose(ws.qs[:3, 1], -np.asarray([1.0, 2.0, 3.0]) / 6.0 * rest, rtol=0, atol=tol)      # ... the others share what it leaves 1 : 2 : 3


def test_all_producers_bhp_bound_stay_below_the_target():
    wl, g, ws, total, slot, tol = _converged(lambda: G.field_deck(target=4000.0, own_orat=3000.0, bhp_limits_bar=(240, 242, 244, 241)))
    assert ws.current[:4].tolist() == [1, 1, 1, 1] and (ws.current[:4] != slot[:4]).all()
    assert 0 < -total < g.target - 100 * tol, (total * DAY, g.target * DAY)


def test_injection_group_meets_its_target():
    wl, g, ws, total, slot, tol = _converged(lambda: G.inject_deck())
    assert (ws.current[:3] == slot[:3]).all() and abs(total - g.target) <= tol
    assert np.allclose(ws.qs[:3, 0], np.asarray([0.25, 0.25, 0.5]) * g.target, rtol=0, atol=tol)


def test_an_injector_on_its_bhp_limit_leaves_its_share_to_the_others():
    wl, g, ws, total, slot, tol = _converged(lambda: G.inject_deck(bhp_limits_bar=(400, 400, 253.0)))
    assert ws.current[:3].tolist() == [slot[0], slot[1], 1] and ws.bhp[2] == 253.0 * decks.BAR
    assert abs(total - g.target) <= tol and ws.qs[2, 0] < 0.5 * g.target - 100 * tol
    assert np.allclose(ws.qs[:2, 0], 0.5 * (g.target - ws.qs[2, 0]), rtol=0, atol=tol)


def test_presolve_forms_agree_under_groups(monkeypatch):
    """the unfused pre-solve (what groups take) and the one-workgroup serial form (OPMGPU_WELL_PRESOLVE_FUSED=2) re-share behind every
    iteration's control update with the same device function: the same bits"""
    out = []
    for mode in ("1", "0", "2"):
        monkeypatch.setenv("OPMGPU_WELL_PRESOLVE_FUSED", mode)
        grid, tab, st, wl = G.field_deck(bhp_limits_bar=(150, 150, 150, 248.5))
        gm = GpuBlackoilModel(grid, tab, capi.default_params())
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
        md.prepareStep(2 * DAY, st)
        gm.assemble(True)
        ws = md.pull_well_state()
        out.append((ws.qs.copy(), ws.bhp.copy(), ws.current.copy(), gm.wellGroupTargets()[0], md.presolve_iterations, md.presolve_converged, gm.residual()))
        gm.close()
    assert out[0][4] >= 2 and out[0][5]
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(a, b, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5: persistence and refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_groups_last_and_are_removed_by_a_new_well_list(gpu_lib):
    make = lambda: G.field_deck(bhp_limits_bar=(150, 150, 150, 248.5), eff=(1.0, 0.8, 1.0, 1.0))          # noqa: E731
    grid, tab, st, wl = make()
    prm = lambda: capi.default_params(solve_welleq_initially=0, linear_solver_reduction=1e-11, linear_solver_maxiter=500)          # noqa: E731  (no pre-solve: it would move the well state)

    def assembled(gm, md, single=False, targets=True):
        """one Newton step from the same start every time and the assembly behind it: the first assembly's cell rows do not see a target
        (without the pre-solve the rates follow the bhp alone), the second one's do"""
        md.push_well_state()
        md.prepareStep(2 * DAY, st)
        gm.setSolvePrecision(single)
        gm.assemble(True)
        gm.getConvergence()
        gm.solveJacobianSystem(single_precision=single)
        gm.updateState()
        gm.assemble(False)
        return (gm.residual(), gm.jacobian()[2]) + ((gm.wellGroupTargets()[0],) if targets else ())

    def same(a, b):
        return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))

    def fresh(single, with_groups=True):
        w2 = make()[3]
        if not with_groups:
            w2.groups = []
        gm = GpuBlackoilModel(grid, tab, prm())
        md = W.DeviceWellModel(gm, w2, W.WellState(w2, st.p))
        out = assembled(gm, md, single, targets=with_groups)
        gm.close()
        return out

    want_d, want_f, plain = fresh(False), fresh(True), fresh(False, with_groups=False)
    assert not np.array_equal(want_d[0], plain[0])
    gm = GpuBlackoilModel(grid, tab, prm())
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    assert same(assembled(gm, md), want_d)
    # saved states: the groups are no part of them
    gm.setWellGroups(None)
    gm.saveState()
    gm.setWellGroups(wl.groups)
    gm.restoreState()
    assert gm.n_well_groups == 1 and same(assembled(gm, md), want_d)
    # a change of the solve's precision
    assert same(assembled(gm, md, True), want_f)
    # A re-plan that changes the ORDERING cannot happen under device wells: rebuild_structure builds the pattern from the grid's
    # connections alone then (the wells are a factored operator, no clique fill) and hands it to the plan with the context's fixed
    # ilu_ordering, so the ordering is a function of the grid.  Asserted below; the groups hold well and control indices, no row.
    # A re-plan: the perforated cells registered as ONE group through opmgpu_set_wells rebuilds the structure under the device wells ...
    order0 = gm.ordering()[0].copy()
    gm.setWells(np.array([0, wl.nperf], np.int32), wl.arrays()[1])
    assert same(assembled(gm, md), want_d) and np.array_equal(gm.ordering()[0], order0)
    # ... and one that registers more cells behind them (another perforation table, the same ordering)
    extra = np.setdiff1d(np.arange(0, grid.nc, 7), wl.arrays()[1]).astype(np.int32)
    gm.setWells(np.array([0, wl.nperf, wl.nperf + extra.size], np.int32), np.concatenate([wl.arrays()[1], extra]))
    assert same(assembled(gm, md), want_d) and np.array_equal(gm.ordering()[0], order0)
    # a new well list: no groups
    w3 = make()[3]
    w3.groups = []
    W.DeviceWellModel(gm, w3, W.WellState(w3, st.p))
    assert gm.n_well_groups == 0 and np.isnan(gm.wellGroupTargets()[0]).all()
    gm.close()


def test_replacing_the_groups_gives_former_members_their_targets_back(gpu_lib):
    """a group of the producers 0..2 set in place of one of 0..3, whose slots the kernel had written: well 3, no member any more, has the
    target of its slot as it was given -- the context is the one that only ever had the smaller group, bit for bit"""
    out = []
    for replaced in (False, True):
        grid, tab, st, wl = G.field_deck()
        groups, wl.groups = wl.groups, []
        smaller = [W.WellGroup("SMALLER", -1, groups[0].target, (0, 1, 0), [0, 1, 2], [1.0, 2.0, 3.0])]
        gm = GpuBlackoilModel(grid, tab, capi.default_params(solve_welleq_initially=0))
        md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
        if replaced:
            gm.setWellGroups(groups)
            assert gm.wellGroupTargets()[0][3] * DAY == pytest.approx(-160.0)          # written into well 3's slot
        gm.setWellGroups(smaller)
        md.prepareStep(2 * DAY, st)
        gm.assemble(True)
        gm.getConvergence()
        md.wellConvergence()
        out.append((gm.residual(), md.well_flux_residual, np.float64(md.well_ctrl_residual), gm.wellGroupTargets()[0]))
        gm.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.isnan(out[0][3][3])


def test_groups_left_to_the_potentials_must_be_installed(gpu_lib):
    """a well list whose guide rates are left to the potentials, driven without the report-step driver: nothing runs until the groups are
    on the device (every member's slot would hold the whole group target otherwise)"""
    grid, tab, st, wl = G.field_deck(guide=(1.0, float("nan"), 3.0, 4.0))
    gm = GpuBlackoilModel(grid, tab, capi.default_params())
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    assert gm.n_well_groups == 0 and md.groups_pending
    with pytest.raises(ValueError, match="not installed"):
        md.prepareStep(2 * DAY, st)
    with pytest.raises(ValueError, match="not installed"):
        md.nonlinearIteration(0)
    gm.setState(st)
    assert md.install_groups(lambda: md.computeWellPotentials(grid.z, tab.surface_density[0])) and gm.n_well_groups == 1 and not md.groups_pending
    assert np.isfinite(wl.groups[0].guide[1]) and wl.groups[0].guide[1] > W.GUIDE_RATE_FLOOR
    md.prepareStep(2 * DAY, st)
    NonlinearSolver(max_iter=15).step(md, single_precision=False)
    gm.close()


def test_setter_refusals(gpu_lib):
    lib = gpu_lib
    grid, tab, st, wl = G.field_deck()
    groups, wl.groups = wl.groups, []
    g = groups[0]
    gm = GpuBlackoilModel(grid, tab, capi.default_params())

    def call(ptr, wells, sign, target, distr, guide):
        k = [capi.i32(ptr), capi.i32(wells), capi.f64(sign), capi.f64(target), capi.f64(distr), capi.f64(guide)]
        return lib.opmgpu_set_well_groups(gm.ctx, len(ptr) - 1, capi.iptr(k[0]), capi.iptr(k[1]), capi.dptr(k[2]), capi.dptr(k[3]), capi.dptr(k[4]), capi.dptr(k[5]))

    def refused(text, ptr=(0, 4), wells=(0, 1, 2, 3), sign=(-1.0,), target=(g.target,), distr=(0.0, 1.0, 0.0), guide=(1.0, 2.0, 3.0, 4.0)):
        assert call(ptr, wells, sign, target, distr, guide) == capi.EINVAL, text
        msg = lib.opmgpu_last_error(gm.ctx).decode()
        assert "opmgpu_set_well_groups" in msg and text in msg, (text, msg)

    refused("no device wells")
    assert lib.opmgpu_set_well_groups(gm.ctx, 0, None, None, None, None, None, None) == capi.EINVAL and "no device wells" in lib.opmgpu_last_error(gm.ctx).decode()
    out = np.zeros(8)
    assert lib.opmgpu_get_well_group_targets(gm.ctx, capi.dptr(out), None) == capi.EINVAL and "no device wells" in lib.opmgpu_last_error(gm.ctx).decode()
    assert lib.opmgpu_set_well_groups(None, 0, None, None, None, None, None, None) == capi.EINVAL
    with pytest.raises(ValueError, match="no device wells"):
        gm.setWellGroups(groups)
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    gm.setWellGroups(groups)
    before = gm.wellGroupTargets()[0]
    refused("well 1 is in two groups", ptr=(0, 2, 4), wells=(0, 1, 1, 2), sign=(-1.0, -1.0), target=(1.0, 1.0), distr=(0, 1, 0, 0, 1, 0))
    refused("the last control of well 4 is not a SURFACE_RATE slot with the distr of group 0", ptr=(0, 1), wells=(4,), guide=(1.0,))       # the injector: its last control is its BHP limit
    refused("the last control of well 0 is not a SURFACE_RATE slot with the distr of group 0", distr=(1.0, 1.0, 0.0))                       # an LRAT group over ORAT slots
    refused("the guide rate of well 2 is not positive", guide=(1.0, 2.0, 0.0, 4.0))
    refused("the guide rate of well 2 is not positive", guide=(1.0, 2.0, -3.0, 4.0))
    refused("the guide rate of well 3 is not finite", guide=(1.0, 2.0, 3.0, np.inf))
    refused("the guide rate of well 0 is not finite", guide=(np.nan, 2.0, 3.0, 4.0))
    refused("the target of group 0 is not finite", target=(np.nan,))
    refused("the target of group 0 is not finite", target=(np.inf,))
    refused("the target of group 0 is negative", target=(-1.0,))
    refused("names well 5, which does not exist", wells=(0, 1, 2, 5))
    # a refused call leaves the groups in force as they were
    assert gm.n_well_groups == 1 and np.array_equal(gm.wellGroupTargets()[0], before, equal_nan=True)
    with pytest.raises(ValueError, match="is negative"):
        gm.setWellGroups([types.SimpleNamespace(sign=-1.0, target=-2.0, distr=(0, 1, 0), wells=[0], guide=[1.0])])
    assert gm.n_well_groups == 1
    gm.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6: deck to file
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_golden_deck_through_the_driver_device_and_host(gpu_lib, oracle, tmp_path):
    """GROUP_SMALL.DATA (FIELD capped at 300 sm3/day of oil; P1 on GRUP, P2 / P3 on their own rates; P3's guide rate from the potentials),
    three report steps, with device wells and with the host well model on the CPU oracle: the field oil rate is the GCONPROD target at
    every report step, the GRUP well stays on its slot, and the two runs' summary and restart files agree under eclio.compare's defaults
    (the reference's regression tolerances).  The variant without GRUP (P1 on an oil rate of 200 sm3/day, 370 with the others) is
    capped too: before the reader knew GCONPROD it ran at 370 without a word, and the deck with GRUP did not run at all."""
    from opmgpu import eclio
    from opmgpu.simulator import Simulator
    import test_group_schedule as S
    tight = dict(tolerance_mb=1e-9, tolerance_cnv=1e-5, tolerance_wells=1e-7, linear_solver_reduction=1e-9, linear_solver_maxiter=400)

    def device_run(deck, base):
        sim = Simulator(deck, params=capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, **tight), output_base=base)
        sim.model.max_single_precision_days = 0.0            # double solves, like the oracle's
        currents = []
        make = W.DeviceWellModel

        models = []

        def device_wells(gm, wl, ws):
            md = make(gm, wl, ws, vfp_tables=sim.vfp_tables)
            models.append(md)
            currents.append(ws.current)          # the driver pulls the well state into this object at the end of the report step
            return md
        sim.well_model_factory = device_wells
        reps = sim.run()
        assert sim.model.n_well_groups == 1
        guide = [list(md.w.groups[0].guide) for md in models]
        sim.close()
        return reps, S._summary(base), [c.tolist() for c in currents], guide

    base_d, base_h = str(tmp_path / "DEV"), str(tmp_path / "HOST")
    rd, rows_d, cur_d, guide = device_run(S.DECK, base_d)
    rh, rows_h, cur_h = S.host_run(oracle, S.DECK, base_h)
    assert [r["days"] for r in rd] == [r["days"] for r in rh] == [10.0, 20.0, 40.0]
    for gd in guide:                                         # P3's guide rate came from the potentials, once per report step
        assert gd[:2] == [0.002, 0.004] and np.isfinite(gd[2]) and gd[2] > W.GUIDE_RATE_FLOOR
    for rows in (rows_d, rows_h):
        assert len(rows) == 3
        for row in rows:
            assert abs(row[("FOPR", S.F)] - 300.0) <= S.FOPR_TOL, row[("FOPR", S.F)]
            assert abs(row[("WOPR", "P1")] - 130.0) <= S.FOPR_TOL
    assert len(cur_d) == len(cur_h) == 3 and all(c[0] == 1 for c in cur_d + cur_h)      # at the end of every report step the GRUP well is on its slot (its last control)
    bad = eclio.compare(base_d, base_h)
    assert not bad, bad
    # the variant without GRUP
    path = S._variant(tmp_path, "'P1' 'OPEN' 'GRUP' 5* 150 /", "'P1' 'OPEN' 'ORAT' 200 4* 150 /")
    rv, rows_v, cur_v, _ = device_run(path, str(tmp_path / "VAR"))
    for row in rows_v:
        assert abs(row[("FOPR", S.F)] - 300.0) <= S.FOPR_TOL, row[("FOPR", S.F)]
        assert abs(row[("WOPR", "P2")] - 80.0) <= S.FOPR_TOL and abs(row[("WOPR", "P3")] - 90.0) <= S.FOPR_TOL
    assert len(cur_v) == 3 and all(c[0] == 2 for c in cur_v)


def test_groups_are_refused_in_a_decomposed_context(gpu_lib, monkeypatch):
    """a context with a communicator attached (the shared-memory test transport, one rank with one isolated ghost copy of cell 0): a group's
    wells may sit on several ranks, so the setter refuses -- and so does attaching a communicator to a context with groups"""
    from opmgpu import partition
    monkeypatch.setenv("OPMGPU_COMM_TRANSPORT", "shm")
    grid, tab, st, wl = G.field_deck()
    nc = grid.nc
    src = np.concatenate([np.arange(nc), [0]])
    grid_b = decks.GridData(nc + 1, grid.conn_cells, grid.trans, grid.pv[src], grid.z[src])

    class Dom:
        n_owned, neigh_rank, send_ptr, send_cells = nc, capi.i32([0]), capi.i32([0, 1]), capi.i32([0])
        recv_ptr, recv_cells = capi.i32([0, 1]), capi.i32([nc])

    groups, wl.groups = wl.groups, []
    gm = GpuBlackoilModel(grid_b, tab, capi.default_params())
    partition.attach_comm(gm, Dom, 0, 1, partition.make_unique_id())
    W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    with pytest.raises(ValueError, match="opmgpu_set_well_groups: a communicator is attached"):
        gm.setWellGroups(groups)
    gm.close()
    gm = GpuBlackoilModel(grid_b, tab, capi.default_params())
    W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    gm.setWellGroups(groups)
    before = gm.wellGroupTargets()
    with pytest.raises(Exception, match="controlled well groups are set"):
        partition.attach_comm(gm, Dom, 0, 1, partition.make_unique_id())
    # refused before anything is attached: the context is still single-domain -- the groups can be read, removed and set again (the
    # setter refuses a context with a communicator), and opmgpu_comm_set_pressure_hierarchy finds no communicator
    assert gpu_lib.opmgpu_comm_set_pressure_hierarchy(gm.ctx, 0) == capi.EINVAL
    after = gm.wellGroupTargets()
    assert np.array_equal(before[0], after[0], equal_nan=True) and np.array_equal(before[1], after[1])
    gm.setWellGroups(None)
    gm.setWellGroups(groups)
    assert gm.n_well_groups == 1 and np.array_equal(gm.wellGroupTargets()[0], before[0], equal_nan=True)
    gm.close()
