"""GPU: oil-water decks (opmgpu_tables.active_phases = OPMGPU_PHASES_OIL_WATER) against the CPU oracle on the three-phase twin
(tests/twophase.py; the twin is pinned on the oracle itself in test_twophase_twin.py).  Water / oil quantities are compared at the
tolerances the three-phase tests use against the same oracle; what concerns the pinned gas unknown is compared EXACTLY: identity gas
row, zero third column, zero gas residual, zero gas CPR weight, and the third plane of every solve's dx == 0.0 bit for bit."""
import ctypes as C

import numpy as np
import pytest

from opmgpu import capi, decks, wells as W
from opmgpu.model import GpuBlackoilModel
from util import OracleBackend, perforated_diag_mask, rel_err

import twophase as tp

pytestmark = pytest.mark.gpu

RTOL, ATOL_REL = 1e-11, 1e-13          # eval_cell outputs: tests/test_gpu_simulator_data.py, tests/test_gpu_stone.py
RTOL_JAC = 1e-11                       # Jacobian blocks / residual: tests/test_gpu_assembly.py
DT = 5 * decks.DAY


def _close(got, ref, rtol=RTOL):
    return np.allclose(got, ref, rtol=rtol, atol=ATOL_REL * np.abs(ref).max())


def _prop(oracle, props, name, k=0):
    return props[:, oracle.PROP_NAMES.index(name), k]


def _create(g, t, prm=None):
    """(status, text of opmgpu_last_error(NULL)) of opmgpu_create; a context that came to life is destroyed again"""
    lib = capi.load()
    ctx = C.c_void_p()
    prm = prm or capi.default_params()
    st = lib.opmgpu_create(C.byref(ctx), 0, C.byref(g.struct()), C.byref(t.struct()), C.byref(prm))
    why = lib.opmgpu_last_error(None)
    if ctx:
        lib.opmgpu_destroy(ctx)
    return st, (why or b"").decode()


# ---------------------------------------------------------------------------------------------------------------------------------------
# G1: cell properties
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("endpoints", [False, True])
def test_cell_properties_match_the_twin(gpu_lib, oracle, endpoints):
    g = tp.grid(5, 7, 9, endpoints=endpoints, vertical=endpoints)
    st = tp.state(g)
    props = oracle.cell_props(g, tp.twin_tables(), st)
    cells = np.arange(0, g.nc, 3, dtype=np.int32)
    m = GpuBlackoilModel(g, tp.tables(), wells=(np.array([0, cells.size], np.int32), cells))
    m.setState(st)
    sd = m.simulatorData()
    pp = m.perfProps(cells.size).reshape(cells.size, 9, 4)
    got = m.getState()
    m.close()
    for ph, (b, den, mu, kr) in zip("wo", (("1OVERBW", "WAT_DEN", "WAT_VISC", "WATKR"), ("1OVERBO", "OIL_DEN", "OIL_VISC", "OILKR"))):
        assert _close(sd[b], _prop(oracle, props, "b_" + ph)), ph
        assert _close(sd[den], _prop(oracle, props, "rho_" + ph)), ph
        assert _close(sd[mu], _prop(oracle, props, "mu_" + ph)), ph
        assert _close(sd[kr], _prop(oracle, props, "kr_" + ph)), ph
    # the inactive gas phase: b = 1, rho = 0, mu = 1, kr = 0; nothing dissolved, no saturation pressures
    assert np.all(sd["1OVERBG"] == 1.0) and np.all(sd["GAS_DEN"] == 0.0) and np.all(sd["GAS_VISC"] == 1.0) and np.all(sd["GASKR"] == 0.0)
    for name in ("RSSAT", "RVSAT", "PBUB", "PDEW"):
        assert np.all(sd[name] == 0.0), name
    # perforation properties [p, rs, rv, b_w, b_o, b_g, mob_w, mob_o, mob_g] x [value, d/dp, d/dSw, d/dXvar]
    assert np.array_equal(pp[:, 0, 0], st.p[cells]) and np.all(pp[:, 1:3] == 0.0)
    for k, name in ((3, "b_w"), (4, "b_o"), (6, "mob_w"), (7, "mob_o")):
        ref = props[cells, oracle.PROP_NAMES.index(name)]
        assert _close(pp[:, k, 0], ref[:, 0]), name
        assert _close(pp[:, k, 1], ref[:, 1], 1e-9) and _close(pp[:, k, 2], ref[:, 2], 1e-9), name          # derivatives: RTOL_D of test_gpu_stone.py
        assert np.all(pp[:, k, 3] == 0.0), name                                                              # nothing depends on the dummy unknown
    assert np.array_equal(pp[:, 5], np.tile([1.0, 0.0, 0.0, 0.0], (cells.size, 1))) and np.all(pp[:, 8] == 0.0)
    # the state: Sg = rs = rv = 0, hc reported as GAS_AND_OIL
    assert np.all(got.sat[:, 2] == 0.0) and np.all(got.rs == 0.0) and np.all(got.rv == 0.0) and np.all(got.hc == capi.HC_GAS_AND_OIL)
    assert np.array_equal(got.p, st.p) and np.array_equal(got.sat[:, :2], st.sat[:, :2])


def test_state_gas_entries_are_ignored_on_input(gpu_lib):
    g = tp.grid(5, 7, 9)
    st = tp.state(g)
    st.sat[:, 2] = 0.1; st.rs[:] = 50.0; st.rv[:] = 1e-4; st.hc[:] = capi.HC_OIL_ONLY
    m = GpuBlackoilModel(g, tp.tables())
    m.setState(st)
    got = m.getState()
    m.close()
    assert np.all(got.sat[:, 2] == 0.0) and np.all(got.rs == 0.0) and np.all(got.rv == 0.0) and np.all(got.hc == capi.HC_GAS_AND_OIL)


# ---------------------------------------------------------------------------------------------------------------------------------------
# G2: one assembly
# ---------------------------------------------------------------------------------------------------------------------------------------
def _check_assembly(oracle, m, g, twin, st, dt, accum0, rowptr, col, scale, tol_jac):
    """residual and Jacobian of the resident assembly against the oracle's twin assembly; returns the oracle's accum0"""
    nc = g.nc
    r, val, accum0, _ = oracle.assemble(g, twin, dt, st, rowptr, col, scale=tuple(scale), accum0=accum0)
    gr, gc, gv = m.jacobian()
    assert np.array_equal(gr, rowptr) and np.array_equal(gc, col)
    gv, val = gv.reshape(-1, 3, 3), val.reshape(-1, 3, 3)
    res = m.residual()
    assert rel_err(res[:2 * nc], r[:2 * nc]) < RTOL_JAC, rel_err(res[:2 * nc], r[:2 * nc])
    assert rel_err(gv[:, :2, :2], val[:, :2, :2]) < tol_jac, rel_err(gv[:, :2, :2], val[:, :2, :2])
    diag = np.repeat(np.arange(nc), np.diff(rowptr)) == col
    assert np.all(res[2 * nc:] == 0.0)                                                    # gas residual
    assert np.all(gv[:, :2, 2] == 0.0)                                                    # third column of the water / oil rows
    assert np.all(gv[~diag][:, 2, :] == 0.0)                                              # gas row off the diagonal
    assert np.array_equal(gv[diag][:, 2, :], np.tile([0.0, 0.0, 1.0], (nc, 1)))           # identity on it, whatever matbalscale[2]
    return accum0


@pytest.mark.parametrize("variant", ["plain", "endpoints", "threepoint_thpres"])
@pytest.mark.parametrize("single", [False, True])
def test_assembly_matches_the_twin(gpu_lib, oracle, variant, single):
    g = tp.grid(9, 8, 9, endpoints=variant != "plain", vertical=variant != "plain", scalecrs=variant == "threepoint_thpres",
                thpres=variant == "threepoint_thpres")
    two, twin = tp.tables(), tp.twin_tables()
    st = tp.state(g)
    prm = capi.default_params(use_cpr=1, cpr_use_amg=1, cpr_max_ell_iter=0, linear_solver_reduction=1e-8, linear_solver_maxiter=400)
    scale = np.asarray(prm.matbalscale[:])
    rowptr, col = oracle.pattern(g)
    m = GpuBlackoilModel(g, two, prm)
    m.prepareStep(DT, st)
    m.setSolvePrecision(single)
    m.assemble(True)
    tol = 2e-6 if single else RTOL_JAC                                                    # a float Jacobian: test_gpu_assembly.py's figure
    acc = _check_assembly(oracle, m, g, twin, st, DT, None, rowptr, col, scale, tol)
    # the CPR weights of this matrix: no gas weight
    w = np.zeros(3 * g.nc)
    m.getConvergence()
    dx = m.solveJacobianSystem(want_dx=True, single_precision=single)
    assert m.lib.opmgpu_get_cpr_weights(m.ctx, capi.dptr(w)) == capi.OK
    w = w.reshape(3, g.nc)
    assert np.all(w[2] == 0.0) and np.all(w[:2].sum(0) >= 1.0)
    assert np.all(dx[2 * g.nc:] == 0.0) and np.abs(dx[:g.nc]).max() > 0.0
    # a second assembly of a moved state against the stored accumulation term
    m.updateState()
    st1 = m.getState()
    assert np.all(st1.sat[:, 2] == 0.0) and np.all(st1.rs == 0.0) and np.all(st1.rv == 0.0) and np.all(st1.hc == capi.HC_GAS_AND_OIL)
    assert np.abs(st1.sat[:, 0] - st.sat[:, 0]).max() > 1e-4 and np.abs(st1.p - st.p).max() > 0.0        # the state moved
    # (the twin's range of validity: a cell the update took closer to connate water than 1e-3 is put back there, so the check always runs)
    st1.sat[:, 0] = np.maximum(st1.sat[:, 0], tp.connate(g) + 1e-3); st1.sat[:, 1] = 1.0 - st1.sat[:, 0]
    m.setState(st1)
    m.assemble(False)
    _check_assembly(oracle, m, g, twin, st1, DT, acc, rowptr, col, scale, tol)
    m.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# G3: the connate region, where the twin is NOT the yardstick: kro = krow(Sw), the plain table column, constant below its first node
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_kro_near_connate_water_is_the_krow_column(gpu_lib):
    g = tp.grid(5, 7, 9)
    st = tp.state(g)
    swco = tp.connate(g)
    n = g.nc
    kind = np.arange(n) % 4                      # 0: Sw = Swco, 1: Sw < Swco, 2: Sw = Swco + 5e-6 (inside the default law's blend), 3: as drawn
    st.sat[kind == 0, 0] = swco[kind == 0]
    st.sat[kind == 1, 0] = swco[kind == 1] - 0.03
    st.sat[kind == 2, 0] = swco[kind == 2] + 5e-6
    st.sat[:, 1] = 1.0 - st.sat[:, 0]
    cells = np.arange(n, dtype=np.int32)
    m = GpuBlackoilModel(g, tp.tables(), wells=(np.array([0, n], np.int32), cells))
    m.setState(st)
    sd = m.simulatorData()
    pp = m.perfProps(n).reshape(n, 9, 4)
    m.close()
    kro, slope = np.empty(n), np.empty(n)
    for c in range(n):
        t = np.array(tp.SWOF[g.satnum[c]])
        sw = st.sat[c, 0]
        kro[c] = np.interp(sw, t[:, 0], t[:, 2])
        # slope of the segment x[i] < Sw <= x[i+1] (SWOF is searched from the left); 0 at and beyond the table's ends
        i = np.searchsorted(t[:, 0], sw, side="left") - 1
        slope[c] = 0.0 if sw <= t[0, 0] or sw >= t[-1, 0] else (t[i + 1, 2] - t[i, 2]) / (t[i + 1, 0] - t[i, 0])
    assert _close(sd["OILKR"], kro)
    mu_o = sd["OIL_VISC"]
    assert _close(pp[:, 7, 0] * mu_o, kro, 1e-9)                      # mobility x viscosity: RTOL_D of test_gpu_stone.py
    assert _close(pp[:, 7, 2] * mu_o, slope, 1e-9)                    # d mob_o / d Sw = kro' / mu_o (mu_o does not depend on Sw)
    assert np.all(slope[kind <= 1] == 0.0) and np.all(slope[kind == 2] < 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# G5: refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def _bare(**over):
    """a two-phase FluidTables whose struct is then bent into a refused combination"""
    t = tp.tables()
    s = t.struct()
    for k, v in over.items():
        setattr(s, k, v)
    return t


def test_refusals_at_creation(gpu_lib):
    g = tp.grid(5, 7, 9)
    cases = {"has_disgas": _bare(has_disgas=1), "has_vapoil": _bare(has_vapoil=1), "vap1": _bare(vap1=0.5), "vap2": _bare(vap2=0.5),
             "threephase_model": _bare(threephase_model=capi.KRO_STONE2), "active_phases": _bare(active_phases=2)}
    for word, t in cases.items():
        st, why = _create(g, t)
        assert st == capi.EINVAL and why and word.split("_")[-1] in why, (word, st, why)
    gh = decks.GridData(g.nc, g.conn_cells, g.trans, g.pv, g.z, pvtnum=g.pvtnum, satnum=g.satnum, imbnum=g.satnum)
    st, why = _create(gh, tp.tables())
    assert st == capi.EINVAL and "hysteresis" in why
    # a three-phase context created afterwards works, and so does a two-phase one
    assert _create(g, tp.twin_tables())[0] == capi.OK
    assert _create(g, tp.tables())[0] == capi.OK


def _wells(g, kind):
    nx, ny, nz = g.dims
    colm = lambda i, j: [i + nx * j + nx * ny * k for k in range(nz)]
    WI = 5.0 * float(np.median(g.trans))
    wl = W.Wells()
    inj = (0.0, 0.0, 1.0) if kind == "gas_injector" else (1.0, 0.0, 0.0)
    wl.add_well("INJ", W.INJECTOR, g.z[colm(0, 0)[0]], colm(0, 0), WI, inj, (W.SURFACE_RATE, 30.0 / 86400.0, inj), limits=[(W.BHP, 600 * decks.BAR)])
    if kind == "grat":
        ctrl, limits = (W.SURFACE_RATE, -20.0 / 86400.0, (0.0, 0.0, 1.0)), [(W.BHP, 100 * decks.BAR)]
    elif kind == "grat_limit":
        ctrl, limits = (W.BHP, 150 * decks.BAR), [(W.SURFACE_RATE, -20.0 / 86400.0, (0.0, 1.0, 1.0))]
    elif kind == "thp":
        ctrl, limits = (W.BHP, 150 * decks.BAR), [(W.THP, 20 * decks.BAR, None, 1, 0.0)]
    else:
        ctrl, limits = (W.BHP, 150 * decks.BAR), []
    wl.add_well("P1", W.PRODUCER, g.z[colm(nx - 1, ny - 1)[0]], colm(nx - 1, ny - 1)[:4], WI, (0.0, 1.0, 0.0), ctrl, limits=limits)
    if kind == "lockstep":       # a producer on ORAT whose BHP limit breaks at once: it switches to BHP
        wl.add_well("P2", W.PRODUCER, g.z[colm(nx - 1, 0)[0]], colm(nx - 1, 0), WI, (0.0, 1.0, 0.0), (W.SURFACE_RATE, -400.0 / 86400.0, (0.0, 1.0, 0.0)),
                    limits=[(W.BHP, 120 * decks.BAR)])
    return wl


@pytest.mark.parametrize("kind", ["gas_injector", "grat", "grat_limit", "thp"])
def test_refusals_at_well_setup(gpu_lib, kind):
    g = tp.grid(5, 7, 9)
    st = tp.state(g)
    m = GpuBlackoilModel(g, tp.tables())
    with pytest.raises(ValueError, match="without a gas phase"):            # OPMGPU_EINVAL with the text of opmgpu_last_error(ctx)
        W.DeviceWellModel(m, _wells(g, kind), W.WellState(_wells(g, kind), st.p))
    m.close()
    # the same wells on the three-phase twin are accepted (THP needs its VFP table: not that one)
    if kind != "thp":
        m3 = GpuBlackoilModel(g, tp.twin_tables())
        W.DeviceWellModel(m3, _wells(g, kind), W.WellState(_wells(g, kind), st.p))
        m3.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# G7: fluid in place
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_fluid_in_place_matches_the_twin(gpu_lib, oracle):
    g = tp.grid(5, 7, 9)
    st = tp.state(g)
    fipnum = (1 + np.arange(g.nc) % 3).astype(np.int32)
    fipnum[::17] = 0                                              # cells outside every region
    ob = OracleBackend(oracle, g, tp.twin_tables(), capi.default_params())
    ob.prepareStep(DT, st)
    vo, co = ob.computeFluidInPlace(fipnum, cells=True)
    m = GpuBlackoilModel(g, tp.tables())
    m.setState(st)
    vg, cg = m.computeFluidInPlace(fipnum, cells=True)
    m.close()
    for k in (0, 1, 5, 6):                                        # water, oil, pore volume, hydrocarbon-pv weighted pressure
        assert np.allclose(vg[:, k], vo[:, k], rtol=1e-12), k
        assert np.allclose(cg[k], co[k], rtol=1e-12, atol=1e-13 * np.abs(co[k]).max()), k
    assert np.all(vg[:, 2:5] == 0.0) and np.all(cg[2:5] == 0.0)   # gas, dissolved gas, vaporised oil


def test_voidage_coefficients_and_perforation_pvt_without_gas(gpu_lib, oracle):
    g = tp.grid(5, 7, 9)
    st = tp.state(g)
    cells = np.arange(0, g.nc, 5, dtype=np.int32)
    m = GpuBlackoilModel(g, tp.tables(), wells=(np.array([0, cells.size], np.int32), cells))
    m.setState(st)
    press = st.p[cells] * 1.03
    b, rsmax, rvmax = m.perfPvtAt(press)
    n = 4
    p = np.linspace(150, 350, n) * decks.BAR
    coeff = np.zeros((n, 3))
    reg = np.array([0, 1, 0, 1], np.int32)
    m._chk(m.lib.opmgpu_voidage_coefficients(m.ctx, n, capi.dptr(p), capi.dptr(np.zeros(n)), capi.dptr(np.zeros(n)), capi.iptr(reg), capi.dptr(coeff)))
    m.close()
    twin = tp.twin_tables()
    pvtnum = g.pvtnum[cells]
    assert _close(b[:, 0], oracle.pvt(twin, "bWat", press, pvtnum=pvtnum)[:, 0])
    assert _close(b[:, 1], oracle.pvt(twin, "bOil", press, np.zeros(cells.size), np.ones(cells.size, np.int8), pvtnum)[:, 0])
    assert np.all(b[:, 2] == 1.0) and np.all(rsmax == 0.0) and np.all(rvmax == 0.0)
    assert _close(coeff[:, 0], 1.0 / oracle.pvt(twin, "bWat", p, pvtnum=reg)[:, 0])
    assert _close(coeff[:, 1], 1.0 / oracle.pvt(twin, "bOil", p, np.zeros(n), np.ones(n, np.int8), reg)[:, 0])
    assert np.all(coeff[:, 2] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# G4: lockstep Newton iterations with device wells -- the logic of util.lockstep_parity with the two-phase tables on the device and the twin
# under the oracle (host well model with the explicit Schur complement), at lockstep_parity's tolerances
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["ilu0_bicgstab", "cpr_gmres", "cpr_gmres_float"])
def test_lockstep_newton_with_wells(gpu_lib, oracle, config):
    cpr, gmres, single = {"ilu0_bicgstab": (0, 0, False), "cpr_gmres": (1, 1, False), "cpr_gmres_float": (1, 1, True)}[config]
    # lockstep_parity's defaults; the float solve with the figures of its one float user (test_gpu_fullsize.py, TIMED_KW["cart100_f32"])
    reduction, tol_p, tol_s, tol_jac, tol_op = (1e-10, 1e-6, 1e-6, 1e-11, 1e-9) if not single else (1e-5, 1e-3, 5e-3, 5e-7, 2e-5)
    g = tp.grid(5, 7, 9, pvt_regions=1)
    two, twin = tp.tables(), tp.twin_tables()
    st = tp.state(g)
    st.sat[:, 0] = np.minimum(st.sat[:, 0], 0.6); st.sat[:, 1] = 1.0 - st.sat[:, 0]
    wl = _wells(g, "lockstep")
    nc = g.nc
    prm_g = capi.default_params(linear_solver_reduction=reduction, linear_solver_maxiter=2000, cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=cpr,
                                newton_use_gmres=gmres, cpr_stage2_relax=0.9 if single else 1.0)
    prm_o = capi.default_params(linear_solver_reduction=1e-10, linear_solver_maxiter=8000)
    gm = GpuBlackoilModel(g, two, prm_g)
    rowptr0, col0 = oracle.pattern(g)
    scale = np.asarray(prm_g.matbalscale[:])
    md = W.DeviceWellModel(gm, wl, W.WellState(wl, st.p))
    ob = OracleBackend(oracle, g, twin, prm_o, wells=wl.arrays())
    mo = W.WellCoupledModel(ob, W.StandardWellsHost(wl, g.z, twin.surface_density[0]), W.WellState(wl, st.p))
    diag_perf = perforated_diag_mask(rowptr0, col0, wl.cells)
    diag = np.repeat(np.arange(nc), np.diff(rowptr0)) == col0
    dt = 2 * decks.DAY
    md.prepareStep(dt, st); mo.prepareStep(dt, st)
    rng = np.random.default_rng(5)
    switched = False
    for it in range(3):
        gm.setSolvePrecision(single)
        gm.assemble(it == 0)
        mo.assemble(it == 0)
        _, val_res, _, _ = oracle.assemble(g, twin, dt, ob.st, rowptr0, col0, scale=tuple(scale), accum0=ob.acc0)
        if it == 0:
            md.pull_well_state()
            assert md.presolve_converged and md.presolve_iterations == mo.wh.well_iterations
        gr, gc, gv = gm.jacobian()
        assert np.array_equal(gr, rowptr0) and np.array_equal(gc, col0)
        res = gm.residual()
        assert rel_err(res[:2 * nc], ob.r[:2 * nc]) < 1e-11, (it, rel_err(res[:2 * nc], ob.r[:2 * nc]))
        assert np.all(res[2 * nc:] == 0.0), it
        gv, val_res = gv.reshape(-1, 3, 3), val_res.reshape(-1, 3, 3)
        keep = ~diag_perf
        assert rel_err(gv[keep][:, :2, :2], val_res[keep][:, :2, :2]) < tol_jac, it
        # the pinned gas unknown, the perforated cells' blocks included (the wells add nothing to it)
        assert np.all(gv[:, :2, 2] == 0.0) and np.all(gv[~diag][:, 2, :] == 0.0), it
        assert np.array_equal(gv[diag][:, 2, :], np.tile([0.0, 0.0, 1.0], (nc, 1))), it
        # the coupled operator on vectors without a gas component (the twin's third column is not the two-phase code's)
        for _ in range(2):
            x3 = rng.standard_normal(3 * nc) * np.tile([1e5, 1e-2, 0.0], nc)
            yo = oracle.spmv(ob.rowptr, ob.col, ob.val, x3).reshape(nc, 3)
            yg = gm.spmv(x3).reshape(nc, 3)
            assert rel_err(yg[:, :2], yo[:, :2]) < tol_op, (it, rel_err(yg[:, :2], yo[:, :2]))
            assert np.all(yg[:, 2] == 0.0), it
        cg = gm.getConvergence(); co = ob.getConvergence()
        assert np.allclose(gm.CNV[:2], ob.CNV[:2], rtol=1e-9) and np.allclose(gm.MB[:2], ob.MB[:2], rtol=1e-7, atol=1e-18)
        assert np.allclose(gm.B_avg[:2], ob.B_avg[:2], rtol=1e-12) and gm.B_avg[2] == 1.0 and gm.CNV[2] == 0.0 and gm.MB[2] == 0.0
        cg = md.wellConvergence() and cg; co = mo.wh.converged(ob.B_avg) and co
        assert np.allclose(md.well_flux_residual[:2], mo.wh.well_flux_residual[:2], rtol=1e-7, atol=1e-14) and md.well_flux_residual[2] == 0.0
        assert md.well_ctrl_residual == pytest.approx(mo.wh.well_ctrl_residual, rel=1e-7, abs=1e-14)
        assert cg == co
        dx = gm.solveJacobianSystem(want_dx=True, single_precision=single)
        assert gm.linear_reduction <= reduction, (it, gm.linear_reduction)
        assert np.all(dx[2 * nc:] == 0.0) and np.abs(dx[:nc]).max() > 0.0, it                       # bit for bit, in float and in double
        gm.updateState()
        ob.solveJacobianSystem(single_precision=False)
        mo.wh.recover_and_update(ob.perfDx(wl.nperf), mo.ws)
        ob.updateState()
        a, b = gm.getState(), ob.getState()
        assert np.all(a.sat[:, 2] == 0.0) and np.all(a.rs == 0.0) and np.all(a.rv == 0.0) and np.all(a.hc == capi.HC_GAS_AND_OIL), it
        assert np.abs(a.p - b.p).max() <= tol_p * np.abs(b.p).max(), (it, np.abs(a.p - b.p).max() / np.abs(b.p).max())
        assert np.abs(a.sat[:, :2] - b.sat[:, :2]).max() <= tol_s, (it, np.abs(a.sat - b.sat).max())
        ob.st = a.copy()
        ws = md.pull_well_state()
        assert np.allclose(ws.bhp, mo.ws.bhp, rtol=max(1e-6, tol_p)), (it, ws.bhp, mo.ws.bhp)
        assert np.allclose(ws.qs[:, :2], mo.ws.qs[:, :2], rtol=max(1e-5, 10 * tol_p), atol=max(1e-8, tol_p) * np.abs(mo.ws.qs).max()), it
        assert np.array_equal(ws.current, mo.ws.current), it
        assert np.allclose(ws.perf_rates[:, :2], mo.ws.perf_rates[:, :2], rtol=1e-6, atol=1e-9 * np.abs(mo.ws.perf_rates).max()), it
        assert np.all(ws.qs[:, 2] == 0.0) and np.all(ws.perf_rates[:, 2] == 0.0), it
        switched = switched or ws.current[2] == 1
        mo.ws.assign(ws)
    assert switched                                        # the ORAT producer went to its BHP limit
    gm.close()
