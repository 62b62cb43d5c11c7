"""GPU: rock regions and irreversible compaction on the device (the rule: include/opmgpu.h at opmgpu_set_rock_regions; restated in
rock_reference.py; the cells: rock_cases.py, whose census test_rock_reference.py asserts).

  a  the history kernel at 1, 63, 64, 65, 255, 256, 257 cells, bit for bit against np.minimum, twice (one thread per cell on a grid sized
     by the cell count: the kernel has no grid cap, so there is no size past one)
  b  opmgpu_get_rock_multipliers on the edge set: |device - restatement| <= 2 * 2^-52 * (|y_i| + |slope (x - x_i)|) -- one fused against
     two rounded operations --; a ROCK-form cell within 4 * 2^-52 (three roundings next to 1) with trans_mult == 1.0; an off-curve cell
     does not depend on p at all (the same bits a bar higher: its derivative is exactly 0.0 -- the entry point hands out values only)
  c  the evaluator slot by slot through k_perf_props, k_simulator_data and k_assemble_rows on isolated cells, three-phase and oil-water,
     tables in LDS and read from the blob
  d  one region with test_vappars_rocktab_parity's table, REVERSIBLE, on the 7 x 6 x 5 grid against the oracle at RTOL_JAC
  e  regions set and removed give the bits of a context that never had any
  f  one converged step down and one up: p_min is the running minimum, recovered cells keep the pore volume of their minimum, the same
     two steps REVERSIBLE end elsewhere
  g  persistence (save / restore, a failed sub-step, precision, re-plans) and every OPMGPU_EINVAL
  h  tests/golden/decks/ROCKCOMP_SMALL.DATA through the report-step driver, restart included

Tolerance of c: test_gpu_cell_edges.py's -- per (property, slot) and group of cells 8 times the oracle's error on the same cells WITHOUT
rock regions (only the argument of two look-ups changes), capped at the oracle's own bound, floor 64 ulp.  The oil-water cells are held
to the oracle's error on their three-phase twin (twophase.py) in the water and oil slots."""
import ctypes as C
import os

import numpy as np
import pytest

import cell_edge_cases as E
import cell_reference as R
import rock_cases as RC
import rock_reference as K
from opmgpu import capi, decks, eclio, wells as W
from opmgpu.model import GpuBlackoilModel, newton_step
from opmgpu.simulator import Simulator
from util import rel_err, slot_err

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DECK = os.path.join(HERE, "golden", "decks", "ROCKCOMP_SMALL.DATA")
U = 2.0 ** -52
MARGIN, FLOOR = 8.0, 64 * U                     # test_gpu_cell_edges.py's
RTOL_JAC = 1e-11                                # test_gpu_assembly.py's
DT = 3 * decks.DAY
BAR = decks.BAR
INF = float("inf")


def _loose_grid(nc):
    return decks.GridData(nc, np.zeros((0, 2), np.int32), np.zeros(0), np.full(nc, 50.0), np.full(nc, 2000.0))


# ---------------------------------------------------------------- a
@pytest.mark.parametrize("nc", [1, 63, 64, 65, 255, 256, 257])
def test_history_kernel_bit_for_bit(gpu_lib, nc):
    rng = np.random.default_rng(nc)
    p = rng.uniform(100, 400, nc) * BAR
    st = decks.State(p, np.tile([0.2, 0.6, 0.2], (nc, 1)), np.full(nc, 50.0), np.zeros(nc), np.full(nc, capi.HC_GAS_AND_OIL, np.int8))
    m = GpuBlackoilModel(_loose_grid(nc), decks.satfunc_standard_tables(), capi.default_params())
    m.setRockRegions(decks.RockRegions(np.zeros(nc, np.int32), [(1.0, 0.0)], [[(50.0, 0.9, 0.8), (450.0, 1.1, 1.2)]], irreversible=True))
    assert np.all(np.isinf(m.rockHistory())) and np.all(m.rockHistory() > 0)           # starts at +inf
    m.setState(st)
    m.updateRockHistory()
    assert np.array_equal(m.rockHistory(), p)
    h0 = np.where(rng.random(nc) < 0.3, INF, p + rng.uniform(-30, 30, nc) * BAR)
    h0[0] = p[0]                                                                         # a tie
    if nc > 2:
        h0[1], h0[-1] = np.nextafter(p[1], INF), np.nextafter(p[-1], 0.0)
    m.setRockHistory(h0)
    want = K.history(h0, p)
    for _ in range(2):                                                                   # two calls give the same bits
        m.updateRockHistory()
        assert np.array_equal(m.rockHistory(), want)
    m.close()


# ---------------------------------------------------------------- b, c
class _Plain:
    """the cells of a rock case set WITHOUT rock regions: what the oracle can evaluate, the yardstick's reference"""

    def __init__(self, Cs):
        self.state, self.nc = Cs.state, Cs.nc
        self.ref, self.recs = R.cells(Cs.ref_tab, Cs.pvtnum, Cs.satnum, Cs.state)


@pytest.fixture(scope="module")
def edge(oracle):
    """{form: (cells, the oracle's error table {hc group: err[23][4]} on the same cells without rock regions)}"""
    out = {}
    for form in RC.FORMS:
        Cs = RC.load(form)
        P = _Plain(Cs)
        g = Cs.grid()
        props = oracle.cell_props(decks.GridData(g.nc, g.conn_cells, g.trans, g.pv, g.z, pvtnum=g.pvtnum, satnum=g.satnum), Cs.ref_tab, Cs.state)
        out[form] = (Cs, E.error_table(P, props, R.NAMES[:oracle.NPROP]))
    return out


def limits(Cs, yard, names, slots):
    """test_gpu_cell_edges.limits: {group: limit[len(names)][len(slots)]}"""
    cap = E.oracle_limits(Cs, R.NAMES[:23])
    yard = {g: np.minimum(yard[g], cap[g]) for g in yard}
    out = {}
    for g in yard:
        rows = []
        for n in names:
            src = yard["gas+oil"] if n in ("rsSat", "rvSat") and "gas+oil" in yard else yard[g]
            rows.append(src[R.NAMES.index({"rsSat": "rs", "rvSat": "rv"}.get(n, n))][list(slots)])
        out[g] = np.maximum(MARGIN * np.array(rows), FLOOR)
    return out


def check(Cs, got, names, yard, what, slots=(0, 1, 2, 3)):
    err, lim = E.error_table(Cs, got, names, slots), limits(Cs, yard, names, slots)
    for g in err:
        i, s = np.unravel_index(np.argmax(err[g] / lim[g]), err[g].shape)
        print("%s, '%s': largest error %.2e; nearest its limit: %s %s, %.2e of %.2e" % (what, g, err[g].max(), names[i], R.SLOTS[slots[s]], err[g][i, s], lim[g][i, s]))
        bad = np.argwhere(err[g] > lim[g])
        assert bad.size == 0, [(what, g, names[i], R.SLOTS[slots[s]], err[g][i, s], lim[g][i, s]) for i, s in bad]


def model_of(Cs, big=False, wells=None, **prm):
    m = GpuBlackoilModel(Cs.grid(), Cs.tab, capi.default_params(**prm), wells=wells)
    m.setRockRegions(RC.regions(Cs.rocknum, big=big))
    m.prepareStep(DT, Cs.state)
    m.setRockHistory(Cs.p_min)
    return m


@pytest.mark.parametrize("form", RC.FORMS)
def test_multipliers_on_the_edge_set(gpu_lib, form):
    Cs = RC.load(form)
    pv, tr, _, _, mpv, mtr = K.multipliers(Cs.regions, Cs.rocknum, Cs.state.p, Cs.p_min)
    tab = np.array([b["form"] == "table" for b in Cs.rock_recs])
    off = np.array([b["form"] == "table" and not b["on_curve"] for b in Cs.rock_recs])
    m = model_of(Cs)
    gpv, gtr = m.rockMultipliers()
    print("%s: worst pv_mult %.2f, trans_mult %.2f of the bound" % (form, (np.abs(gpv - pv)[tab] / (2 * U * mpv[tab])).max(), (np.abs(gtr - tr)[tab] / (2 * U * mtr[tab])).max()))
    assert np.all(np.abs(gpv - pv)[tab] <= 2 * U * mpv[tab]) and np.all(np.abs(gtr - tr)[tab] <= 2 * U * mtr[tab])
    assert np.all(np.abs(gpv - pv)[~tab] <= 4 * U) and np.all(gtr[~tab] == 1.0)
    # an off-curve cell a bar higher: the same bits (d/dp exactly 0.0); every other cell moves
    s = Cs.state
    m.setState(decks.State(s.p + np.where(off, 1.0 * BAR, 0.0), s.sat, s.rs, s.rv, s.hc))
    hpv, htr = m.rockMultipliers()
    assert off.sum() >= 3 * RC.MIN_CELLS and np.array_equal(hpv, gpv) and np.array_equal(htr, gtr)
    m.setState(decks.State(s.p - np.where(off, 0.0, 1.0 * BAR), s.sat, s.rs, s.rv, s.hc))          # the others a bar lower: on the curve, they move
    lpv, _ = m.rockMultipliers()
    assert np.all(lpv[~off] != gpv[~off]) and np.array_equal(lpv[off], gpv[off])
    assert np.array_equal(m.rockHistory(), Cs.p_min)                                                # nothing here updates the history
    m.close()
    # without regions: the one rock of the tables
    m = GpuBlackoilModel(Cs.grid(), Cs.tab, capi.default_params())
    m.setState(s)
    qpv, qtr = m.rockMultipliers()
    X = Cs.tab.rock_comp * (s.p - Cs.tab.rock_pref)
    assert np.all(np.abs(qpv - (1.0 + X + 0.5 * X * X)) <= 4 * U) and np.all(qtr == 1.0)
    m.close()


WOG_PERF = ["p_o", "rs", "rv", "b_w", "b_o", "b_g", "mob_w", "mob_o", "mob_g"]
WO_KEEP = {"p_o", "b_w", "b_o", "mob_w", "mob_o", "rho_w", "rho_o", "mu_w", "mu_o", "kr_w", "kr_o", "accum_w", "accum_o"}
SD_PAIRS = [("1OVERBW", "b_w"), ("1OVERBO", "b_o"), ("1OVERBG", "b_g"), ("WAT_DEN", "rho_w"), ("OIL_DEN", "rho_o"), ("GAS_DEN", "rho_g"),
            ("WAT_VISC", "mu_w"), ("OIL_VISC", "mu_o"), ("GAS_VISC", "mu_g"), ("WATKR", "kr_w"), ("OILKR", "kr_o"), ("GASKR", "kr_g"),
            ("RSSAT", "rsSat"), ("RVSAT", "rvSat")]


@pytest.mark.parametrize("form", RC.FORMS)
def test_perf_props_and_simulator_data_with_regions(gpu_lib, edge, form):
    """k_perf_props (one well through every cell) and k_simulator_data: mob_* carries trans_mult; in the oil-water form the water and oil
    slots with respect to (p, Sw)"""
    Cs, yard = edge[form]
    wo = form == "wo"
    m = model_of(Cs, wells=(np.array([0, Cs.nc], np.int32), np.arange(Cs.nc, dtype=np.int32)))
    assert np.array_equal(m.rockHistory(), Cs.p_min)                                                # (carried through the constructor's well re-plan order)
    m.assemble(True)
    pp = m.perfProps(Cs.nc).reshape(Cs.nc, 9, 4)
    d = m.simulatorData()
    m.close()
    keep = [i for i, n in enumerate(WOG_PERF) if not wo or n in WO_KEEP]
    check(Cs, pp[:, keep][:, :, :3 if wo else 4], [WOG_PERF[i] for i in keep], yard, "perfProps " + form, slots=(0, 1, 2) if wo else (0, 1, 2, 3))
    pairs = [(k, n) for k, n in SD_PAIRS if not wo or n in WO_KEEP]
    check(Cs, np.stack([d[k] for k, _ in pairs], 1)[:, :, None], [n for _, n in pairs], yard, "simulatorData " + form, slots=(0,))
    # the multiplier is IN the mobilities: against the plain cells they differ wherever trans_mult is not 1
    tr = K.multipliers(Cs.regions, Cs.rocknum, Cs.state.p, Cs.p_min)[1]
    assert (np.abs(tr - 1.0) > 0.01).sum() > Cs.nc // 2


@pytest.mark.parametrize("blob", [False, True], ids=["lds", "blob"])
@pytest.mark.parametrize("form", RC.FORMS)
def test_isolated_cell_assembly_with_regions(gpu_lib, edge, form, blob):
    """k_assemble_rows on a grid without connections (test_gpu_cell_edges.py's mapping): the diagonal block of a cell is matbalscale[a] *
    pv/dt * d accum_a / d(p, Sw, X), its residual pv/dt * (accum_a - accum0_a) -- after assemble(True) and after a second arrangement of
    the same cells (state, rock region and history permuted) + assemble(False); tables in LDS and, a long table added, read from the blob"""
    Cs, yard = edge[form]
    wo = form == "wo"
    grid = Cs.grid()
    reg = RC.regions(Cs.rocknum, big=blob)
    f64 = sum(a.nbytes for a in vars(Cs.tab).values() if isinstance(a, np.ndarray) and a.dtype == np.float64)
    rock_bytes = 5 * 8 * int(reg.tab_ptr[-1])
    assert (f64 + rock_bytes > 24 * 1024) if blob else (2 * sum(a.nbytes for a in vars(Cs.tab).values() if isinstance(a, np.ndarray)) + 2 * rock_bytes < 24 * 1024)
    names = ["accum_w", "accum_o"] + ([] if wo else ["accum_g"])
    ne = len(names)
    acc = Cs.ref[:, [R.NAMES.index(n) for n in names]]                                   # [nc][ne][4]
    scale = np.asarray(capi.default_params().matbalscale[:])
    pvdt = np.asarray(grid.pv) / DT
    f = scale[None, :, None] * pvdt[:, None, None]
    st2, rn2, pm2, perm = Cs.shifted()
    m = model_of(Cs, big=blob)
    for initial, src in ((True, np.arange(Cs.nc)), (False, perm)):                      # cell i holds the arrangement of cell src[i]
        def at_source(a):
            out = np.empty_like(a)
            out[src] = a
            return out
        if not initial:
            m.setState(st2)
            m.setRockRegions(RC.regions(rn2, big=blob))
            m.setRockHistory(pm2)
        m.assemble(initial)
        rowptr, col, val = m.jacobian()
        assert np.array_equal(col, np.arange(Cs.nc)) and np.array_equal(rowptr, np.arange(Cs.nc + 1))
        tag = "%s %s assemble(%s)" % (form, "blob" if blob else "lds", initial)
        blocks = val.reshape(-1, 3, 3) / f
        if wo:
            assert np.all(blocks[:, :2, 2] == 0.0)                                       # nothing depends on the inactive third variable
            check(Cs, at_source(blocks[:, :2, :2]), names, yard, "Jacobian " + tag, slots=(1, 2))
        else:
            check(Cs, at_source(blocks), names, yard, "Jacobian " + tag, slots=(1, 2, 3))
        excess = m.residual().reshape(3, Cs.nc).T[:, :ne] / pvdt[:, None] - (acc[src][:, :, 0] - acc[:, :, 0])
        check(Cs, (acc[:, :, 0] + at_source(excess))[:, :, None], names, yard, "residual " + tag, slots=(0,))
    m.close()


def test_reversible_mode_on_the_edge_set(gpu_lib, edge):
    """the same cells under OPMGPU_ROCK_REVERSIBLE: every cell on its curve, whatever its history"""
    Cs, yard = edge["wog"]
    ref, _ = RC.reversible(Cs)

    class Rev:
        state, nc, recs = Cs.state, Cs.nc, Cs.recs
    Rev.ref = ref
    m = GpuBlackoilModel(Cs.grid(), Cs.tab, capi.default_params(), wells=(np.array([0, Cs.nc], np.int32), np.arange(Cs.nc, dtype=np.int32)))
    m.setRockRegions(RC.regions(Cs.rocknum, irreversible=False))
    m.prepareStep(DT, Cs.state)
    m.setRockHistory(Cs.p_min)
    m.assemble(True)
    pp = m.perfProps(Cs.nc).reshape(Cs.nc, 9, 4)
    check(Rev, pp, WOG_PERF, yard, "perfProps reversible")
    gpv, _ = m.rockMultipliers()
    rpv, _, _, _, mag, _ = K.multipliers(RC.regions(Cs.rocknum, irreversible=False), Cs.rocknum, Cs.state.p, Cs.p_min)
    tab = mag > 0
    assert np.all(np.abs(gpv - rpv)[tab] <= 2 * U * mag[tab])
    m.close()


# ---------------------------------------------------------------- d
def test_one_reversible_region_meets_the_oracles_rocktab(gpu_lib, oracle):
    rocktab = [(100.0, 0.98, 0.95), (200.0, 1.0, 1.0), (300.0, 1.03, 1.08), (500.0, 1.05, 1.12)]       # test_vappars_rocktab_parity's
    plain = decks.satfunc_standard_tables()
    tab = decks.satfunc_standard_tables(rocktab=rocktab)
    grid = decks.cartesian_grid(7, 6, 5, lognormal_sigma=0.5)
    prm = capi.default_params()
    scale = tuple(prm.matbalscale)
    rowptr, col = oracle.pattern(grid)
    dt = 2 * decks.DAY
    for seed in (1, 2):
        st = decks.random_state(grid, tab, seed=seed)
        m = GpuBlackoilModel(grid, plain, prm)
        m.setRockRegions(decks.RockRegions(np.zeros(grid.nc, np.int32), [(1.0, 0.0)], [rocktab], irreversible=False))
        m.prepareStep(dt, st)
        m.setRockHistory(np.full(grid.nc, 50.0 * BAR))                                 # REVERSIBLE: no evaluator reads it
        m.assemble(True)
        r0, v0, _, _ = oracle.assemble(grid, tab, dt, st, rowptr, col, scale=scale)
        r_plain, v_plain, _, _ = oracle.assemble(grid, plain, dt, st, rowptr, col, scale=scale)
        assert rel_err(v_plain, v0) > 1e-3                                             # the table matters for this state
        print("seed %d: Jacobian %.2e (slot %.2e), residual %.2e" % (seed, rel_err(m.jacobian()[2], v0), slot_err(m.jacobian()[2], v0), rel_err(m.residual(), r0)))
        assert rel_err(m.jacobian()[2], v0) < RTOL_JAC and slot_err(m.jacobian()[2], v0) < RTOL_JAC
        assert rel_err(m.residual(), r0) < RTOL_JAC
        m.close()


# ---------------------------------------------------------------- e
def _two_iterations(m, dt, st):
    m.prepareStep(dt, st)
    out = []
    for it in range(2):
        m.assemble(it == 0)
        m.getConvergence()
        out += [m.residual(), m.jacobian()[2], m.solveJacobianSystem(want_dx=True, single_precision=False)]
        m.updateState()
    g = m.getState()
    return out + [g.p, g.sat, g.rs, g.rv, g.hc]


@pytest.mark.parametrize("rocktab", [False, True], ids=["rock", "rocktab"])
def test_regions_removed_give_the_bits_of_a_context_without(gpu_lib, rocktab):
    """never set == set, used and removed: residual, Jacobian, dx and the state of two Newton iterations, bit for bit"""
    extra = dict(rocktab=[(100.0, 0.98, 0.95), (200.0, 1.0, 1.0), (300.0, 1.03, 1.08), (500.0, 1.05, 1.12)]) if rocktab else {}
    tab = decks.satfunc_standard_tables(**extra)
    grid = decks.cartesian_grid(6, 5, 4, lognormal_sigma=0.4)
    st = decks.random_state(grid, tab, seed=4)
    prm = capi.default_params(linear_solver_reduction=1e-8, linear_solver_maxiter=200)
    dt = 2 * decks.DAY
    a = GpuBlackoilModel(grid, tab, prm)
    want = _two_iterations(a, dt, st)
    a.close()
    b = GpuBlackoilModel(grid, tab, prm)
    reg = decks.RockRegions(np.arange(grid.nc) % 2, [(1.0, 0.0), (150.0, 4e-5)], [[(80.0, 0.9, 0.7), (250.0, 1.0, 1.0), (400.0, 1.02, 1.1)], None], irreversible=True)
    b.setRockRegions(reg)
    with_regions = _two_iterations(b, dt, st)
    assert rel_err(with_regions[1], want[1]) > 1e-4                                    # they were in force
    b.updateRockHistory()
    b.setRockRegions(None)
    assert b.rock_regions is None and np.all(np.isinf(b.rockHistory()))
    got = _two_iterations(b, dt, st)
    b.close()
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------- f
_SOFT = [(100.0, 0.88, 0.5), (200.0, 0.94, 0.75), (300.0, 1.0, 1.0), (400.0, 1.02, 1.1)]


def _down_and_up(irreversible):
    """a 6 x 5 x 3 box at about 300 bar: one step with a producer at 140 bar, one with a water injector at 330 bar; the state is saved
    after each.  Returns (the pressures at the three saved states, p_min after each save, the multipliers at the end, the regions)"""
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(6, 5, 3, lognormal_sigma=0.3)
    nx, ny, nz = grid.dims
    nc = grid.nc
    p0 = (300.0 + 0.7 * (np.arange(nc) // (nx * ny))) * BAR
    st = decks.State(p0, np.tile([0.2, 0.8, 0.0], (nc, 1)), np.full(nc, 40.0), np.zeros(nc), np.full(nc, capi.HC_OIL_ONLY, np.int8))
    reg = decks.RockRegions(np.arange(nc) % 2, [(1.0, 0.0), (300.0, 4e-5)], [_SOFT, None], irreversible=irreversible)
    m = GpuBlackoilModel(grid, tab, capi.default_params(linear_solver_reduction=1e-8, linear_solver_maxiter=300))
    m.setRockRegions(reg)
    m.setState(st)
    m.updateRockHistory()
    m.saveState()
    ps, hs = [m.getState().p], [m.rockHistory()]
    colm = lambda i, j: [i + nx * j + nx * ny * k for k in range(nz)]      # noqa: E731
    WI = 5.0 * float(np.median(grid.trans))
    for name, wtype, cells, frac, bhp in (("P", W.PRODUCER, colm(nx - 1, ny - 1), (0.0, 1.0, 0.0), 140.0), ("I", W.INJECTOR, colm(0, 0), (1.0, 0.0, 0.0), 330.0)):
        wl = W.Wells()
        wl.add_well(name, wtype, grid.z[cells[0]], cells, WI, frac, (W.BHP, bhp * BAR), limits=[])
        md = W.DeviceWellModel(m, wl, W.WellState(wl, m.getState().p))
        md.prepareStep(4 * decks.DAY)
        newton_step(md, max_iter=20)
        md.saveState()
        if not irreversible:
            m.updateRockHistory()                     # (saveState does it only under IRREVERSIBLE; REVERSIBLE keeps the plane all the same)
        ps.append(m.getState().p); hs.append(m.rockHistory())
    mult = m.rockMultipliers()
    m.close()
    return ps, hs, mult, reg


@pytest.fixture(scope="module")
def down_and_up(gpu_lib):
    return _down_and_up(True), _down_and_up(False)


def test_history_is_the_running_minimum_of_the_saved_states(down_and_up):
    (ps, hs, _, _), _ = down_and_up
    assert np.all(ps[1] < ps[0] - 20 * BAR) and np.all(ps[2] > ps[1] + 5 * BAR)       # down, then up, everywhere
    run = np.full(ps[0].size, INF)
    for p, h in zip(ps, hs):
        run = np.minimum(run, p)
        assert np.array_equal(h, run)


def test_recovered_cells_keep_the_pore_volume_of_their_minimum(down_and_up):
    (ps, hs, (pv, tr), reg), (qs, _, (rpv, _), _) = down_and_up
    soft = reg.rocknum == 0
    above = ps[2] > hs[2]
    assert above[soft].sum() >= 10
    want = K.multipliers(reg, reg.rocknum, hs[2], np.full(hs[2].size, INF))            # the table AT p_min
    pick = soft & above
    assert np.all(np.abs(pv - want[0])[pick] <= 2 * U * want[4][pick]) and np.all(np.abs(tr - want[1])[pick] <= 2 * U * want[5][pick])
    at_p = K.multipliers(reg, reg.rocknum, ps[2], np.full(hs[2].size, INF))
    assert np.all(pv[pick] < at_p[0][pick] - 1e-4)                                     # not the curve's value at the recovered pressure
    # the ROCK-form region is elastic: its multiplier is the one at p
    assert np.all(np.abs(pv - at_p[0])[~soft] <= 4 * U)
    # the same two steps REVERSIBLE end at another pressure
    assert np.abs(qs[2] - ps[2]).max() > 0.5 * BAR and np.all(np.abs(rpv - K.multipliers(reg, reg.rocknum, qs[2], np.full(hs[2].size, INF))[0])[soft] <= 2 * U * 2)


# ---------------------------------------------------------------- g
def _wells(g):
    nx, ny, nz = g.dims
    colm = lambda i, j: [i + nx * j + nx * ny * k for k in range(nz)]      # noqa: E731
    WI = 5.0 * float(np.median(g.trans))
    wl = W.Wells()
    wl.add_well("INJ", W.INJECTOR, g.z[colm(0, 0)[0]], colm(0, 0), WI, (0.0, 0.0, 1.0), (W.SURFACE_RATE, 300.0 / 86400.0, (0.0, 0.0, 1.0)),
                limits=[(W.BHP, 600 * BAR)])
    wl.add_well("P1", W.PRODUCER, g.z[colm(nx - 1, ny - 1)[0]], colm(nx - 1, ny - 1)[:3], WI, (0.0, 1.0, 0.0), (W.BHP, 150 * BAR), limits=[])
    return wl


def test_regions_and_history_persist(gpu_lib):
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(6, 5, 4, lognormal_sigma=0.3)
    nc = grid.nc
    st = decks.random_state(grid, tab, seed=3)
    reg = decks.RockRegions(np.random.default_rng(2).integers(0, 3, nc), [(1.0, 0.0), (1.0, 0.0), (200.0, 5e-5)],
                            [_SOFT, [(50.0, 0.9, 0.9), (450.0, 1.1, 1.1)], None], irreversible=True)
    dt = 4 * decks.DAY
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    m.setRockRegions(reg)
    m.prepareStep(dt, st)
    h0 = st.p + np.random.default_rng(5).uniform(-40, 25, nc) * BAR
    m.setRockHistory(h0)
    mult0 = m.rockMultipliers()

    def same():
        a = m.rockMultipliers()
        return np.array_equal(m.rockHistory(), h0) and np.array_equal(a[0], mult0[0]) and np.array_equal(a[1], mult0[1])
    # save keeps the history in IRREVERSIBLE mode up to date; restore does not touch it
    m.saveState()
    h1 = np.minimum(h0, st.p)
    assert np.array_equal(m.rockHistory(), h1)
    m.setRockHistory(h0)
    # a failed sub-step: the state moves, is restored; the history never saw it
    rng = np.random.default_rng(1)
    dx = np.concatenate([rng.standard_normal(nc) * 60 * BAR, rng.standard_normal(nc) * 0.05, rng.standard_normal(nc) * 0.05])
    m.updateState(dx)
    assert not np.array_equal(m.getState().p, st.p) and np.array_equal(m.rockHistory(), h0)
    m.restoreState()
    assert np.array_equal(m.getState().p, st.p) and same()
    m.prepareStep(dt / 4)
    assert same()
    # a change of the solve precision
    for single in (True, False):
        m.setSolvePrecision(single)
        m.assemble(True)
        assert same() and m.rock_regions is reg
    jac = m.jacobian()[2]
    # re-plans: host wells on and off, then device wells
    m.setWells(np.array([0, 3], np.int32), np.array([2, 32, 62], np.int32))
    assert same()
    m.setWells(np.array([0], np.int32), np.zeros(0, np.int32))
    m.setSolvePrecision(False)
    m.assemble(True)
    assert np.array_equal(m.jacobian()[2], jac)                                       # the same assembly after two re-plans
    wl = _wells(grid)
    W.DeviceWellModel(m, wl, W.WellState(wl, st.p))
    assert same()
    m.assemble(True)
    m.close()


def _spec(nc, **over):
    """a valid opmgpu_rock_regions (two regions: a 3-row table and the ROCK form) with fields replaced; returns (struct, keep-alive)"""
    keep = dict(rocknum=capi.i32(np.arange(nc) % 2), rock_pref=capi.f64([1e5, 2e7]), rock_comp=capi.f64([0.0, 4e-10]), tab_ptr=capi.i32([0, 3, 3]),
                tab_p=capi.f64([1e7, 2e7, 4e7]), tab_pvmult=capi.f64([0.9, 1.0, 1.05]), tab_transmult=capi.f64([0.0, 1.0, 1.1]))
    s = capi.RockRegionsSpec()
    s.nregions, s.mode = over.pop("nregions", 2), over.pop("mode", capi.ROCK_IRREVERSIBLE)
    for k, v in keep.items():
        if k in over:
            v = over[k]
            v = None if v is None else (capi.i32(v) if k in ("rocknum", "tab_ptr") else capi.f64(v))
            keep[k] = v
        setattr(s, k, None if v is None else (capi.iptr(v) if v.dtype == np.int32 else capi.dptr(v)))
    return s, keep


def test_every_refusal_leaves_the_previous_set(gpu_lib):
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(4, 3, 2)
    nc = grid.nc
    st = decks.random_state(grid, tab, seed=1)
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    lib, ctx = m.lib, m.ctx
    err = lambda: lib.opmgpu_last_error(ctx).decode()         # noqa: E731
    # before a state / without regions
    assert lib.opmgpu_get_rock_multipliers(ctx, None, None) == capi.EINVAL and "state" in err()
    assert lib.opmgpu_set_rock_history(ctx, capi.dptr(np.full(nc, 1e7))) == capi.EINVAL and "no rock regions" in err()
    assert lib.opmgpu_update_rock_history(ctx) == capi.EINVAL
    good, keep0 = _spec(nc)
    assert lib.opmgpu_set_rock_regions(ctx, C.byref(good)) == capi.OK
    m.setState(st)
    h0 = st.p - 3 * BAR
    m.setRockHistory(h0)
    mult0 = m.rockMultipliers()
    nan, inf = float("nan"), INF
    bad = [
        (dict(rocknum=None), "NULL"), (dict(rock_pref=None), "NULL"), (dict(rock_comp=None), "NULL"), (dict(tab_ptr=None), "NULL"),
        (dict(tab_p=None), "NULL"), (dict(tab_pvmult=None), "NULL"), (dict(tab_transmult=None), "NULL"),
        (dict(nregions=0), "nregions"), (dict(nregions=-1), "nregions"),
        (dict(rocknum=np.where(np.arange(nc) == 5, 2, 0)), "rocknum of cell 5"), (dict(rocknum=np.where(np.arange(nc) == 7, -1, 0)), "rocknum of cell 7"),
        (dict(mode=2), "mode"), (dict(mode=-1), "mode"),
        (dict(tab_ptr=[0, 1, 1]), "exactly 1 row"), (dict(tab_ptr=[0, 3, 4]), "exactly 1 row"), (dict(tab_ptr=[0, 3, 2]), "decreases"), (dict(tab_ptr=[1, 3, 3]), "start at 0"),
        (dict(tab_p=[1e7, 1e7, 4e7]), "strictly increasing"), (dict(tab_p=[1e7, 5e7, 4e7]), "strictly increasing"),
        (dict(tab_p=[1e7, nan, 4e7]), "not finite"), (dict(tab_pvmult=[0.9, inf, 1.05]), "not finite"), (dict(tab_transmult=[0.0, 1.0, nan]), "not finite"),
        (dict(tab_pvmult=[0.0, 1.0, 1.05]), "pv_mult"), (dict(tab_pvmult=[0.9, -1.0, 1.05]), "pv_mult"), (dict(tab_transmult=[-0.1, 1.0, 1.1]), "trans_mult"),
        (dict(rock_pref=[nan, 2e7]), "rock_pref"), (dict(rock_comp=[0.0, inf]), "rock_comp"),
    ]
    for over, text in bad:
        s, keep = _spec(nc, **over)
        assert lib.opmgpu_set_rock_regions(ctx, C.byref(s)) == capi.EINVAL, over
        assert text in err(), (over, err())
        a = m.rockMultipliers()
        assert np.array_equal(a[0], mult0[0]) and np.array_equal(a[1], mult0[1]) and np.array_equal(m.rockHistory(), h0), over
    h = h0.copy(); h[3] = nan
    assert lib.opmgpu_set_rock_history(ctx, capi.dptr(h)) == capi.EINVAL and "NaN" in err() and np.array_equal(m.rockHistory(), h0)
    assert lib.opmgpu_get_rock_history(ctx, None) == capi.EINVAL
    # the dissolution limits and the regions refuse each other
    with pytest.raises(ValueError, match="rock regions"):
        m.setDissolutionLimits(1e-7)
    assert m.dissolution_limits is None
    lib.opmgpu_set_rock_regions(ctx, None)
    m.setDissolutionLimits(1e-7)
    assert lib.opmgpu_set_rock_regions(ctx, C.byref(good)) == capi.EINVAL and "dissolution limits" in err()
    assert np.all(np.isinf(m.rockHistory()))
    m.close()
    # PVCDO likewise
    import pvcdo_cases as PC
    own, _ = PC.tables("default")
    g = PC.grid()
    mp = GpuBlackoilModel(g, own, capi.default_params())                                # the analytic oil is in force
    s, keep = _spec(g.nc)
    assert mp.lib.opmgpu_set_rock_regions(mp.ctx, C.byref(s)) == capi.EINVAL and "opmgpu_set_pvcdo" in mp.lib.opmgpu_last_error(mp.ctx).decode()
    mp.setPvcdo(None)
    assert mp.lib.opmgpu_set_rock_regions(mp.ctx, C.byref(s)) == capi.OK
    with pytest.raises(ValueError, match="rock regions"):
        mp.setPvcdo(own.pvcdo)
    mp.setPvcdo(None)                                                                   # nothing to take off: the regions stay
    assert np.all(np.isinf(mp.rockHistory()))
    mp.close()


# ---------------------------------------------------------------- h
@pytest.fixture(scope="module")
def golden_run(gpu_lib, tmp_path_factory):
    """the golden deck through the report-step driver: (base of the full run's files, the pressures the model held at every saveState,
    the reports, base of the REVERS variant's files, base of the run restarted from report 2)"""
    d = tmp_path_factory.mktemp("rockcomp")
    tight = dict(linear_solver_reduction=1e-8, linear_solver_maxiter=300)
    saved = []

    class Recording(GpuBlackoilModel):
        def saveState(self):
            super().saveState()
            saved.append(self.getState().p)
    base = str(d / "FULL")
    sim = Simulator(DECK, params=capi.default_params(**tight), output_base=base, model_factory=lambda g, t, p: Recording(g, t, p))
    assert sim.rock_regions is not None and sim.model.rock_regions is sim.rock_regions
    reports = sim.run()
    p_init = sim.state0.p
    sim.close()
    rev = str(d / "REV.DATA")
    with open(rev, "w") as f:
        f.write(open(DECK).read().replace(" IRREVERS 2 /", " REVERS 2 /"))
    base_r = str(d / "REVOUT")
    sr = Simulator(rev, params=capi.default_params(**tight), output_base=base_r)
    assert sr.rock_regions.mode == capi.ROCK_REVERSIBLE
    sr.run(); sr.close()
    base_s = str(d / "RESTARTED")
    ss = Simulator(DECK, params=capi.default_params(**tight), output_base=base_s, restart=(base, 3))      # report 3 of the file = the state after report step 2
    ss.run(); ss.close()
    return base, [p_init] + saved, reports, base_r, base_s


def test_golden_deck_presrock_is_the_running_minimum(golden_run):
    base, saved, reports, _, _ = golden_run
    assert len(reports) == 4
    run = np.minimum.accumulate(np.array(saved), axis=0)
    # a restart array is a float32 of the value in bar, like PRESSURE; the report states are saved states
    for k in range(1, 6):
        r = eclio.read_restart(base, k)
        assert "PRESROCK" in r
        i = max(j for j in range(len(saved)) if np.array_equal((saved[j] / BAR).astype(np.float32), np.asarray(r["PRESSURE"], np.float32)))
        assert np.array_equal(np.asarray(r["PRESROCK"], np.float32), (run[i] / BAR).astype(np.float32)), k
    end = eclio.read_restart(base, 5)
    above = np.asarray(end["PRESSURE"], float) - np.asarray(end["PRESROCK"], float)
    print("cells more than 1 bar above their PRESROCK at the end: %d of %d (largest %.1f bar)" % ((above > 1.0).sum(), above.size, above.max()))
    assert (above > 1.0).sum() >= 10                                                   # the deck's precondition: it depletes, then recovers


def test_golden_deck_revers_variant_and_restart(golden_run):
    base, _, _, base_r, base_s = golden_run
    bad = eclio.compare(base, base_r)
    assert any(kind == "UNSMRY" and name.startswith("FPR") for kind, name, _, _, _ in bad), bad       # REVERS ends at another field pressure
    fa = [x[2] for x in eclio.read_arrays(base + ".UNSMRY") if x[0] == "PARAMS"][-1]
    fb = [x[2] for x in eclio.read_arrays(base_r + ".UNSMRY") if x[0] == "PARAMS"][-1]
    kw = [str(k).strip() for k in {x[0]: x[2] for x in eclio.read_arrays(base + ".SMSPEC")}["KEYWORDS"]]
    i = kw.index("FPR")
    print("final FPR: IRREVERS %.3f bar, REVERS %.3f bar" % (fa[i], fb[i]))
    assert abs(fa[i] - fb[i]) > 2e-2 and abs(fa[i] - fb[i]) > 1e-5 * max(abs(fa[i]), abs(fb[i]))
    # the run restarted from report 2 reproduces the full one (the restart file carries PRESROCK)
    assert eclio.compare(base, base_s, by_seqnum=True, summary=False, restart_keywords=("PRESSURE", "SWAT", "SGAS", "RS", "RV", "PRESROCK")) == []
