"""GPU: DRSDT / DRVDT on the device (the rule: include/opmgpu.h at opmgpu_set_dissolution_limits; restated in drsdt_reference.py).

  1  the caps kernel at 1, 63, 64, 65, 255, 256, 257 cells, both options, both rates, bit for bit (one thread per cell on a grid sized by
     the cell count: the kernel has no grid cap, so there is no size past one)
  2  the capped evaluator slot by slot on the edge-case cells through k_perf_props, k_simulator_data and k_assemble_rows (tables in LDS and,
     the regions repeated, read from the blob), caps at 0.3 / 0.9 (binding) and 1.1 / +inf (not binding) of the reference's saturated ratios
  3  the state update with caps against the NumPy restatement
  4  limits switched off again give the bits of a context that never had them; limits that never bind meet the oracle
  5  one converged time step under DRSDT 0: no cell's rs above its cap
  6  persistence (save / restore, device wells, host wells, precision, a failed sub-step) and every OPMGPU_EINVAL
  7  tests/golden/decks/DRSDT_SMALL.DATA through the report-step driver

Tolerance of 2: test_gpu_cell_edges.py's -- per (property, slot) and group of cells 8 times the oracle's error on the same cells WITHOUT
caps, floor 64 ulp.  A cell whose oil is capped while gas is free evaluates the undersaturated oil table, the branch of the OIL_ONLY
cells: its oil slots are held to the larger of its own group's limit and the "oil" group's (its own group's still bounds the
saturation-function part of a mobility, the other the PVT part); a cell whose gas is capped while oil is free likewise with the "gas"
group.  Measured on the MI355X: DESIGN section 7a."""
import os

import numpy as np
import pytest

import cell_edge_cases as E
import cell_reference as R
import drsdt_reference as D
from opmgpu import capi, decks, partition, wells as W
from opmgpu.model import GpuBlackoilModel, newton_step
from util import OracleBackend, rel_err, slot_err

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DECK = os.path.join(HERE, "golden", "decks", "DRSDT_SMALL.DATA")
MARGIN, FLOOR = 8.0, 64 * 2.0 ** -52          # test_gpu_cell_edges.py's
DT = 3 * decks.DAY
COPIES = 10                                   # repeated regions: a table blob past the 24 KiB that fit in LDS
FRACS = (0.3, 0.9, 1.1, float("inf"))
OIL_SLOTS = ("b_o", "mu_o", "rho_o", "mob_o", "rs", "rsSat", "accum_o", "accum_g")
GAS_SLOTS = ("b_g", "mu_g", "rho_g", "mob_g", "rv", "rvSat", "accum_o", "accum_g")


# ---------------------------------------------------------------- 1
def _loose_grid(nc):
    return decks.GridData(nc, np.zeros((0, 2), np.int32), np.zeros(0), np.full(nc, 50.0), np.full(nc, 2000.0))


@pytest.mark.parametrize("nc", [1, 63, 64, 65, 255, 256, 257])
def test_caps_kernel_bit_for_bit(gpu_lib, nc):
    rng = np.random.default_rng(nc)
    sg = np.where(rng.random(nc) < 0.4, 0.0, rng.random(nc) * 0.3)
    if nc > 1:
        sg[0], sg[-1] = 0.0, 0.2
    st = decks.State(rng.uniform(150, 250, nc) * decks.BAR, np.stack([np.full(nc, 0.2), 0.8 - sg, sg], 1), rng.uniform(10, 150, nc), rng.uniform(0, 4e-4, nc),
                     np.full(nc, capi.HC_GAS_AND_OIL, np.int8))
    m = GpuBlackoilModel(_loose_grid(nc), decks.satfunc_standard_tables(), capi.default_params())
    dt = 3.7 * decks.DAY
    for drsdt, free_only, drvdt in ((2.5e-7, False, 1e-12), (2.5e-7, True, None), (0.0, True, 3e-13), (None, False, 1e-12), (0.0, False, None)):
        m.setDissolutionLimits(drsdt, free_only, drvdt)
        m.prepareStep(dt, st)
        got = m.dissolutionCaps()
        want = D.caps(st, dt, drsdt, free_only, drvdt)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (drsdt, free_only, drvdt)
        if free_only and nc > 1:
            assert np.isinf(got[0][0]) and np.isfinite(got[0][-1])
    m.setDissolutionLimits()                                                   # off: no caps
    assert m.dissolution_limits is None and all(np.all(np.isinf(c)) for c in m.dissolutionCaps())
    m.close()


# ---------------------------------------------------------------- 2
@pytest.fixture(scope="module")
def edge(oracle):
    """the edge-case sets and, per set, the oracle's error table on the cells WITHOUT caps {hc group: err[23][4]}: the yardstick"""
    sets, _ = E.load()
    names = R.NAMES[:oracle.NPROP]
    return sets, {ts: E.error_table(C, E.oracle_props(oracle, C), names) for ts, C in sets.items()}


_capped = {}


def capped(C, frac):
    """(rs_cap, rv_cap, ref[nc][26][4], branch records) of a set with caps at frac of the reference's saturated ratios"""
    key = (C.tset, frac)
    if key not in _capped:
        rs_cap, rv_cap = frac * C.ref[:, R.NAMES.index("rsSat"), 0], frac * C.ref[:, R.NAMES.index("rvSat"), 0]
        if not np.isfinite(frac):
            rs_cap, rv_cap = np.full(C.nc, np.inf), np.full(C.nc, np.inf)
        ref, recs = D.cells(C.tab, C.pvtnum, C.satnum, C.state, C.so_max, rs_cap, rv_cap)
        binding = frac < 1.0
        ncap = sum(r["capped_s"] for r in recs) + sum(r["capped_v"] for r in recs)
        assert (ncap > 0) if binding else (ncap == 0 and np.array_equal(ref, C.ref)), (key, ncap)
        _capped[key] = (rs_cap, rv_cap, ref, recs)
    return _capped[key]


def limits(C, yard, names, slots):
    """test_gpu_cell_edges.limits: {group: limit[len(names)][len(slots)]} from the oracle's error table, capped at the oracle's own bound"""
    cap = E.oracle_limits(C, R.NAMES[:23])
    yard = {g: np.minimum(yard[g], cap[g]) for g in yard}
    out = {}
    for g in yard:
        rows = []
        for n in names:
            src = yard["gas+oil"] if n in ("rsSat", "rvSat") and "gas+oil" in yard else yard[g]
            rows.append(src[R.NAMES.index({"rsSat": "rs", "rvSat": "rv"}.get(n, n))][list(slots)])
        out[g] = np.maximum(MARGIN * np.array(rows), FLOOR)
    return out


def check(C, frac, got, names, yard, what, slots=(0, 1, 2, 3)):
    """the error of every (property, slot) over each group of cells against its limit (module docstring); returns the worst error / limit"""
    _, _, ref, recs = capped(C, frac)
    lim = limits(C, yard, names, slots)
    k = [R.NAMES.index(n) for n in names]
    cs = np.array([r["capped_s"] and r["hc"] != R.OIL_ONLY for r in recs])
    cv = np.array([r["capped_v"] and r["hc"] != R.GAS_ONLY for r in recs])
    worst = 0.0
    for g, idx in E.hc_groups(C).items():
        if not idx.size:
            continue
        for j, n in enumerate(names):
            # the cells of the group by the branch their slot evaluates
            other_s = cs[idx] & (n in OIL_SLOTS) & ("oil" in lim)
            other_v = cv[idx] & (n in GAS_SLOTS) & ("gas" in lim)
            for part, extra in ((~other_s & ~other_v, ()), (other_s & ~other_v, ("oil",)), (~other_s & other_v, ("gas",)), (other_s & other_v, ("oil", "gas"))):
                sub = idx[part]
                if not sub.size:
                    continue
                r = ref[sub][:, k[j]][:, list(slots)]
                d, s = np.abs(np.asarray(got)[sub][:, j] - r).max(0), np.abs(ref[idx][:, k[j]][:, list(slots)]).max(0)      # (normalised over the whole group, as there)
                err = np.where(s > 0, d / np.where(s > 0, s, 1.0), np.where(d > 0, np.inf, 0.0))
                bound = np.maximum.reduce([lim[g][j]] + [lim[e][j] for e in extra])
                worst = max(worst, float((err / bound).max()))
                assert np.all(err <= bound), (what, g, extra, n, [R.SLOTS[q] for q in slots], err, bound)
    print("%s: worst error / limit %.3f" % (what, worst))
    return worst


def model_of(C, grid, tab, frac, wells=None):
    m = GpuBlackoilModel(grid, tab, capi.default_params(), wells=wells)
    m.setDissolutionLimits(0.0, False, 0.0)
    m.prepareStep(DT, C.state)
    if tab.vap1 > 0.0 or tab.vap2 > 0.0:
        m.setSatOilMax(C.so_max)
    rs_cap, rv_cap, _, _ = capped(C, frac)
    m.setDissolutionCaps(rs_cap, rv_cap)
    got = m.dissolutionCaps()
    assert np.array_equal(got[0], rs_cap) and np.array_equal(got[1], rv_cap)
    return m


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("tset", E.TSETS)
def test_perf_props_and_simulator_data_with_caps(gpu_lib, edge, tset, frac):
    """k_perf_props (one well through every cell) and k_simulator_data (eval_cell<OUTPUT>: RSSAT / RVSAT are the effective ratios)"""
    sets, yard = edge
    C = sets[tset]
    m = model_of(C, C.grid(), C.tab, frac, wells=(np.array([0, C.nc], np.int32), np.arange(C.nc, dtype=np.int32)))
    m.assemble(True)
    pp = m.perfProps(C.nc).reshape(C.nc, 9, 4)
    d = m.simulatorData()
    m.close()
    check(C, frac, pp, ["p_o", "rs", "rv", "b_w", "b_o", "b_g", "mob_w", "mob_o", "mob_g"], yard[tset], "perfProps %s %.1f" % (tset, frac))
    pairs = [("1OVERBW", "b_w"), ("1OVERBO", "b_o"), ("1OVERBG", "b_g"), ("WAT_DEN", "rho_w"), ("OIL_DEN", "rho_o"), ("GAS_DEN", "rho_g"),
             ("WAT_VISC", "mu_w"), ("OIL_VISC", "mu_o"), ("GAS_VISC", "mu_g"), ("WATKR", "kr_w"), ("OILKR", "kr_o"), ("GASKR", "kr_g"),
             ("RSSAT", "rsSat"), ("RVSAT", "rvSat")]
    got = np.stack([d[k] for k, _ in pairs], 1)[:, :, None]
    check(C, frac, got, [n for _, n in pairs], yard[tset], "simulatorData %s %.1f" % (tset, frac), slots=(0,))
    if frac < 1.0:        # the effective ratio of a capped cell is the cap itself, to the bit
        rs_cap, rv_cap, _, recs = capped(C, frac)
        ks, kv = np.array([r["capped_s"] for r in recs]), np.array([r["capped_v"] for r in recs])
        assert np.array_equal(d["RSSAT"][ks], rs_cap[ks]) and np.array_equal(d["RVSAT"][kv], rv_cap[kv])


@pytest.mark.parametrize("blob", [False, True], ids=["lds", "blob"])
@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("tset", E.TSETS)
def test_isolated_cell_assembly_with_caps(gpu_lib, edge, tset, frac, blob):
    """k_assemble_rows on a grid without connections, as test_gpu_cell_edges.py reads it: the diagonal block of a cell is
    matbalscale[a] * pv/dt * d accum_a / d(p, Sw, X), its residual pv/dt * (accum_a - accum0_a) -- after assemble(True) and, the cells'
    states and caps shifted within their groups, after assemble(False); tables in LDS and read from the blob"""
    sets, yard = edge
    C = sets[tset]
    copies = COPIES if blob else 1
    tab, grid = (E.tables(tset, copies), C.grid(copies)) if blob else (C.tab, C.grid())
    names = ["accum_w", "accum_o", "accum_g"]
    rs_cap, rv_cap, ref, _ = capped(C, frac)
    acc = ref[:, [R.NAMES.index(n) for n in names]]
    scale = np.asarray(capi.default_params().matbalscale[:])
    pvdt = np.asarray(grid.pv) / DT
    f = scale[None, :, None] * pvdt[:, None, None]
    st2, so_max2, perm = C.shifted()
    m = model_of(C, grid, tab, frac)
    for initial, src in ((True, np.arange(C.nc)), (False, perm)):           # cell i holds the state (and the caps) of cell src[i]
        def at_source(a):
            out = np.empty_like(a)
            out[src] = a
            return out
        if not initial:
            m.setState(st2)
            if tset == "vap":
                m.setSatOilMax(so_max2)
            m.setDissolutionCaps(rs_cap[perm], rv_cap[perm])
        m.assemble(initial)
        rowptr, col, val = m.jacobian()
        assert np.array_equal(col, np.arange(C.nc)) and np.array_equal(rowptr, np.arange(C.nc + 1))
        tag = "%s %.1f %s assemble(%s)" % (tset, frac, "blob" if blob else "lds", initial)
        check(C, frac, at_source(val.reshape(-1, 3, 3) / f), names, yard[tset], "Jacobian " + tag, slots=(1, 2, 3))
        excess = m.residual().reshape(3, C.nc).T / pvdt[:, None] - (acc[src][:, :, 0] - acc[:, :, 0])
        check(C, frac, (acc[:, :, 0] + at_source(excess))[:, :, None], names, yard[tset], "residual " + tag, slots=(0,))
    m.close()


# ---------------------------------------------------------------- 3
def test_update_state_with_caps(gpu_lib):
    """the grid, states and increments of test_gpu_assembly.py::test_update_state_parity, caps at the state's rs / rv times U(0.5, 1.5)
    (drsdt_reference.update_cases); hc exactly, values at that test's tolerances; cells whose switching comparison is within 1e-9
    (relative) of a tie are left out, at most 1 % (test_drsdt_reference.py holds the restatement to that on the CPU)"""
    for tab, grid, prm, st, dx, rs_cap, rv_cap in D.update_cases():
        zero = np.zeros(grid.nc, np.int32)
        o, margin = D.update_state(tab, zero, zero, prm, dx, st, rs_cap, rv_cap, with_margins=True)
        keep = margin >= 1e-9
        assert (~keep).mean() <= 0.01
        m = GpuBlackoilModel(grid, tab, prm)
        m.setDissolutionLimits(0.0, False, 0.0)
        m.prepareStep(decks.DAY, st)
        m.setDissolutionCaps(rs_cap, rv_cap)
        m.updateState(dx)
        g = m.getState()
        m.close()
        assert np.array_equal(g.hc[keep], o.hc[keep])
        assert np.allclose(g.p[keep], o.p[keep], rtol=1e-14, atol=0) and np.allclose(g.sat[keep], o.sat[keep], rtol=0, atol=1e-14)
        assert np.allclose(g.rs[keep], o.rs[keep], rtol=1e-13, atol=1e-13) and np.allclose(g.rv[keep], o.rv[keep], rtol=1e-13, atol=1e-18)


# ---------------------------------------------------------------- 4
def test_limits_switched_off_give_the_bits_of_no_limits(gpu_lib):
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(7, 6, 5, lognormal_sigma=0.7)
    st, st2 = decks.random_state(grid, tab, seed=1), decks.random_state(grid, tab, seed=11)
    st2.hc[:] = st.hc
    out = []
    for with_limits in (False, True):
        m = GpuBlackoilModel(grid, tab, capi.default_params())
        if with_limits:
            m.setDissolutionLimits(0.0, False, 0.0)
            m.prepareStep(DT, st)
            m.assemble(True)
            capped_jac = m.jacobian()[2]
            m.setDissolutionLimits()
        m.prepareStep(DT, st)
        m.assemble(True)
        a = (m.jacobian()[2], m.residual())
        m.setState(st2)
        m.assemble(False)
        m.updateState(np.full(3 * grid.nc, 1e-3))
        g = m.getState()
        out.append(a + (m.jacobian()[2], m.residual(), g.p, g.sat, g.rs, g.rv, g.hc))
        m.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    assert not np.array_equal(capped_jac, out[0][0])                           # (with the limits on, the assembly was another one)


@pytest.mark.parametrize("name", ["cart", "wells"])
def test_limits_that_never_bind_meet_the_oracle(gpu_lib, oracle, name):
    """limits on (the KM_DRDT instantiations run) with rates so large that no cap binds: test_gpu_assembly.py's cases at its RTOL_JAC"""
    from test_gpu_assembly import RTOL_JAC, _cases
    tab = decks.satfunc_standard_tables()
    prm = capi.default_params()
    scale = tuple(prm.matbalscale)
    (_, grid, wells), = [c for c in _cases() if c[0] == name]
    for seed in (1, 2):
        st = decks.random_state(grid, tab, seed=seed)
        m = GpuBlackoilModel(grid, tab, prm, wells=wells)
        m.setDissolutionLimits(1e3, False, 1e3)
        m.prepareStep(DT, st)
        assert all(np.all(c > 1e8) for c in m.dissolutionCaps())
        m.assemble(True)
        rowptr, col = oracle.pattern(grid, *(wells or (None, None)))
        r0, v0, acc0, _ = oracle.assemble(grid, tab, DT, st, rowptr, col, scale=scale)
        gr, gc, gv = m.jacobian()
        assert np.array_equal(gr, rowptr) and np.array_equal(gc, col)
        assert rel_err(gv, v0) < RTOL_JAC and slot_err(gv, v0) < RTOL_JAC and rel_err(m.residual(), r0) < RTOL_JAC
        st2 = decks.random_state(grid, tab, seed=seed + 10)
        st2.hc[:] = st.hc
        m.setState(st2)
        m.assemble(False)
        r1, v1, _, _ = oracle.assemble(grid, tab, DT, st2, rowptr, col, scale=scale, accum0=acc0)
        gv1 = m.jacobian()[2]
        assert rel_err(gv1, v1) < RTOL_JAC and slot_err(gv1, v1) < RTOL_JAC and rel_err(m.residual(), r1) < RTOL_JAC
        m.close()


# ---------------------------------------------------------------- 5
def _gas_over_oil(grid, tab):
    """free gas at its saturated ratios in the top layer over undersaturated oil (rs at 0.6 of the curve), pressures scattered over 25 bar:
    gas re-dissolves wherever the pressure of a gas-bearing cell rises or gas reaches an undersaturated cell"""
    nx, ny, nz = grid.dims
    nc = grid.nc
    k = np.arange(nc) // (nx * ny)
    p = (180 + 25 * np.random.default_rng(8).random(nc)) * decks.BAR
    sw = np.full(nc, 0.2)
    sg = np.where(k == 0, 0.25, 0.0)
    hc = np.where(sg > 0, capi.HC_GAS_AND_OIL, capi.HC_OIL_ONLY).astype(np.int8)
    T = R.Tables(tab)
    rs_sat = D._pvt_lin(T.oil(0)["psat"], T.oil(0)["rs"], p)
    rv_sat = D._pvt_lin(T.gas(0)["pg"], T.gas(0)["rv"], p + D._sat_right(T.sat(0)["sg"], T.sat(0)["pcgo"], sg))
    return decks.State(p, np.stack([sw, 1 - sw - sg, sg], 1), np.where(sg > 0, rs_sat, 0.6 * rs_sat), np.where(sg > 0, rv_sat, 0.0), hc)


@pytest.fixture(scope="module")
def drsdt_zero_step(oracle):
    """the step of 5: (cells whose rs rises without limits -- the CPU oracle, run first --, Newton iterations of the device under
    DRSDT 0, its verdict, the caps, the state it ends in)"""
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(6, 5, 4, lognormal_sigma=0.3)
    st = _gas_over_oil(grid, tab)
    prm = capi.default_params(linear_solver_reduction=1e-8, linear_solver_maxiter=300)
    dt = 2 * decks.DAY
    ob = OracleBackend(oracle, grid, tab, prm)
    ob.prepareStep(dt, st)
    for it in range(12):
        ob.assemble(it == 0)
        if ob.getConvergence() and it > 0:
            break
        ob.solveJacobianSystem()
        ob.updateState()
    else:
        pytest.fail("the oracle did not converge the step without limits")
    rises = int((ob.getState().rs > st.rs * (1 + 1e-12)).sum())
    m = GpuBlackoilModel(grid, tab, prm)
    m.setDissolutionLimits(0.0)
    m.prepareStep(dt, st)
    cap = m.dissolutionCaps()[0]
    assert np.array_equal(cap, st.rs)
    its, _ = newton_step(m, max_iter=15)
    conv = m.getConvergence()
    e = m.getState()
    m.close()
    print("without limits rs rises in %d of %d cells; DRSDT 0: converged in %d iterations, %d cells on their cap" % (rises, grid.nc, its, int((e.rs == cap).sum())))
    return rises, its, conv, cap, e


def test_a_converged_step_under_drsdt_zero_holds_every_cap(drsdt_zero_step):
    """Free gas over undersaturated oil, one time step solved to convergence under DRSDT 0: getConvergence passes and EVERY cell ends
    with rs <= rs_cap.  Without limits (the CPU oracle, run first) the same step raises rs in 72 of the 120 cells, by up to 17.5 sm3/sm3
    -- the count when this test was written; the test asks for at least one.
    The cells that decide this check are the OIL_ONLY ones, whose rs is the primary variable: the switching logic frees their gas only
    past rs > RsSat (1 + 1.49e-8) with the previous rs already within that factor, so the state update limits a cell it leaves OIL_ONLY
    to its cap (include/opmgpu.h).  Without that limit one cell of this step ended 1.65e-4 above its cap of 55.925."""
    rises, its, conv, cap, e = drsdt_zero_step
    assert rises >= 1 and conv
    assert np.all(e.rs <= cap), ((e.rs - cap).max(), int((e.rs > cap).sum()))


def test_cells_that_end_with_free_gas_hold_their_cap(drsdt_zero_step):
    """the same step: a cell that ends it with free gas has the capped saturated ratio, so it is on or below its cap to the bit, and
    gas that may not re-dissolve keeps cells on it"""
    rises, its, conv, cap, e = drsdt_zero_step
    gas = e.hc != capi.HC_OIL_ONLY
    assert conv and gas.any() and np.all(e.rs[gas] <= cap[gas]) and (e.rs[gas] == cap[gas]).any()


# ---------------------------------------------------------------- 6
def _wells(g):
    nx, ny, nz = g.dims
    colm = lambda i, j: [i + nx * j + nx * ny * k for k in range(nz)]      # noqa: E731
    WI = 5.0 * float(np.median(g.trans))
    wl = W.Wells()
    wl.add_well("INJ", W.INJECTOR, g.z[colm(0, 0)[0]], colm(0, 0), WI, (0.0, 0.0, 1.0), (W.SURFACE_RATE, 300.0 / 86400.0, (0.0, 0.0, 1.0)),
                limits=[(W.BHP, 600 * decks.BAR)])
    wl.add_well("P1", W.PRODUCER, g.z[colm(nx - 1, ny - 1)[0]], colm(nx - 1, ny - 1)[:3], WI, (0.0, 1.0, 0.0), (W.BHP, 150 * decks.BAR), limits=[])
    return wl


def test_limits_and_caps_persist(gpu_lib):
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(6, 5, 4, lognormal_sigma=0.3)
    st = decks.random_state(grid, tab, seed=3)
    lim = (2e-7, True, 1e-12)
    dt = 4 * decks.DAY
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    m.setDissolutionLimits(*lim)
    m.prepareStep(dt, st)
    c0 = m.dissolutionCaps()
    want = D.caps(st, dt, *lim)
    assert np.array_equal(c0[0], want[0]) and np.array_equal(c0[1], want[1]) and np.isinf(c0[0]).any() and np.isfinite(c0[0]).any()

    def same_caps():
        c = m.dissolutionCaps()
        return np.array_equal(c[0], c0[0]) and np.array_equal(c[1], c0[1])
    # save / restore do not touch the caps
    m.saveState()
    rng = np.random.default_rng(1)
    dx = np.concatenate([rng.standard_normal(grid.nc) * 5 * decks.BAR, rng.standard_normal(grid.nc) * 0.05, rng.standard_normal(grid.nc) * 0.05])
    m.updateState(dx)
    moved = m.getState()
    assert not np.array_equal(moved.rs, st.rs) and same_caps()
    m.restoreState()
    back = m.getState()
    assert np.array_equal(back.rs, st.rs) and np.array_equal(back.sat, st.sat) and same_caps()
    # a failed sub-step: the state restored, a shorter dt: the caps follow from the restored state
    m.prepareStep(dt / 4)
    w4 = D.caps(st, dt / 4, *lim)
    c4 = m.dissolutionCaps()
    assert np.array_equal(c4[0], w4[0]) and np.array_equal(c4[1], w4[1])
    m.prepareStep(dt)
    assert same_caps()
    # a change of the solve precision
    for single in (True, False):
        m.setSolvePrecision(single)
        m.assemble(True)
        assert same_caps() and m.dissolution_limits == lim
    jac = m.jacobian()[2]
    # a re-plan: host wells, then device wells
    m.setWells(np.array([0, 3], np.int32), np.array([2, 32, 62], np.int32))
    assert same_caps()
    m.setWells(np.array([0], np.int32), np.zeros(0, np.int32))
    m.setSolvePrecision(False)
    m.assemble(True)
    assert np.array_equal(m.jacobian()[2], jac)                                 # the same capped assembly after two re-plans
    wl = _wells(grid)
    md = W.DeviceWellModel(m, wl, W.WellState(wl, st.p))
    assert same_caps()
    md.prepareStep(dt / 4)                                                      # the wrapper forwards prepareStep: the limits are still in force
    c4 = m.dissolutionCaps()
    assert np.array_equal(c4[0], w4[0]) and np.array_equal(c4[1], w4[1])
    # the caps themselves, either plane alone (restart)
    m.setDissolutionCaps(rs_cap=c0[0])
    c = m.dissolutionCaps()
    assert np.array_equal(c[0], c0[0]) and np.array_equal(c[1], w4[1])
    m.setDissolutionCaps(rv_cap=c0[1])
    assert same_caps()
    m.close()


def test_every_refusal_leaves_the_previous_limits(gpu_lib, monkeypatch):
    import pvcdo_cases as cases
    from opmgpu import deck as deckmod
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(5, 4, 3)
    st = decks.random_state(grid, tab, seed=2)
    lim = (3e-7, False, 2e-12)
    m = GpuBlackoilModel(grid, tab, capi.default_params())
    m.setDissolutionLimits(*lim)
    m.prepareStep(decks.DAY, st)
    c0 = m.dissolutionCaps()

    def unchanged():
        c = m.dissolutionCaps()
        return m.dissolution_limits == lim and np.array_equal(c[0], c0[0]) and np.array_equal(c[1], c0[1])
    for bad in ((float("nan"), False, None), (float("inf"), False, None), (None, False, float("nan")), (0.0, False, float("inf"))):
        with pytest.raises(ValueError, match="opmgpu_set_dissolution_limits.*not finite"):
            m.setDissolutionLimits(*bad)
        assert unchanged()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert gpu_lib.opmgpu_begin_dissolution_step(m.ctx, bad) == capi.EINVAL
        assert b"dt" in gpu_lib.opmgpu_last_error(m.ctx) and unchanged()
    with pytest.raises(ValueError, match="dissolution limits"):                 # PVCDO refuses a context with limits
        m.setPvcdo(np.array([[2e7, 1.1, 1e-9, 1e-3, 0.0]]))
    assert unchanged()
    # the previous limits are still what the device runs: the same step gives the same caps
    m.prepareStep(decks.DAY)
    assert unchanged()
    m.close()
    # without dissolved gas / vaporised oil; the analytic dead oil; no gas phase
    own, twin = cases.tables("default")
    g = cases.grid()
    for t, args, match in ((twin, (0.0, False, None), "drsdt needs dissolved gas"), (twin, (None, False, 0.0), "drvdt needs vaporised oil"),
                           (own, (None, False, 0.0), "analytic dead oil")):
        mm = GpuBlackoilModel(g, t, capi.default_params())
        with pytest.raises(ValueError, match=match):
            mm.setDissolutionLimits(*args)
        assert mm.dissolution_limits is None and all(np.all(np.isinf(c)) for c in mm.dissolutionCaps())
        assert gpu_lib.opmgpu_begin_dissolution_step(mm.ctx, 1.0) == capi.EINVAL          # no limits: nothing to begin
        with pytest.raises(ValueError, match="no dissolution limit"):
            mm.setDissolutionCaps(np.zeros(g.nc))
        mm.close()
    d = deckmod.read_deck(os.path.join(HERE, "golden", "decks", "OILWATER_SMALL.DATA"))
    mm = GpuBlackoilModel(d.grid(), d.tables(), capi.default_params())
    with pytest.raises(ValueError, match="no gas phase"):
        mm.setDissolutionLimits(0.0)
    mm.close()
    # a communicator: attached first, and attached later
    monkeypatch.setenv("OPMGPU_COMM_TRANSPORT", "shm")
    nc = grid.nc
    src = np.concatenate([np.arange(nc), [0]])
    grid_b = decks.GridData(nc + 1, grid.conn_cells, grid.trans, grid.pv[src], grid.z[src])

    class Dom:
        n_owned, neigh_rank, send_ptr, send_cells = nc, capi.i32([0]), capi.i32([0, 1]), capi.i32([0])
        recv_ptr, recv_cells = capi.i32([0, 1]), capi.i32([nc])
    mm = GpuBlackoilModel(grid_b, tab, capi.default_params())
    partition.attach_comm(mm, Dom, 0, 1, partition.make_unique_id())
    with pytest.raises(ValueError, match="opmgpu_set_dissolution_limits: a communicator is attached"):
        mm.setDissolutionLimits(0.0)
    assert mm.dissolution_limits is None
    mm.close()
    mm = GpuBlackoilModel(grid_b, tab, capi.default_params())
    mm.setDissolutionLimits(*lim)
    with pytest.raises(ValueError, match="DRSDT / DRVDT"):                      # opmgpu/partition.py
        partition.attach_comm(mm, Dom, 0, 1, partition.make_unique_id())
    kept, mm.dissolution_limits = mm.dissolution_limits, None                  # past the Python check: the library's own
    with pytest.raises(Exception, match="dissolution limits"):
        partition.attach_comm(mm, Dom, 0, 1, partition.make_unique_id())
    mm.dissolution_limits = kept
    assert gpu_lib.opmgpu_comm_set_pressure_hierarchy(mm.ctx, 0) == capi.EINVAL  # refused before anything was attached
    stb = decks.State(st.p[src], st.sat[src], st.rs[src], st.rv[src], st.hc[src])
    mm.prepareStep(decks.DAY, stb)
    want = D.caps(stb, decks.DAY, *lim)
    assert np.array_equal(mm.dissolutionCaps()[0], want[0])
    mm.close()


# ---------------------------------------------------------------- 7
@pytest.fixture(scope="module")
def golden_run(gpu_lib):
    """DRSDT_SMALL.DATA through the report-step driver, two report steps: per prepareStep (dt, the limits in force, the state, rs_cap),
    and the state the run ends in"""
    from opmgpu.simulator import Simulator
    log = []

    class Recording(GpuBlackoilModel):
        def prepareStep(self, dt, state=None):
            super().prepareStep(dt, state)
            if self.dissolution_limits is not None:
                log.append((float(dt), self.dissolution_limits, self.getState(), self.dissolutionCaps()[0]))

    sim = Simulator(DECK, model_factory=lambda grid, tables, params: Recording(grid, tables, params))
    reports = sim.run()
    end = sim.model.getState()
    sim.close()
    first = [l for l in log if l[1][0] == 0.0]
    print("sub-steps: %d under DRSDT 0, %d under DRSDT 1e-3 FREE; newton %s" % (len(first), len(log) - len(first), [r["newton"] for r in reports]))
    return reports, log, end


def _substeps(log, end):
    return zip(log, [l[2] for l in log[1:]] + [end])


def test_report_step_driver_installs_the_limits_and_caps(golden_run):
    """the limits of each report step are in force before its first sub-step, every sub-step's caps are the restatement's, the injector
    does make free gas, and a cell that ends a sub-step with free gas is on or below its cap to the bit"""
    reports, log, end = golden_run
    assert len(reports) == 2 and log[0][1] == (0.0, False, None) and log[-1][1] == (1e-3 / decks.DAY, True, None)
    n_free = 0
    for (dt, (a_s, free_only, _), st, cap), nxt in _substeps(log, end):
        want = D.caps(st, dt, a_s, free_only, None)[0]
        assert np.array_equal(cap, want)
        assert np.isfinite(cap).all() or free_only
        gas = (nxt.hc != capi.HC_OIL_ONLY) & np.isfinite(cap)
        assert np.all(nxt.rs[gas] <= cap[gas])
        n_free += int((st.sat[:, 2] > 0).sum())
    assert (end.sat[:, 2] > 0).any() and n_free > 0


def test_report_step_driver_on_the_golden_deck(golden_run):
    """DRSDT 0: rs rises in no cell over any sub-step of the first report step; DRSDT 1e-3 FREE: in the cells that held free gas at the
    begin of a sub-step it rises by at most a_s dt.  Relative slack 1e-12.  (Without the state update's limit on cells left OIL_ONLY the
    rs of cells far from both wells drifted from 70 to 70 + 2.4e-10 over the first sub-step: the noise of a linear solve in a primary
    variable, inside the factor 1 + 1.49e-8 the switching logic tolerates.)"""
    reports, log, end = golden_run
    slack = 1 + 1e-12
    for (dt, (a_s, free_only, _), st, cap), nxt in _substeps(log, end):
        held = np.isfinite(cap)
        assert np.all(nxt.rs[held] <= cap[held] * slack), (a_s, dt, float((nxt.rs[held] / cap[held] - 1).max()))
