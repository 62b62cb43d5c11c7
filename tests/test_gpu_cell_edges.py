"""The device's cell evaluator (eval_cell, csrc/fluid_eval.hpp) slot by slot on the edge-case cells (cell_edge_cases.py): the three
kernels that hand its results out -- k_perf_props, k_simulator_data (the OUTPUT instantiation), k_assemble_rows -- against the 50-digit
reference (cell_reference.py), and the assembly of the same cells on a connected grid against the oracle, per Jacobian slot.

Tolerance against the reference: the error of a (property, slot), max |device - ref| / max |ref| over the cells of one group
(cell_edge_cases.hc_groups: a hydrocarbon state, the cells that divide by a blend argument below 2 eps apart), may be at most MARGIN = 8
times the ORACLE's error in that (property, slot) (a few 1e-16; counted at no more than the bound test_cell_reference.py holds the
oracle to, so that this file stands alone), with a floor of 64 ulp = 1.4e-14.  The margin is for the Newton path's documented
arithmetic -- a reciprocal and a multiplication where the oracle divides, slopes formed on the host, FMA contraction: one more rounding
in each of about ten chained operations.
Measured on the MI355X (worst slot of each test): see DESIGN section 7a."""
import numpy as np
import pytest

import cell_edge_cases as E
import cell_reference as R
from opmgpu import capi, decks
from opmgpu.model import GpuBlackoilModel
from util import slot_err

pytestmark = pytest.mark.gpu

RTOL_JAC = 1e-11                # test_gpu_assembly.py's, here per slot
MARGIN, FLOOR = 8.0, 64 * 2.0 ** -52
DT = 3 * decks.DAY
COPIES = 10                     # repeated regions: a table blob past the 24 KiB that fit in LDS


@pytest.fixture(scope="module")
def edge(oracle):
    """the edge-case sets and, per set, the oracle's error table {hc group: err[23][4]}: the yardstick"""
    sets, _ = E.load()
    names = R.NAMES[:oracle.NPROP]
    return sets, {ts: E.error_table(C, E.oracle_props(oracle, C), names) for ts, C in sets.items()}


def limits(C, yard, names, slots=(0, 1, 2, 3)):
    """{group: limit[len(names)][len(slots)]} from the oracle's error table of one set, capped at the oracle's own bound.  rsSat / rvSat,
    which the oracle does not list, take the limit of rs / rv with free gas and oil, where those ARE the saturated ratios."""
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


def check(C, got, names, yard, what, slots=(0, 1, 2, 3)):
    err, lim = E.error_table(C, got, names, slots), limits(C, yard, names, slots)
    for g in err:
        i, s = np.unravel_index(np.argmax(err[g] / lim[g]), err[g].shape)
        print("%s, '%s': largest error %.2e; nearest its limit: %s %s, %.2e of %.2e" % (what, g, err[g].max(), names[i], R.SLOTS[slots[s]], err[g][i, s], lim[g][i, s]))
        bad = np.argwhere(err[g] > lim[g])
        assert bad.size == 0, [(what, g, names[i], R.SLOTS[slots[s]], err[g][i, s], lim[g][i, s]) for i, s in bad]


def model_of(C, grid, tab, wells=None, state=None, so_max=None, **prm):
    m = GpuBlackoilModel(grid, tab, capi.default_params(**prm), wells=wells)
    m.prepareStep(DT, C.state if state is None else state)
    if tab.vap1 > 0.0 or tab.vap2 > 0.0:
        m.setSatOilMax(C.so_max if so_max is None else so_max)
    return m


@pytest.mark.parametrize("tset", E.TSETS)
def test_perf_props_at_the_edges(gpu_lib, edge, tset):
    """k_perf_props: one well through every cell; p_o, rs, rv, b, mobilities with their derivatives against the reference"""
    sets, yard = edge
    C = sets[tset]
    m = model_of(C, C.grid(), C.tab, wells=(np.array([0, C.nc], np.int32), np.arange(C.nc, dtype=np.int32)))
    m.assemble(True)
    pp = m.perfProps(C.nc).reshape(C.nc, 9, 4)
    m.close()
    check(C, pp, ["p_o", "rs", "rv", "b_w", "b_o", "b_g", "mob_w", "mob_o", "mob_g"], yard[tset], "perfProps " + tset)


@pytest.mark.parametrize("tset", E.TSETS)
def test_simulator_data_at_the_edges(gpu_lib, edge, tset):
    """k_simulator_data (eval_cell<OUTPUT>): 1/B, densities, viscosities, kr, RSSAT, RVSAT against the reference's values"""
    sets, yard = edge
    C = sets[tset]
    m = model_of(C, C.grid(), C.tab)
    d = m.simulatorData()
    m.close()
    pairs = [("1OVERBW", "b_w"), ("1OVERBO", "b_o"), ("1OVERBG", "b_g"), ("WAT_DEN", "rho_w"), ("OIL_DEN", "rho_o"), ("GAS_DEN", "rho_g"),
             ("WAT_VISC", "mu_w"), ("OIL_VISC", "mu_o"), ("GAS_VISC", "mu_g"), ("WATKR", "kr_w"), ("OILKR", "kr_o"), ("GASKR", "kr_g"),
             ("RSSAT", "rsSat"), ("RVSAT", "rvSat")]
    got = np.stack([d[k] for k, _ in pairs], 1)[:, :, None]
    check(C, got, [n for _, n in pairs], yard[tset], "simulatorData " + tset, slots=(0,))


@pytest.mark.parametrize("blob", [False, True], ids=["lds", "blob"])
@pytest.mark.parametrize("tset", E.TSETS)
def test_isolated_cell_assembly_at_the_edges(gpu_lib, edge, tset, blob):
    """k_assemble_rows on a grid without connections: the diagonal block of a cell is matbalscale[a] * pv/dt * d accum_a / d(p, Sw, X) and
    its residual pv/dt * (accum_a - accum0_a) (test_cell_reference.py confirms the mapping on the oracle) -- after assemble(True) and
    after setState + assemble(False), with the tables in LDS and, the regions repeated past 24 KiB, read from the blob.
    The residual over pv/dt is held to the limit of ONE accumulation value, though it is the difference of two."""
    sets, yard = edge
    C = sets[tset]
    copies = COPIES if blob else 1
    tab, grid = (E.tables(tset, copies), C.grid(copies)) if blob else (C.tab, C.grid())
    f64 = sum(a.nbytes for a in vars(tab).values() if isinstance(a, np.ndarray) and a.dtype == np.float64)
    assert f64 > 24 * 1024 if blob else 2 * sum(a.nbytes for a in vars(tab).values() if isinstance(a, np.ndarray)) < 24 * 1024
    names = ["accum_w", "accum_o", "accum_g"]
    acc = C.ref[:, [R.NAMES.index(n) for n in names]]                                      # [nc][3][4]
    scale = np.asarray(capi.default_params().matbalscale[:])
    f = scale[None, :, None] * (np.asarray(grid.pv) / DT)[:, None, None]
    st2, so_max2, perm = C.shifted()
    m = model_of(C, grid, tab)
    pvdt = np.asarray(grid.pv) / DT
    for initial, src in ((True, np.arange(C.nc)), (False, perm)):           # cell i holds the state of cell src[i]
        def at_source(a):
            out = np.empty_like(a)
            out[src] = a
            return out
        if not initial:
            m.setState(st2)
            if tset == "vap":
                m.setSatOilMax(so_max2)
        m.assemble(initial)
        rowptr, col, val = m.jacobian()
        assert np.array_equal(col, np.arange(C.nc)) and np.array_equal(rowptr, np.arange(C.nc + 1))
        tag = "%s %s assemble(%s)" % (tset, "blob" if blob else "lds", initial)
        check(C, at_source(val.reshape(-1, 3, 3) / f), names, yard[tset], "Jacobian " + tag, slots=(1, 2, 3))
        # the residual's (unscaled) excess over pv/dt * (accum - accum0), normalised like an accumulation value
        excess = m.residual().reshape(3, C.nc).T / pvdt[:, None] - (acc[src][:, :, 0] - acc[:, :, 0])
        check(C, (acc[:, :, 0] + at_source(excess))[:, :, None], names, yard[tset], "residual " + tag, slots=(0,))
    m.close()


@pytest.mark.parametrize("ordering", [capi.ORDER_NATURAL, capi.ORDER_MULTICOLOR])
def test_connected_assembly_slot_by_slot(gpu_lib, oracle, ordering):
    """the edge-case cells on a 10 x 10 x 6 grid with gravity: Jacobian and residual against the oracle, every (equation, variable) slot
    and every equation at RTOL_JAC within itself (util.slot_err), first assembly and a second state"""
    C = E.load()[0]["base"]
    grid, st, _ = E.connected(C)
    st2 = decks.State(np.roll(st.p, 7), np.roll(st.sat, 7, axis=0), np.roll(st.rs, 7), np.roll(st.rv, 7), np.roll(st.hc, 7))
    prm = capi.default_params(ilu_ordering=ordering)
    scale = tuple(prm.matbalscale)
    rowptr, col = oracle.pattern(grid)
    m = GpuBlackoilModel(grid, C.tab, prm)
    m.prepareStep(DT, st)
    acc0 = None
    for s in (st, st2):
        if acc0 is not None:
            m.setState(s)
        m.assemble(acc0 is None)
        r, v, acc0, _ = oracle.assemble(grid, C.tab, DT, s, rowptr, col, scale=scale, accum0=acc0)
        gr, gc, gv = m.jacobian()
        assert np.array_equal(gr, rowptr) and np.array_equal(gc, col)
        print("connected, ordering %d: Jacobian slot_err %.2e, residual slot_err %.2e" % (ordering, slot_err(gv, v), slot_err(m.residual(), r)))
        assert slot_err(gv, v) < RTOL_JAC, slot_err(gv, v)
        assert slot_err(m.residual(), r) < RTOL_JAC, slot_err(m.residual(), r)
    m.close()
