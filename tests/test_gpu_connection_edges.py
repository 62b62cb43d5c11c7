"""The connection half of k_assemble_rows (csrc/blackoil.hip) connection by connection on the edge cases of connection_edge_cases.py: upwind
ties, |dh| == thp and one float off it, both listing orders, T == 0 and tiny T, a hub row, leaves and isolated cells -- against
oracle.assemble on oracle.pattern of the same grid, whose rule at a tie is the reference's (dh >= 0 -> c1).

Measure, per connection and (equation, variable) slot: max |device - oracle| over the two off-diagonal blocks (c1, c2) and (c2, c1), which
hold this connection alone, over max |oracle| of the slot in the same two blocks; a slot that is identically zero in the oracle must be
exactly zero on the device.  Diagonal blocks per row and slot, relative to the largest magnitude of the slot among the row's blocks; the
residual per row and equation, relative to the largest of its contributions (the connections' fluxes, pv / dt times the old and the new
accumulation).
Tolerance RTOL_JAC = 1e-11 (double) and RTOL_JAC_F32 = 2e-6 (a float Jacobian), the bounds of test_gpu_assembly.py, here PER CONNECTION:
the condition on the inputs (test_connection_cases.py) bounds the cancellation in dh by 1e3, about ten roundings times that is 2e-12.
Next to the relative bound stands an absolute one for what a number format cannot hold: K.subnormal_floor (products with T == 5e-324 are
multiples of 2^-1074) and, for a float Jacobian, 2^-149 (entries below the float range: those of T == 1e-300).
Measured on the MI355X (worst connection and slot of each test): see DESIGN section 7a."""
import ctypes as C

import numpy as np
import pytest

import connection_edge_cases as K
from opmgpu import capi, decks
from opmgpu.model import GpuBlackoilModel, ISTLError, LinearSolverProblem, NumericalIssue

pytestmark = pytest.mark.gpu

DT = 3 * decks.DAY
SEEDS = (1, 2)
COPIES = 12                      # 24 saturation and 24 PVT regions: a table blob past the 24 KiB that fit in LDS
LDS_BYTES = 24 * 1024
ORDERINGS = {"natural": capi.ORDER_NATURAL, "multicolour": capi.ORDER_MULTICOLOR}
SCALE = tuple(capi.default_params().matbalscale)
F32_FLOOR = 2.0 ** -149
WO_SLOTS = [0, 1, 3, 4]          # water and oil equations, d/dp and d/dSw

_REF = {}


def reference(oracle, kind, variant):
    """per state of SEEDS: the oracle's system on the fixture (first assembly with state 1, second state against its accumulation), and the
    connections' values.  Computed once per (deck, variant), shared and left unchanged."""
    if (kind, variant) not in _REF:
        g = K.grid(variant)
        tab = K.tables() if kind == "wog" else K.twin_wo()
        rowptr, col = oracle.pattern(g)
        out, acc0 = [], None
        for seed in SEEDS:
            st = K.state(seed, kind)
            old = acc0
            r, val, acc0, _ = oracle.assemble(g, tab, DT, st, rowptr, col, scale=SCALE, accum0=acc0)
            props = oracle.cell_props(g, tab, st)
            cv = K.connection_values(g, props)
            acc = props[:, [K.NAMES.index("accum_" + a) for a in "wog"], 0]
            rnorm = K.residual_norms(g, cv, DT) if old is None else K.residual_norms(g, cv, DT, acc, old.reshape(3, -1).T)
            ref = dict(st=st, r=r.reshape(3, -1).T, val=val, blocks=K.connection_blocks(rowptr, col, g.conn_cells, val), cv=cv, rnorm=rnorm,
                       floor=K.subnormal_floor(cv, SCALE))
            for a in ref.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            out.append(ref)
            acc0 = acc0.copy()
        _REF[(kind, variant)] = (g, rowptr, col, out)
    return _REF[(kind, variant)]


def check(what, g, rowptr, col, ref, gval, gres, rtol=K.RTOL_JAC, floor32=0.0, slots=None):
    """the measure of the module docstring; prints the worst connection, diagonal row and residual row before it asserts"""
    F = K.fixture()
    slots = list(range(9)) if slots is None else slots
    tiny = (g.trans > 0) & (g.trans < 2.3e-308)        # subnormal T: the only connections where the oracle may hold a 0 the device rounds otherwise
    floor = ref["floor"] + floor32
    dev = K.connection_blocks(rowptr, col, g.conn_cells, gval)
    err, norm = K.connection_error(dev[:, :, slots], ref["blocks"][:, :, slots])
    assert np.all(err[(norm == 0) & ~tiny[:, None]] == 0.0), what                # identically zero in the oracle: exactly zero here
    rel = K.relative(np.maximum(err - floor[:, None], 0.0), norm)
    f, s = np.unravel_index(np.argmax(rel), rel.shape)
    print("%s: worst connection %d (%s, cells %s) slot %s: error %.2e of %.2e = %.2e relative" %
          (what, f, F.case[f], g.conn_cells[f].tolist(), K.SLOTS[slots[s]], err[f, s], norm[f, s], rel[f, s]))
    bad = np.argwhere(rel > rtol)
    assert bad.size == 0, [(int(f), F.case[f], K.SLOTS[slots[s]], err[f, s], norm[f, s]) for f, s in bad[:8]]
    # diagonal blocks: per row and slot, relative to the largest magnitude of the slot among the row's blocks
    rows = np.arange(g.nc)
    d = K.block_index(rowptr, col, rows, rows)
    dfloor, rfloor = np.zeros(g.nc), np.zeros(g.nc)          # of a row: the sums over its connections
    for k in (0, 1):
        np.add.at(dfloor, g.conn_cells[:, k], floor)
        np.add.at(rfloor, g.conn_cells[:, k], ref["floor"])
    derr = np.abs(np.asarray(gval)[d] - ref["val"][d])[:, slots]
    drel = K.relative(np.maximum(derr - dfloor[:, None], 0.0), K.row_norms(rowptr, col, ref["val"])[:, slots])
    c, s = np.unravel_index(np.argmax(drel), drel.shape)
    print("%s: worst diagonal block: cell %d slot %s, %.2e relative" % (what, c, K.SLOTS[slots[s]], drel[c, s]))
    assert drel.max() <= rtol, (what, c, K.SLOTS[slots[s]], drel[c, s])
    # residual (always double): per row and equation, relative to the largest of its contributions
    eqs = sorted({s // 3 for s in slots})
    rerr = np.abs(np.asarray(gres).reshape(3, -1).T - ref["r"])[:, eqs]
    rrel = K.relative(np.maximum(rerr - rfloor[:, None], 0.0), ref["rnorm"][:, eqs])
    c, a = np.unravel_index(np.argmax(rrel), rrel.shape)
    print("%s: worst residual: cell %d equation %s, %.2e relative" % (what, c, "wog"[eqs[a]], rrel[c, a]))
    assert rrel.max() <= K.RTOL_JAC, (what, c, "wog"[eqs[a]], rrel[c, a], rerr[c, a], ref["rnorm"][c, eqs[a]])
    return dev


def assemble_both(m, refs):
    """first assembly with state 1, then state 2 against the accumulation of state 1: [(rowptr, col, val, residual)]"""
    out = []
    for k, ref in enumerate(refs):
        if k == 0:
            m.prepareStep(DT, ref["st"])
        else:
            m.setState(ref["st"])
        m.assemble(k == 0)
        out.append(m.jacobian() + (m.residual(),))
    return out


@pytest.mark.parametrize("ordering", list(ORDERINGS))
@pytest.mark.parametrize("variant", K.VARIANTS)
def test_every_connection_against_the_oracle(gpu_lib, oracle, variant, ordering):
    """assemble(True) and a second state with assemble(False) in both orderings: the pattern, every connection, every row's diagonal
    block and residual; the diagonal of the named cells sits first, last and in the middle of its row (from the model's own ordering)"""
    F = K.fixture()
    g, rowptr, col, refs = reference(oracle, "wog", variant)
    m = GpuBlackoilModel(g, K.tables(), capi.default_params(ilu_ordering=ORDERINGS[ordering]))
    got = assemble_both(m, refs)
    pos = m.ordering()[0]
    m.close()
    assert np.array_equal(pos, K.plan_position(rowptr, col, ORDERINGS[ordering]))       # the numbering the census of the CPU test used
    named = np.unique(np.concatenate([F.conn[K.cases(n)].ravel() for n in K.PAIR_CASES] + [np.array(F.leaves + [F.hub])]))
    kinds = K.diagonal_kind(F.conn, pos)
    assert {"first", "middle", "last"} <= set(kinds[named]) and set(kinds[np.array(F.isolated)]) == {"only"}
    for k, (ref, (gr, gc, gv, res)) in enumerate(zip(refs, got)):
        assert np.array_equal(gr, rowptr) and np.array_equal(gc, col)
        dev = check("%s %s assemble(%s)" % (variant, ordering, k == 0), g, rowptr, col, ref, gv, res)
        # exact statements beside the oracle: a closed connection and one with T == 0 leave exact zeros in all nine slots of both blocks
        closed = ~ref["cv"]["open"].any(1) | (g.trans == 0.0)
        if variant != "nothp":
            assert closed[K.cases("one float below")].all() and closed[K.cases("closed")].all()
        assert closed[K.cases("T == 0")].all() and np.all(dev[closed] == 0.0)
        assert np.all(np.abs(dev[K.cases("one float above")]).max((1, 2)) > 0) and np.all(np.abs(dev[K.cases("dh == +thp")]).max((1, 2)) > 0)
        if k == 0:      # a three-phase tie carries no flux: the cells that have nothing else keep an exactly zero residual
            alone = [c for c in F.alone if F.role[c][0] == "three-phase tie"]
            assert len(alone) == 4 and np.all(np.asarray(res).reshape(3, -1)[:, alone] == 0.0)


def test_water_tie_takes_the_first_cell(gpu_lib, oracle):
    """at a water tie by region |J[water][p]| of both off-diagonal blocks is matbalscale[0] * T * U_w(c1), with U_w = (1 / B_w) kr_w / mu_w
    of the device's own output record; U_w(c2) is at least a factor of 2 away"""
    g, rowptr, col, refs = reference(oracle, "wog", "base")
    m = GpuBlackoilModel(g, K.tables())
    f = K.cases("water tie by region")
    c1, c2 = g.conn_cells[f, 0], g.conn_cells[f, 1]
    for k, ref in enumerate(refs):
        m.prepareStep(DT, ref["st"])
        m.assemble(True)
        d = m.simulatorData()
        U = d["1OVERBW"] * d["WATKR"] / d["WAT_VISC"]
        rp, cc, val = m.jacobian()
        J = np.abs(K.connection_blocks(rp, cc, g.conn_cells, val)[f][:, :, 0])              # [instance][block (c1, c2) | (c2, c1)]
        want = SCALE[0] * g.trans[f] * U[c1]
        other = SCALE[0] * g.trans[f] * U[c2]
        print("water ties, state %d: |J_wp| / (s T U_w(c1)) - 1 = %s; U_w(c2) / U_w(c1) = %s" % (k + 1, (J / want[:, None] - 1).ravel(), U[c2] / U[c1]))
        assert np.all(np.abs(J - want[:, None]) <= K.RTOL_JAC * want[:, None])
        assert np.all(np.maximum(other / want, want / other) >= 2.0)
    m.close()


def _table_bytes(tab, f64_only):
    return sum(a.nbytes for a in vars(tab).values() if isinstance(a, np.ndarray) and (a.dtype == np.float64 or not f64_only))


@pytest.mark.parametrize("shape", ["blob", "float", "mixed", "blob-float"])
def test_the_shapes_connection_by_connection(gpu_lib, oracle, shape):
    """the same fixture through the other shapes of the kernel (tests/test_gpu_assembly_shapes.py): tables read from the blob (the four
    regions repeated past 24 KiB, the cells' region numbers drawn from all copies), a float Jacobian (setSolvePrecision(True)), the
    float copy written next to the double one (preconditioner_single).  Float: RTOL_JAC_F32 per connection, zero blocks stay exact
    zeros; mixed: the double Jacobian equals the plain double one bit for bit."""
    g0, rowptr, col, refs = reference(oracle, "wog", "base")
    blob = shape.startswith("blob")
    tab = K.tables(COPIES if blob else 1)
    g = K.grid("base", COPIES) if blob else g0
    assert _table_bytes(tab, True) > LDS_BYTES if blob else 2 * _table_bytes(tab, False) < LDS_BYTES
    if blob:
        assert len(set(g.satnum // 2)) == COPIES and len(set(g.pvtnum // 2)) == COPIES and np.array_equal(g.satnum % 2, g0.satnum) and np.array_equal(g.pvtnum % 2, g0.pvtnum)
    single = shape.endswith("float")
    m = GpuBlackoilModel(g, tab, capi.default_params(preconditioner_single=int(shape == "mixed")))
    m.setSolvePrecision(single)
    got = assemble_both(m, refs)
    m.close()
    plain = None
    if shape == "mixed":
        m = GpuBlackoilModel(g, tab)
        plain = assemble_both(m, refs)
        m.close()
    for k, (ref, (gr, gc, gv, res)) in enumerate(zip(refs, got)):
        assert np.array_equal(gr, rowptr) and np.array_equal(gc, col)
        if single:
            assert np.array_equal(gv, gv.astype(np.float32).astype(np.float64))       # it IS a float Jacobian
        dev = check("%s assemble(%s)" % (shape, k == 0), g0, rowptr, col, ref, gv, res, rtol=K.RTOL_JAC_F32 if single else K.RTOL_JAC,
                    floor32=F32_FLOOR if single else 0.0)
        closed = ~ref["cv"]["open"].any(1) | (g0.trans == 0.0)
        assert np.all(dev[closed] == 0.0)
        if plain is not None:
            assert np.array_equal(gv, plain[k][2]) and np.array_equal(res, plain[k][3])


@pytest.mark.parametrize("ordering", list(ORDERINGS))
def test_oil_water_connections(gpu_lib, oracle, ordering):
    """KM_OW has its own branch in the loop: the fixture on the oil-water deck (ties, |dh| == thp, one float below, T == 0, both listing
    orders) against the oracle on the three-phase twin, in the water and oil rows and the p and Sw columns; the third column and the gas
    row of every off-diagonal block are exact zeros, the gas diagonal is exactly 1"""
    g, rowptr, col, refs = reference(oracle, "wo", "base")
    m = GpuBlackoilModel(g, K.tables_wo(), capi.default_params(ilu_ordering=ORDERINGS[ordering]))
    got = assemble_both(m, refs)
    m.close()
    rows = np.arange(g.nc)
    d = K.block_index(rowptr, col, rows, rows)
    for k, (ref, (gr, gc, gv, res)) in enumerate(zip(refs, got)):
        assert np.array_equal(gr, rowptr) and np.array_equal(gc, col)
        dev = check("oil-water %s assemble(%s)" % (ordering, k == 0), g, rowptr, col, ref, gv, res, slots=WO_SLOTS)
        assert np.all(dev[:, :, [2, 5, 6, 7, 8]] == 0.0)
        assert np.all(gv[d][:, [2, 5, 6, 7]] == 0.0) and np.all(gv[d][:, 8] == 1.0) and np.all(np.asarray(res).reshape(3, -1)[2] == 0.0)
        closed = ~ref["cv"]["open"][:, :2].any(1) | (g.trans == 0.0)
        assert closed[K.cases("one float below")].all() and closed[K.cases("T == 0")].all() and np.all(dev[closed] == 0.0)
        assert np.all(np.abs(dev[K.cases("oil tie")]).max((1, 2)) > 0)


@pytest.mark.parametrize("single", [False, True], ids=["double", "float"])
def test_cpr_weights_of_the_fixture(gpu_lib, oracle, single):
    """use_cpr: the weights the kernel forms from its sums of |dR_j / dp_i| (sod[]) against formEllipticSystem's rule on the assembled
    matrix, the comparison of test_cpr_pressure_equation_weights.  Rows whose only connections are closed (and the isolated cells) have
    an off-diagonal sum of 0: x / 0 is strong for x > 0, and 0 / 0 compares false."""
    F = K.fixture()
    g, rowptr, col, refs = reference(oracle, "wog", "base")
    m = GpuBlackoilModel(g, K.tables(), capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, linear_solver_maxiter=20))
    m.prepareStep(DT, refs[0]["st"])
    m.setSolvePrecision(single)
    m.assemble(True)
    rp, cc, val = m.jacobian()
    try:
        m.getConvergence()
        m.solveJacobianSystem(single_precision=single)
    except (NumericalIssue, LinearSolverProblem, ISTLError):
        pass                                             # twenty iterations on random states: the solve is not the point here
    w = np.zeros(3 * g.nc)
    m._chk(m.lib.opmgpu_get_cpr_weights(m.ctx, capi.dptr(w)))
    m.close()
    nb = g.nc
    rows = np.repeat(np.arange(nb), np.diff(rp))
    v3 = val.reshape(-1, 3, 3)
    expect, margin = np.zeros((3, nb)), np.zeros((3, nb))
    for eq in range(3):
        dj = np.abs(v3[rows == cc, eq, 0])
        off = np.zeros(nb)
        np.add.at(off, cc[rows != cc], np.abs(v3[rows != cc, eq, 0]))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):          # (off may be a subnormal sum: T == 5e-324)
            expect[eq] = dj / off > 0.01
            margin[eq] = np.abs(dj / off / 0.01 - 1.0)
    none = expect.sum(0) == 0
    expect[1, none] = 1.0
    dead = np.array(F.isolated + [c for c in F.alone if F.role[c][0] == "T == 0"])
    off_p = np.zeros(nb)
    np.add.at(off_p, cc[rows != cc], np.abs(v3[rows != cc, :, 0]).sum(1))
    assert np.all(off_p[dead] == 0.0)
    decided = np.nan_to_num(margin, nan=1.0).min(0) > 1e-6                   # (a ratio within 1e-6 of the threshold is rounding's to decide)
    print("CPR weights: %d rows, %d with nothing strong, %d with an off-diagonal sum of 0, %d within 1e-6 of the threshold" %
          (nb, none.sum(), (off_p == 0).sum(), (~decided).sum()))
    assert decided.sum() >= nb - 2 and (off_p == 0).sum() >= dead.size
    bad = np.flatnonzero((w.reshape(3, nb) != expect).any(0) & decided)
    assert bad.size == 0, (bad[:10], w.reshape(3, nb)[:, bad[:4]], expect[:, bad[:4]])


def test_a_pair_joined_twice_is_refused(gpu_lib):
    """what makes 'one connection per pair of off-diagonal blocks' true: the same pair listed again, either way round, is OPMGPU_EINVAL"""
    g = K.grid()
    for extra in (g.conn_cells[5], g.conn_cells[5, ::-1]):
        conn = np.concatenate([g.conn_cells, extra[None, :]])
        g2 = decks.GridData(g.nc, conn, np.append(g.trans, 1e-13), g.pv, g.z, thpres=np.append(g.thpres, 0.0), pvtnum=g.pvtnum, satnum=g.satnum)
        ctx = C.c_void_p()
        st = gpu_lib.opmgpu_create(C.byref(ctx), 0, C.byref(g2.struct()), C.byref(K.tables().struct()), None)
        assert st == capi.EINVAL and not ctx and b"duplicate cell pair" in gpu_lib.opmgpu_last_error(None)
