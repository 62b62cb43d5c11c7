"""The cases tests/test_gpu_killough.py, tests/test_gpu_killough_dist.py and their worker share: the grids (hysteresis alone; hysteresis
with imbibition end points, SCALECRS and vertical scaling -- the decks of tests/test_gpu_assembly.py::test_satfunc_options_parity), the
history a state leaves, and the twin deck on which the unchanged oracle evaluates Killough's curves (tests/killough_reference.py)."""
import numpy as np

import killough_reference as kref
from opmgpu import decks
from test_satfunc_options import _hyst_tables

A = 0.1
CASES = ("hysteresis", "scaled", "all")          # "scaled": imbibition end points + SCALECRS; "all": vertical scaling on top


def tables():
    return _hyst_tables()                                  # region 0 = drainage curves, region 1 = imbibition curves


def grid_of(case, dims=(7, 6, 7)):
    """7 x 6 x 7 = 294 cells: more than one 256-thread block of the history kernel and no multiple of it"""
    base = decks.cartesian_grid(*dims, lognormal_sigma=0.5)
    nc = base.nc
    imb = np.ones(nc, np.int32)
    if case == "hysteresis":                               # hysteresis alone: no end-point scaling at all
        return decks.GridData(nc, base.conn_cells, base.trans, base.pv, base.z, dims=base.dims, satnum=np.zeros(nc, np.int32), imbnum=imb)
    rng = np.random.default_rng(5)
    eps = decks.random_endpoints(base, seed=3)
    eps["SOWCR"] = np.clip(eps["SOWCR"] + 0.08, 0.0, 0.5); eps["SOGCR"] = np.clip(eps["SOGCR"] + 0.05, 0.0, 0.5)
    ie = decks.random_endpoints(base, seed=4)
    ie["SGCR"] = np.clip(ie["SGCR"] + 0.15, 0.0, 0.6); ie["SOWCR"] = np.clip(ie["SOWCR"] + 0.2, 0.0, 0.6)
    eps_v = {"KRW": rng.uniform(0.3, 0.9, nc), "KRO": rng.uniform(0.6, 1.0, nc), "KRG": rng.uniform(0.5, 1.0, nc),
             "PCW": rng.uniform(0.5, 2.0, nc) * decks.BAR, "PCG": rng.uniform(1.0, 3.0, nc) * decks.BAR}
    if case == "scaled":
        return decks.with_endpoints(base, eps, scalecrs=True, imbnum=imb, ieps=ie)
    return decks.with_endpoints(base, eps, scalecrs=True, eps_v=eps_v, imbnum=imb, ieps=ie)


def history_state(grid, tab, seed):
    """the state that becomes history: tests/test_gpu_assembly.py's random states (its oil-only cells hold no gas and many cells hold
    little oil, so cells whose turning point lies in a drainage curve's run of zeros -- a guard -- occur by themselves)"""
    return decks.random_state(grid, tab, seed=seed)


def history_of(st, mdc_ow=None, mdc_go=None):
    """the two history planes after the state st became history (the "inconsistent" update: running minima of 1 - So and 1 - Sg)"""
    nc = st.sat.shape[0]
    mdc_ow = np.full(nc, 2.0) if mdc_ow is None else mdc_ow
    mdc_go = np.full(nc, 2.0) if mdc_go is None else mdc_go
    return np.minimum(mdc_ow, 1.0 - st.sat[:, 1]), np.minimum(mdc_go, 1.0 - np.clip(st.sat[:, 2], 0.0, 1.0))


def branch_fractions(tab, grid, mdc_ow, mdc_go, st, a=A):
    """per system the fractions of cells that the state st finds on a scanning curve, on the drainage curve and in a guard"""
    out = {}
    for name, mdc, sn in (("ow", mdc_ow, None), ("go", mdc_go, st.sat[:, 2])):
        scan = drain = guard = 0
        for c in range(grid.nc):
            s = kref.cell_systems(tab, grid, c)[name]
            if sn is None:
                swco = grid.eps[0][c] if grid.eps is not None else tab.swof_sw[0]
                snc = 1.0 - (st.sat[c, 2] + max(st.sat[c, 0], swco))
            else:
                snc = sn[c]
            if kref.in_guard(s, mdc[c]):
                guard += 1
            elif mdc[c] < 2.0 and 1.0 - snc > mdc[c]:
                scan += 1
            else:
                drain += 1
        out[name] = (scan / grid.nc, drain / grid.nc, guard / grid.nc)
    return out


def twin_deck(tab, grid, mdc_ow, mdc_go, a=A):
    """(tables, grid) of the twin of a deck WITHOUT end-point scaling at a frozen history: the deck's two regions and, as regions 2 .. nc + 1,
    one twin imbibition region per cell (kref.twin_table: abscissae (x - A0) / m, ordinates R y).  Carlson with zero shifts on it -- the
    unchanged oracle with Hysteresis.mdc_* set -- evaluates Killough's curves."""
    assert grid.eps is None and grid.ieps is None and grid.eps_v is None
    rows = lambda ptr, cols, r: list(zip(*[col[ptr[r]:ptr[r + 1]] for col in cols]))       # noqa: E731
    wcols = (tab.swof_sw, tab.swof_krw, tab.swof_krow, tab.swof_pcow / decks.BAR)
    gcols = (tab.sgof_sg, tab.sgof_krg, tab.sgof_krog, tab.sgof_pcgo / decks.BAR)
    swof = [rows(tab.swof_ptr, wcols, r) for r in (0, 1)]
    sgof = [rows(tab.sgof_ptr, gcols, r) for r in (0, 1)]
    for c in range(grid.nc):
        sy = kref.cell_systems(tab, grid, c)
        ireg = int(grid.imbnum[c])
        t, m, R = kref.scan(sy["go"], mdc_go[c], a)
        xg, yg = kref.twin_table(sy["go"].table_i.x, sy["go"].table_i.y, sy["go"].sncri - m * t, m, R)
        sgof.append([(x, y, o[2], o[3]) for x, y, o in zip(xg, yg, sgof[ireg])])
        t, m, R = kref.scan(sy["ow"], mdc_ow[c], a)
        xw, yw = kref.twin_table(sy["ow"].table_i.x, sy["ow"].table_i.y, 1.0 - sy["ow"].sncri - m * (1.0 - t), m, R)
        swof.append([(x, o[1], y, o[3]) for x, y, o in zip(xw, yw, swof[ireg])])
    twin_tab = decks.FluidTables(density_wog=[[1000.0, 700.0, 1.0]], pvtw=[[1.0, 1.0, 4.0e-5, 0.96, 0.0]],
                                 pvto=[[(0, [(1., 1.0, 1.2)]), (200, [(400., 1.12, .94), (500., 1.1189, .94)])]],
                                 pvtg=[[(100, [(0.0001, 0.010, 0.1), (0.0, 0.0104, 0.1)]), (200, [(0.0004, 0.005, 0.2), (0.0, 0.0054, 0.2)])]],
                                 swof=swof, sgof=sgof, rock=(1.0, 5.0e-5))
    twin_grid = decks.GridData(grid.nc, grid.conn_cells, grid.trans, grid.pv, grid.z, gravity=grid.gravity, dims=grid.dims,
                               satnum=grid.satnum, imbnum=2 + np.arange(grid.nc, dtype=np.int32))
    return twin_tab, twin_grid


def twin_deck_scaled(tab, grid, mdc_ow, mdc_go, a=A):
    """(tables, grid) of the twin of a deck with imbibition end points and SCALECRS (no vertical scaling) at a frozen history.  The
    imbibition curve of a cell is table(map_I(S)) with map_I piecewise linear through its fixed points (s_j <-> u_j); Killough's curve
    R table(map_I(A0 + m S)) is therefore the SAME table with ordinates R y seen through the fixed points (s_j - A0) / m: one twin
    region per cell holds the ordinates, the cell's twin imbibition end points hold the affine form.  KRG takes [SGCR, 1 - SOGCR - SWL,
    SGU], KROW (in Sw) [SWL + SGL, SWCR + SGL, 1 - SOWCR - SGL]: with SGL = 0 the six numbers fix SWL SWCR SOWCR SGCR SGU SOGCR; SWU, read
    by no curve the hysteresis uses, is put above the others.  A guard cell (R = m = 0) keeps the ordinates and gets fixed points that
    map every saturation into the table's run of zeros.  Carlson with zero shifts on it -- the unchanged oracle -- evaluates Killough's."""
    assert grid.ieps is not None and grid.scalecrs and grid.eps_v is None
    rows = lambda ptr, cols, r: list(zip(*[col[ptr[r]:ptr[r + 1]] for col in cols]))       # noqa: E731
    wcols = (tab.swof_sw, tab.swof_krw, tab.swof_krow, tab.swof_pcow / decks.BAR)
    gcols = (tab.sgof_sg, tab.sgof_krg, tab.sgof_krog, tab.sgof_pcgo / decks.BAR)
    swof = [rows(tab.swof_ptr, wcols, r) for r in (0, 1)]
    sgof = [rows(tab.sgof_ptr, gcols, r) for r in (0, 1)]
    ie = {k: np.zeros(grid.nc) for k in decks.GridData.EPS_NAMES}
    for c in range(grid.nc):
        sy = kref.cell_systems(tab, grid, c)
        ireg = int(grid.imbnum[c])
        t, m, R = kref.scan(sy["go"], mdc_go[c], a)
        if m > 0.0:
            a0 = sy["go"].sncri - m * t
            g = [(s - a0) / m for s in sy["go"].table_i.s_pts]
            sgof.append([(o[0], R * o[1], o[2], o[3]) for o in sgof[ireg]])
        else:
            g = [2.0, 3.0, 4.0]                            # every Sg <= 1 lies below the critical saturation
            sgof.append(list(sgof[ireg]))
        t, m, R = kref.scan(sy["ow"], mdc_ow[c], a)
        if m > 0.0:
            a0 = 1.0 - sy["ow"].sncri - m * (1.0 - t)
            w = [(s - a0) / m for s in sy["ow"].table_i.s_pts]
            swof.append([(o[0], o[1], R * o[2], o[3]) for o in swof[ireg]])
        else:
            w = [-3.0, -2.0, -1.0]                         # every Sw >= 0 lies above 1 - SOWCR
            swof.append(list(swof[ireg]))
        ie["SGL"][c], ie["SWL"][c], ie["SWCR"][c], ie["SOWCR"][c] = 0.0, w[0], w[1], 1.0 - w[2]
        ie["SGCR"][c], ie["SGU"][c], ie["SOGCR"][c], ie["SWU"][c] = g[0], g[2], 1.0 - g[1] - w[0], max(w[2], 1.0) + 0.1
    twin_tab = decks.FluidTables(density_wog=[[1000.0, 700.0, 1.0]], pvtw=[[1.0, 1.0, 4.0e-5, 0.96, 0.0]],
                                 pvto=[[(0, [(1., 1.0, 1.2)]), (200, [(400., 1.12, .94), (500., 1.1189, .94)])]],
                                 pvtg=[[(100, [(0.0001, 0.010, 0.1), (0.0, 0.0104, 0.1)]), (200, [(0.0004, 0.005, 0.2), (0.0, 0.0054, 0.2)])]],
                                 swof=swof, sgof=sgof, rock=(1.0, 5.0e-5))
    eps = {k: grid.eps[i] for i, k in enumerate(decks.GridData.EPS_NAMES)}
    base = decks.GridData(grid.nc, grid.conn_cells, grid.trans, grid.pv, grid.z, gravity=grid.gravity, dims=grid.dims, satnum=grid.satnum)
    twin_grid = decks.with_endpoints(base, eps, scalecrs=True, imbnum=2 + np.arange(grid.nc, dtype=np.int32), ieps=ie)
    return twin_tab, twin_grid
