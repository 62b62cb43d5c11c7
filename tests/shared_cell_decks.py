"""Decks in which several wells perforate the same cell, for tests/test_shared_cell_decks.py (no GPU) and tests/test_gpu_shared_cells.py: small
in cells, so that the oracle side stays cheap, and built so that every place of the device well path that once assumed one perforation per
row sees a shared row (csrc/wells.hip: k_well_assemble / k_well_shared_rows, wells_rebind; csrc/linsolver.hip: lowrank_add; csrc/amg.hip:
border_cell, AmgHierarchy::setup; csrc/elliptic.inl: k_ell_spmv).

  twin_deck()     6 x 6 x 4 cells.  A water and a gas injector (a WAG pair), both rate-controlled with a BHP limit, in the same four cells of
                  one column -- the column alternates between the two colours of the two-colour ordering, so both halves of k_spmv and the
                  GMRES mask see a shared row; two producers that cross in one cell; one cell with THREE wells whose indices (0, 2, 4) are
                  not adjacent in the well list; the gas injector carries the efficiency factor 0.5
  cross_deck()    3 x 3 x 260 cells.  A 260-perforation injector; a 6-perforation producer that shares the injector's perforations 257-259,
                  the second trip of every `j += 256` loop; a third well that shares nothing
  many49_deck()   well_size_decks.many_deck(49) plus one more producer in the column of well 0: 50 wells, so level 0 of the pressure stage
                  has no border and the wells reach it through the shared diagonal only
  within_deck()   one well that names a cell twice (refused)

shared_cells(wl) counts what opmgpu_well_shared_cells reports.      python tests/shared_cell_decks.py      prints the host traces."""
import os
import sys

import numpy as np

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "opm-simulators-legacy_amd"), _root, os.path.dirname(os.path.abspath(__file__))):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import well_size_decks as D  # noqa: E402
from opmgpu import decks, wells as W  # noqa: E402

WATER, OIL, GAS = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
TWIN_DIMS = (6, 6, 4)
CROSS_DIMS = (3, 3, 260)
# what the decks claim: (cells perforated by more than one well, most wells in one cell)
TWIN_SHARED, CROSS_SHARED, MANY49_SHARED = (5, 3), (3, 2), (2, 2)
TWIN_EFF_WELL, TWIN_EFF = 2, 0.5          # the gas injector


def shared_cells(wl):
    """(cells perforated by more than one well, most wells in one cell); (0, 0) without shared cells"""
    cnt = np.bincount(np.asarray(wl.cells, int))
    n = int((cnt >= 2).sum())
    return (n, int(cnt.max())) if n else (0, 0)


def shared_cell_list(wl):
    """the cells perforated by more than one well, ascending"""
    return np.flatnonzero(np.bincount(np.asarray(wl.cells, int)) >= 2)


def wells_of_cell(wl, cell):
    """the wells that perforate `cell`, in ascending perforation index"""
    pw = np.repeat(np.arange(wl.nw), np.diff(np.asarray(wl.connpos)))
    return pw[np.flatnonzero(np.asarray(wl.cells) == cell)].tolist()


def twin_deck():
    nx, ny, nz = TWIN_DIMS
    grid = decks.cartesian_grid(nx, ny, nz, dx=100.0, dy=100.0, dz=5.0, tops=2500.0, poro=0.25, permx_md=150.0, lognormal_sigma=0.5, seed=3)
    tab = decks.satfunc_standard_tables()
    st = decks.initial_state(grid, tab, p_ref=250 * decks.BAR, z_ref=2500.0, gas_cap_fraction=0.0, gas_only_fraction=0.0, perturb=0.002, seed=3)
    col = lambda i, j, ks: [i + nx * (j + ny * k) for k in ks]          # noqa: E731
    day = decks.DAY
    WI = 20.0 * 150.0 * decks.MD * 5.0
    bhp_max = [(W.BHP, 400 * decks.BAR)]
    wl = W.Wells()
    # well 0 / well 2: the WAG pair in the same four cells of column (0, 0)
    wl.add_well("INJW", W.INJECTOR, grid.z[col(0, 0, [0])[0]], col(0, 0, range(4)), WI, WATER, (W.SURFACE_RATE, 80.0 / day, WATER), limits=bhp_max)
    # well 1 / well 4: two producers of column (5, 5) that cross in its layer 2; well 4 goes on into the bottom cell of the pair's column,
    # which then holds the wells 0, 2 and 4
    wl.add_well("P1", W.PRODUCER, grid.z[col(5, 5, [0])[0]], col(5, 5, range(0, 3)), WI, OIL, (W.BHP, 235 * decks.BAR),
                limits=[(W.SURFACE_RATE, -10.0 / day, (1.0, 1.0, 0.0))])          # broken in the first pre-solve iteration: a switch, a second iteration
    wl.add_well("INJG", W.INJECTOR, grid.z[col(0, 0, [0])[0]], col(0, 0, range(4)), WI, GAS, (W.SURFACE_RATE, 5000.0 / day, GAS), limits=bhp_max,
                efficiency=TWIN_EFF)
    # well 3 shares nothing
    wl.add_well("P3", W.PRODUCER, grid.z[col(2, 3, [0])[0]], col(2, 3, range(0, 2)), WI, OIL, (W.BHP, 240 * decks.BAR))
    wl.add_well("P2", W.PRODUCER, grid.z[col(5, 5, [2])[0]], col(5, 5, range(2, 4)) + col(0, 0, [3]), WI, OIL, (W.SURFACE_RATE, -40.0 / day, OIL),
                limits=[(W.BHP, 150 * decks.BAR)])
    return D.Deck("twin", grid, tab, st, wl, 2.0 * day)


def cross_deck():
    nx, ny, nz = CROSS_DIMS
    grid = decks.cartesian_grid(nx, ny, nz, dx=50.0, dy=50.0, dz=0.5, tops=2500.0, poro=0.25, permx_md=150.0, lognormal_sigma=0.3, seed=7)
    tab = decks.satfunc_standard_tables()
    st = decks.initial_state(grid, tab, p_ref=250 * decks.BAR, z_ref=2500.0, gas_cap_fraction=0.0, gas_only_fraction=0.0)
    colz = lambda c, ks: [c + nx * ny * k for k in ks]          # noqa: E731
    day = decks.DAY
    WI = 20.0 * 150.0 * decks.MD * 0.5
    wl = W.Wells()
    wl.add_well("ILONG", W.INJECTOR, grid.z[colz(4, [0])[0]], colz(4, range(260)), WI, WATER, (W.SURFACE_RATE, 200.0 / day, WATER), limits=[(W.BHP, 400 * decks.BAR)])
    wl.add_well("PSHORT", W.PRODUCER, grid.z[colz(4, [257])[0]], colz(4, range(257, 260)) + colz(5, range(257, 260)), WI, OIL, (W.BHP, 240 * decks.BAR),
                limits=[(W.SURFACE_RATE, -10.0 / day, (1.0, 1.0, 0.0))])          # broken in the first pre-solve iteration: a switch, a second iteration
    wl.add_well("P0", W.PRODUCER, grid.z[colz(0, [0])[0]], colz(0, range(0, 64)), WI, OIL, (W.SURFACE_RATE, -150.0 / day, OIL), limits=[(W.BHP, 150 * decks.BAR)])
    return D.Deck("cross", grid, tab, st, wl, 1.0 * day)


def many49_deck():
    """MANY(49) and, in front of its last (special) well, one more BHP producer in the two cells of well 0's column"""
    base = D.many_deck(49)
    wl0 = base.wl
    cells0 = list(wl0.cells[wl0.connpos[0]:wl0.connpos[1]])
    WI0 = np.asarray(wl0.WI[wl0.connpos[0]:wl0.connpos[1]])
    out = W.Wells()
    for w in range(wl0.nw):
        lo, hi = wl0.connpos[w], wl0.connpos[w + 1]
        if w == wl0.nw - 1:
            out.add_well("PEXTRA", W.PRODUCER, wl0.depth_ref[0], cells0, WI0, OIL, (W.BHP, 238 * decks.BAR))
        out.add_well(wl0.name[w], wl0.type[w], wl0.depth_ref[w], wl0.cells[lo:hi], np.asarray(wl0.WI[lo:hi]), wl0.comp_frac[w], wl0.controls[w][0],
                     allow_cf=wl0.allow_cf[w], limits=list(wl0.controls[w][1:]), current=wl0.current0[w])
    return D.Deck("many49+1", base.grid, base.tab, base.st, out, base.dt)


def within_deck():
    """TWIN's grid with ONE well that names its second cell twice"""
    t = twin_deck()
    nx, ny, _ = TWIN_DIMS
    cells = [1, 1 + nx * ny, 1 + nx * ny, 1 + 2 * nx * ny]
    WI = 20.0 * 150.0 * decks.MD * 5.0
    wl = W.Wells()
    wl.add_well("P1", W.PRODUCER, t.grid.z[0], [0, nx * ny], WI, OIL, (W.BHP, 235 * decks.BAR))
    wl.add_well("TWICE", W.PRODUCER, t.grid.z[cells[0]], cells, WI, OIL, (W.BHP, 235 * decks.BAR))
    return D.Deck("within", t.grid, t.tab, t.st, wl, t.dt), 1, cells[1]


DECKS = {"twin": twin_deck, "cross": cross_deck, "many49": many49_deck}


if __name__ == "__main__":
    import time
    from oracle import oracle as orc
    orc.lib()
    np.set_printoptions(linewidth=200, precision=4)
    for name, make in DECKS.items():
        t0 = time.time()
        deck = make()
        tr = D.host_trace(orc, deck, newton=True)
        tr.pop("drawdown"); tr.pop("cdp")
        print(name, shared_cells(deck.wl), {k: v for k, v in tr.items()}, "%.1f s" % (time.time() - t0))
