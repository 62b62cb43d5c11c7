"""No GPU: the decks of tests/shared_cell_decks.py are what tests/test_gpu_shared_cells.py relies on, both CPU restatements of the well model
get through them, the library exports the new call, and a deck with a WAG pair in the same cells runs through the report-step driver.

Both restatements work per perforation and sum into a shared cell with np.add.at, i.e. in ascending perforation index: the order the device
path is specified to use (include/opmgpu.h, the device-well block)."""
import os

import numpy as np
import pytest

import shared_cell_decks as S
import well_size_decks as D
from opmgpu import capi, wells as W
from test_gpu_well_sizes import CDP_TOL, _host_first_assembly, _second_restatement_presolve

HERE = os.path.dirname(os.path.abspath(__file__))
WAG_DECK = os.path.join(HERE, "golden", "decks", "WAG_TWIN.DATA")


def _colour(dims, cell):
    nx, ny, _ = dims
    return (cell % nx + (cell // nx) % ny + cell // (nx * ny)) % 2


def test_the_decks_are_what_they_claim():
    t, c, m = S.twin_deck(), S.cross_deck(), S.many49_deck()
    assert S.shared_cells(t.wl) == S.TWIN_SHARED == (5, 3)
    assert S.shared_cells(c.wl) == S.CROSS_SHARED == (3, 2)
    assert S.shared_cells(m.wl) == S.MANY49_SHARED == (2, 2)
    assert S.shared_cells(D.long_deck().wl) == (0, 0)
    nx, ny, nz = S.TWIN_DIMS
    # TWIN: the pair's four cells, on both colours; the crossing; the cell of three wells with indices that are not adjacent
    pair = [nx * ny * k for k in range(4)]
    assert list(t.wl.cells[t.wl.connpos[0]:t.wl.connpos[1]]) == pair == list(t.wl.cells[t.wl.connpos[2]:t.wl.connpos[3]])
    assert sorted({_colour(S.TWIN_DIMS, x) for x in pair}) == [0, 1]
    assert (t.wl.type[0], t.wl.type[2]) == (W.INJECTOR, W.INJECTOR) and tuple(t.wl.comp_frac[0]) == S.WATER and tuple(t.wl.comp_frac[2]) == S.GAS
    for w in (0, 2):
        assert t.wl.controls[w][0][0] == W.SURFACE_RATE and [k[0] for k in t.wl.controls[w][1:]] == [W.BHP]
    cross = 5 + nx * (5 + ny * 2)
    assert S.shared_cell_list(t.wl).tolist() == sorted(pair + [cross])
    assert S.wells_of_cell(t.wl, cross) == [1, 4] and S.wells_of_cell(t.wl, pair[3]) == [0, 2, 4] and S.wells_of_cell(t.wl, pair[0]) == [0, 2]
    assert t.wl.efficiency_factors().tolist() == [1.0, 1.0, S.TWIN_EFF, 1.0, 1.0] and S.TWIN_EFF_WELL == 2
    # CROSS: the shared perforations are the injector's 257..259
    lo = c.wl.connpos[0]
    assert np.diff(c.wl.connpos).tolist() == [260, 6, 64]
    assert list(c.wl.cells[lo + 257:lo + 260]) == list(c.wl.cells[c.wl.connpos[1]:c.wl.connpos[1] + 3]) == S.shared_cell_list(c.wl).tolist()
    assert not set(c.wl.cells[c.wl.connpos[2]:c.wl.connpos[3]]) & set(c.wl.cells[:c.wl.connpos[2]])
    assert sorted({_colour(S.CROSS_DIMS, x) for x in S.shared_cell_list(c.wl)}) == [0, 1]
    # MANY49: 50 wells (no bordered level 0 beyond 48), the extra producer sits in the column of well 0
    assert m.wl.nw == 50 and m.wl.name[48] == "PEXTRA"
    assert list(m.wl.cells[m.wl.connpos[48]:m.wl.connpos[49]]) == list(m.wl.cells[0:2]) == S.shared_cell_list(m.wl).tolist()
    # WITHIN: one well, one cell twice
    w, well, cell = S.within_deck()
    cells = list(w.wl.cells[w.wl.connpos[well]:w.wl.connpos[well + 1]])
    assert cells.count(cell) == 2 and S.shared_cells(w.wl) == (1, 2)


@pytest.mark.parametrize("name", sorted(S.DECKS))
def test_both_restatements_get_through_the_decks(oracle, name):
    """The host well model on the oracle backend runs the pre-solve and two Newton iterations; oracle/wells.py runs the pre-solve; the two agree
    on the pre-solve's iteration count and on the connection pressures at test_gpu_well_sizes.CDP_TOL."""
    deck = S.DECKS[name]()
    tr = D.host_trace(oracle, deck, newton=True)
    assert tr["newton_ok"] and tr["presolve_iterations"] >= 2 and tr["presolve_switches"], tr["presolve_iterations"]
    cm = _second_restatement_presolve(oracle, deck)
    mo = _host_first_assembly(oracle, deck)
    assert cm.well_iterations == mo.wh.well_iterations == tr["presolve_iterations"]
    scale = np.abs(mo.wh.cdp).max()
    err = np.abs(cm.cdp - mo.wh.cdp).max()
    print("%s: %d pre-solve iterations, connection pressures differ by %.1e of max |cdp| = %.3e Pa" % (name, cm.well_iterations, err / scale, scale))
    assert err <= CDP_TOL * scale


def test_library_exports_the_shared_cell_query():
    lib = capi.load()
    assert hasattr(lib, "opmgpu_well_shared_cells") and "opmgpu_well_shared_cells" in capi.SIGNATURES
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "opmgpu.h")).read()
    assert "opmgpu_well_shared_cells" in hdr and "StandardWells_impl.hpp:396-560" in hdr and "BlackoilModelBase_impl.hpp:953-975" in hdr
    from opmgpu.model import GpuBlackoilModel
    assert hasattr(GpuBlackoilModel, "wellSharedCells") and hasattr(W.DeviceWellModel, "shared_cells")


def test_wag_twin_deck_runs_on_the_oracle_with_host_wells(oracle, tmp_path):
    """tests/golden/decks/WAG_TWIN.DATA (INJW and INJG at the same I, J and K range) through Simulator on the oracle backend with the host
    well model: three report steps, and both injectors inject in every one of them."""
    from opmgpu import eclio
    from opmgpu.simulator import Simulator
    from util import OracleBackend

    def oracle_model(grid, tables, params):
        return OracleBackend(oracle, grid, tables, params)

    def host_wells(model, wl, ws):
        if model.wells is None or list(model.wells[1]) != list(wl.arrays()[1]):
            model.wells = wl.arrays()
            model.rowptr, model.col = oracle.pattern(model.grid, *model.wells)
        return W.WellCoupledModel(model, W.StandardWellsHost(wl, model.grid.z, model.tab.surface_density[0]), ws)

    base = str(tmp_path / "WAG")
    sim = Simulator(WAG_DECK, params=capi.default_params(linear_solver_reduction=1e-8, linear_solver_maxiter=600), output_base=base,
                    model_factory=oracle_model, well_model_factory=host_wells)
    wl = sim.schedule.wells(0)
    assert list(wl.name) == ["INJW", "INJG", "PROD1"] and S.shared_cells(wl) == (3, 2) and wl.efficiency_factors().tolist() == [1.0, 0.5, 1.0]
    assert list(wl.cells[wl.connpos[0]:wl.connpos[1]]) == list(wl.cells[wl.connpos[1]:wl.connpos[2]])
    reps = sim.run()
    assert [r["days"] for r in reps] == [10.0, 20.0, 40.0] and all(r["failed"] == 0 for r in reps)
    sp = {a[0]: a[2] for a in eclio.read_arrays(base + ".SMSPEC")}
    kws, wgn = list(sp["KEYWORDS"]), list(sp["WGNAMES"])
    idx = lambda k, g: next(i for i, (a, b) in enumerate(zip(kws, wgn)) if a == k and b == g)      # noqa: E731
    rows = [a[2] for a in eclio.read_arrays(base + ".UNSMRY") if a[0] == "PARAMS"]
    assert len(rows) >= 3
    for r in rows:
        assert r[idx("WWIR", "INJW")] > 1.0 and r[idx("WGIR", "INJG")] > 100.0, (r[idx("WWIR", "INJW")], r[idx("WGIR", "INJG")])
        assert r[idx("WBHP", "INJW")] <= 320.0 * (1 + 1e-6) and r[idx("WBHP", "INJG")] <= 320.0 * (1 + 1e-6)
        assert r[idx("WOPR", "PROD1")] > 1.0
