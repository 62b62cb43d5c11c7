"""CPU: PVCDO with a non-zero compressibility / viscosibility from the deck to FluidTables(pvcdo=...), the host PVT of the equilibration,
and the C ABI's new entry (opmgpu_set_pvcdo), on the golden deck tests/golden/decks/PVCDO_SMALL.DATA."""
import ctypes as C
import os

import numpy as np
import pytest

from opmgpu import capi, decks, equil
from opmgpu import deck as deckmod

import pvcdo_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = os.path.join(ROOT, "tests", "golden", "decks", "PVCDO_SMALL.DATA")
FLUID = os.path.join(ROOT, "tests", "golden", "decks", "fluid.data")
# the rows of the golden deck, deck units
ROWS = [(230.0, 1.045, 1.2e-4, 1.20, 5.0e-4), (280.0, 1.090, 1.5e-4, 2.30, 3.0e-4)]


def _edited(tmp_path, name, *subs):
    text = open(DECK).read()
    for a, b in subs:
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write(text)
    return path


def test_golden_deck_ingests_to_the_analytic_oil():
    d = deckmod.read_deck(DECK)
    t = d.tables()
    assert t.phases == "wo" and t.n_pvt == 2 and t.has_disgas == 0
    want = ref.si(ROWS)
    assert t.pvcdo.shape == (2, 5) and np.allclose(t.pvcdo, want, rtol=1e-15, atol=0.0)
    assert np.all(t.pvcdo[:, 2] > 0.0) and np.all(t.pvcdo[:, 4] > 0.0) and not np.array_equal(t.pvcdo[0], t.pvcdo[1])
    # what opmgpu_create gets is a valid dead-oil stand-in: the constant two-node table at B_ref, mu_ref
    assert np.array_equal(t.oil_node_ptr, [0, 2, 4]) and np.all(t.oil_rs == 0.0)
    assert np.allclose(t.oil_psat, [230e5, 1030e5, 280e5, 1080e5])
    assert np.array_equal(t.oil_invb_sat, np.repeat(1.0 / want[:, 1], 2))
    assert np.allclose(t.oil_invbmu_sat, np.repeat(1.0 / (want[:, 1] * want[:, 3]), 2), rtol=1e-15)
    g = d.grid()
    assert g.nc == 120 and sorted(np.unique(g.pvtnum).tolist()) == [0, 1]


def test_zero_compressibility_keeps_the_tabulated_path(tmp_path):
    """Co = Cv = 0: exactly the tables of before (the reference's fluid.data), no analytic oil"""
    t = deckmod.read_deck(FLUID).tables()
    want = decks.fluid_data_tables()
    assert t.pvcdo is None and want.pvcdo is None
    for name in ("oil_node_ptr", "oil_col_ptr", "oil_rs", "oil_psat", "oil_invb_sat", "oil_invbmu_sat", "oil_col_p", "oil_col_invb", "oil_col_invbmu"):
        assert np.array_equal(getattr(t, name), getattr(want, name)), name
    # and on the golden deck with its compressibilities taken out
    path = _edited(tmp_path, "ZERO.DATA", (" 1.2E-4 ", " 0 "), (" 5.0E-4 /", " 0 /"), (" 1.5E-4 ", " 0 "), (" 3.0E-4 /", " 0 /"))
    t0 = deckmod.read_deck(path).tables()
    assert t0.pvcdo is None and np.allclose(t0.oil_psat, [230e5, 1030e5, 280e5, 1080e5]) and np.array_equal(t0.oil_invb_sat, np.repeat([1 / 1.045, 1 / 1.090], 2))


def test_refusals_name_the_keyword(tmp_path):
    few = _edited(tmp_path, "FEW.DATA", (" 280.0  1.090  1.5E-4   2.30  3.0E-4 /\n", ""))
    with pytest.raises(ValueError, match="PVCDO"):
        deckmod.read_deck(few).tables()
    # DISGAS over a dead oil (on a three-phase fragment: the oil-water deck refuses DISGAS for its missing gas phase first)
    text = ("RUNSPEC\nDIMENS\n 1 1 1 /\nOIL\nWATER\nGAS\nDISGAS\nMETRIC\nPROPS\nPVCDO\n 230 1.045 1.2E-4 1.2 5E-4 /\nPVTW\n 250 1.02 4E-5 0.5 1E-4 /\n"
            "DENSITY\n 820 1030 1 /\nPVDG\n 1 1 0.01 800 0.002 0.04 /\nSWOF\n 0.1 0 1 0 1 1 0 0 /\nSGOF\n 0 0 1 0 0.9 1 0 0 /\n")
    path = str(tmp_path / "DISGAS.DATA")
    with open(path, "w") as f:
        f.write(text)
    with pytest.raises(ValueError, match="PVCDO"):
        deckmod.read_deck(path).tables()
    ok = deckmod.read_deck(_edited_text(tmp_path, text.replace("DISGAS\n", ""))).tables()
    assert ok.pvcdo is not None and ok.has_disgas == 0
    # FluidTables itself: not with dissolved gas, not with undersaturated branches, one row per region
    kw = dict(density_wog=[[1030.0, 820.0, 1.0]], pvtw=[[250.0, 1.02, 4e-5, 0.5, 1e-4]], pvtg=[[(1.0, [(0.0, 1.0, 0.01)]), (800.0, [(0.0, 0.002, 0.04)])]],
              swof=[[(0.1, 0, 1, 0), (1, 1, 0, 0)]], sgof=[[(0, 0, 1, 0), (0.9, 1, 0, 0)]], rock=(1.0, 0.0), vapoil=False)
    with pytest.raises(ValueError, match="PVCDO"):
        decks.FluidTables(pvto=None, pvcdo=[ROWS[0]], disgas=True, **kw)
    with pytest.raises(ValueError, match="PVCDO"):
        decks.FluidTables(pvto=[[(0.0, [(1.0, 1.0, 1.0)]), (50.0, [(100.0, 1.1, 1.0), (200.0, 1.09, 1.1)])]], pvcdo=[ROWS[0]], **kw)
    with pytest.raises(ValueError, match="PVCDO"):
        decks.FluidTables(pvto=None, pvcdo=ROWS, **kw)
    assert decks.FluidTables(pvto=None, pvcdo=[ROWS[0]], **kw).has_disgas == 0


def _edited_text(tmp_path, text):
    path = str(tmp_path / "OK.DATA")
    with open(path, "w") as f:
        f.write(text)
    return path


def test_host_pvt_is_the_restatement():
    t = deckmod.read_deck(DECK).tables()
    p = np.linspace(50.0, 600.0, 23) * decks.BAR
    for reg in range(2):
        pvt = equil.HostPvt(t, reg)
        want, _ = ref.inv_b(t.pvcdo[reg], p)
        got = np.array([pvt.b_o(float(x), 0.0, True) for x in p])
        assert np.allclose(got, want, rtol=1e-15, atol=0.0)
        assert np.array_equal(got, np.array([pvt.b_o(float(x), 0.0, False) for x in p]))            # dead: no undersaturated branch
        assert got[0] < 1.0 / t.pvcdo[reg][1] < got[-1]                                              # and it is not the constant stand-in


def test_equil_integrates_the_analytic_density():
    """the oil-zone pressure gradient of the golden deck's initial state is g rho_o(p), rho_o from the restatement with the row of the
    equilibration region's first cell (setRegionPvtIdx); tests/test_equil.py's gradient check and tolerance"""
    d = deckmod.read_deck(DECK)
    t, g = d.tables(), d.grid()
    st = d.initial_state(t)
    nx, ny, nz = d.dims
    col = np.arange(nz) * nx * ny                                              # the column of cell (1, 1): layers 10 m apart
    assert np.all(np.diff(g.z[col]) == 10.0) and np.all(g.z[col[:3]] < 2528.0) and np.all(st.sat[col[:3], 1] > 0.0)      # above the contact
    row = t.pvcdo[g.pvtnum[0]]
    k = col[1]
    rho = ref.inv_b(row, st.p[k])[0] * t.surface_density[g.pvtnum[0]][1]
    grad = (st.p[col[2]] - st.p[col[0]]) / 20.0
    assert abs(grad - rho * g.gravity) < 1e-3 * rho * g.gravity
    # against the constant stand-in the integrated column differs: the feature reaches EQUIL
    rho_standin = t.surface_density[g.pvtnum[0]][1] / row[1]
    assert abs(rho - rho_standin) > 1e-4 * rho


def test_driver_refuses_a_model_that_cannot_take_the_form():
    """a model behind the driver that evaluates the tables themselves (the CPU oracle under the host well model) would compute the constant
    stand-in: refused by name; one that offers setPvcdo gets the rows"""
    from opmgpu.simulator import Simulator

    class Tabulated:
        def prepareStep(self, dt, state=None):
            pass

    class Taking(Tabulated):
        rows = None

        def setPvcdo(self, rows):
            Taking.rows = np.array(rows)

    with pytest.raises(ValueError, match="PVCDO"):
        Simulator(DECK, model_factory=lambda grid, tables, params: Tabulated())
    sim = Simulator(DECK, model_factory=lambda grid, tables, params: Taking())
    assert np.array_equal(Taking.rows, sim.tables.pvcdo)


def test_capi_exports_the_setter():
    assert capi.SIGNATURES["opmgpu_set_pvcdo"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_double)])
    lib = capi.load()
    assert lib.opmgpu_set_pvcdo.argtypes == [C.c_void_p, C.POINTER(C.c_double)] and lib.opmgpu_set_pvcdo.restype is C.c_int
    assert lib.opmgpu_set_pvcdo(None, None) == capi.EINVAL                     # no context: refused before anything is touched
    header = open(os.path.join(ROOT, "include", "opmgpu.h")).read()
    assert "int opmgpu_set_pvcdo(opmgpu_ctx* ctx, const double* pvcdo" in header
    from opmgpu.model import GpuBlackoilModel
    assert callable(GpuBlackoilModel.setPvcdo)
    assert "setPvcdo" in open(os.path.join(ROOT, "opm-simulators-legacy_amd", "host", "opmgpu.hpp")).read()
