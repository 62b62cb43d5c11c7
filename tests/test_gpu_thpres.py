"""GPU: threshold pressures installed after creation (opmgpu_set_threshold_pressures = BlackoilModelBase::setThresholdPressures) and the
defaulted THPRES values computed on the device (opmgpu_compute_max_dp = computeMaxDp, opm/simulators/thresholdPressures.hpp:46-298), against
the numpy restatement tests/thpres_reference.py on the cases of tests/thpres_cases.py, and a deck with THPRES through the report-step driver.

Tolerance of the computeMaxDp comparison, derived, not measured: rtol 1e-9 and atol 1e-9 x the largest phase pressure (about 0.04 Pa).
Pressures near 4e7 Pa round at 1e-8 Pa; a 1e-12 relative difference in b between the device evaluators and the oracle moves rho g dz
by at most 1e-6 Pa: four orders of margin.  -1 (pair absent) and 0.0 (present, nothing counts) are compared exactly.  That no strict test
of the rule sits on a rounding tie is asserted on the CPU, in tests/test_thpres_reference.py."""
import os

import numpy as np
import pytest

from opmgpu import capi, decks
from opmgpu import deck as deckmod
from opmgpu.model import GpuBlackoilModel
from opmgpu.simulator import Simulator

import thpres_cases as cases
import thpres_reference as ref
from test_thpres_deck import DECK, without_thpres

pytestmark = pytest.mark.gpu

RTOL, ATOL_REL = 1e-9, 1e-9
DT = 5 * decks.DAY


# ---------------------------------------------------------------------------------------------------------------------------------------
# the setter
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setter_case():
    g = decks.cartesian_grid(9, 8, 9, lognormal_sigma=0.5, seed=21)
    rng = np.random.Generator(np.random.PCG64(22))
    th = 0.5 * decks.BAR * rng.random(g.nconn)
    th[rng.random(g.nconn) < 0.2] = 0.0
    t = decks.satfunc_standard_tables()
    st = decks.initial_state(g, t, perturb=0.01)
    wells = (np.array([0, 3, 5], np.int32), np.array([7, 7 + 72, 7 + 144, 300, 372], np.int32))
    return g, th, t, st, wells


def _with(g, th):
    return decks.GridData(g.nc, g.conn_cells, g.trans, g.pv, g.z, gravity=g.gravity, thpres=th, dims=g.dims)


def _assembled(g, t, st, steps):
    """create on grid g, run the steps (("th", vector or None) / ("wells", wells)) in order, assemble once -> (residual, Jacobian values)"""
    m = GpuBlackoilModel(g, t, capi.default_params())
    for what, arg in steps:
        if what == "th":
            m.setThresholdPressures(arg)
        else:
            m.setWells(*arg)
    m.prepareStep(DT, st)
    m.assemble(True)
    out = m.residual(), m.jacobian()[2]
    m.close()
    return out


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_setter_is_bitwise_the_creation_path(gpu_lib, setter_case):
    g, th, t, st, wells = setter_case
    created_with, created_without = _assembled(_with(g, th), t, st, []), _assembled(g, t, st, [])
    assert not _same(created_with, created_without)                                      # the thresholds act on this state
    assert _same(_assembled(g, t, st, [("th", th)]), created_with)                       # set on a context created without
    assert _same(_assembled(_with(g, th), t, st, [("th", None)]), created_without)       # removed from a context created with
    other = np.roll(th, 7)
    assert _same(_assembled(_with(g, other), t, st, [("th", th)]), created_with)         # replaced
    assert _same(_assembled(g, t, st, [("th", other), ("th", None)]), created_without)


def test_setter_survives_a_new_well_pattern(gpu_lib, setter_case):
    """opmgpu_set_wells re-plans the matrix (rebuild_structure): the plane of thresholds is rebuilt from what the setter left"""
    g, th, t, st, wells = setter_case
    with_th, without = _assembled(_with(g, th), t, st, [("wells", wells)]), _assembled(g, t, st, [("wells", wells)])
    assert not _same(with_th, without)
    assert _same(_assembled(g, t, st, [("th", th), ("wells", wells)]), with_th)
    assert _same(_assembled(_with(g, th), t, st, [("th", None), ("wells", wells)]), without)
    assert _same(_assembled(g, t, st, [("wells", wells), ("th", th)]), with_th)          # and after the re-plan


def test_setter_refuses_bad_values(gpu_lib, setter_case):
    g, th, t, st, wells = setter_case
    m = GpuBlackoilModel(g, t, capi.default_params())
    m.setThresholdPressures(th)
    for bad in (-1.0, np.nan, np.inf):
        v = th.copy(); v[11] = bad
        with pytest.raises(ValueError, match="connection 11"):
            m.setThresholdPressures(v)
    with pytest.raises(ValueError):
        m.setThresholdPressures(th[:-1])
    m.prepareStep(DT, st)                         # a refused call changed nothing
    m.assemble(True)
    got = m.residual(), m.jacobian()[2]
    m.close()
    assert _same(got, _assembled(_with(g, th), t, st, []))


# ---------------------------------------------------------------------------------------------------------------------------------------
# computeMaxDp
# ---------------------------------------------------------------------------------------------------------------------------------------
def _compare(got_max, got_dp, want_max, want_dp, pmax):
    atol = ATOL_REL * pmax
    print("max |dp_conn - ref| = %.3e Pa (atol %.3e), max |max_dp - ref| = %.3e Pa" %
          (np.abs(got_dp - want_dp).max(), atol, np.abs(got_max - want_max).max()))
    assert np.array_equal(got_dp == 0.0, want_dp == 0.0)                                 # the same connections count
    assert np.allclose(got_dp, want_dp, rtol=RTOL, atol=atol)
    exact = want_max <= 0.0                                                              # -1: pair absent; 0.0: present, nothing counts
    assert np.array_equal(got_max[exact], want_max[exact]) and np.all(got_max[~exact] > 0.0)
    assert np.allclose(got_max, want_max, rtol=RTOL, atol=atol) and np.array_equal(got_max, got_max.T)


@pytest.mark.parametrize("case", cases.THREE_PHASE_CASES)
def test_compute_max_dp_three_phase(gpu_lib, oracle, case):
    (g, t, eq, nreg, nface, st), want_max, want_dp, det = cases.reference(oracle, "wog", case)
    m = GpuBlackoilModel(g, t, capi.default_params())
    m.setState(st)
    got_max, got_dp = m.computeMaxDp(eq, nreg, nface, conns=True)
    only_max = m.computeMaxDp(eq, nreg, nface)
    back = m.getState()
    _compare(got_max, got_dp, want_max, want_dp, max(np.abs(det["p1"]).max(), np.abs(det["p2"]).max()))
    assert np.array_equal(only_max, got_max)
    assert np.array_equal(back.p, st.p) and np.array_equal(back.sat, st.sat)             # the resident state is only read
    # the NNCs taken as faces too: more pairs are joined (what n_face_conn is for)
    if g.nconn > nface:
        all_max = m.computeMaxDp(eq, nreg, g.nconn)
        assert (all_max >= 0.0).sum() > (got_max >= 0.0).sum() and np.all(all_max >= got_max)
    # argument checks
    for bad_eq, nr, nf in ((np.where(eq == 4, 5, eq), nreg, nface), (np.where(eq == 1, 0, eq), nreg, nface), (eq, nreg, g.nconn + 1), (eq, nreg, -1), (eq, 0, nface)):
        with pytest.raises(ValueError):
            m.computeMaxDp(bad_eq, nr, nf)
    m.close()


def test_compute_max_dp_needs_a_state_and_survives_wells(gpu_lib, oracle):
    case = cases.THREE_PHASE_CASES[0]
    (g, t, eq, nreg, nface, st), want_max, want_dp, det = cases.reference(oracle, "wog", case)
    m = GpuBlackoilModel(g, t, capi.default_params())
    with pytest.raises(ValueError, match="state"):
        m.computeMaxDp(eq, nreg, nface)
    m.setState(st)
    first = m.computeMaxDp(eq, nreg, nface, conns=True)
    m.setWells(np.array([0, 2], np.int32), np.array([3, 200], np.int32))                 # a new plan: another internal numbering
    second = m.computeMaxDp(eq, nreg, nface, conns=True)
    m.close()
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


@pytest.mark.parametrize("case", cases.OIL_WATER_CASES)
def test_compute_max_dp_oil_water(gpu_lib, oracle, case):
    """a deck without a gas phase against the restatement on its three-phase twin, water and oil only"""
    (g, t, twin, eq, nreg, nface, st), want_max, want_dp, det = cases.reference(oracle, "wo", case)
    m = GpuBlackoilModel(g, t, capi.default_params())
    m.setState(st)
    got_max, got_dp = m.computeMaxDp(eq, nreg, nface, conns=True)
    m.close()
    _compare(got_max, got_dp, want_max, want_dp, max(np.abs(det["p1"]).max(), np.abs(det["p2"]).max()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# deck to run
# ---------------------------------------------------------------------------------------------------------------------------------------
class CountingModel(GpuBlackoilModel):
    calls = 0

    def setThresholdPressures(self, thpres):
        CountingModel.calls += 1
        return super().setThresholdPressures(thpres)

    def computeMaxDp(self, *a, **k):
        CountingModel.calls += 1
        return super().computeMaxDp(*a, **k)


def _states_equal(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("p", "sat", "rs", "rv", "hc"))


def test_deck_with_thpres_runs(gpu_lib, oracle, tmp_path):
    base = str(tmp_path / "TH")
    sim = Simulator(DECK, output_base=base)
    d = sim.deck
    g, eq = sim.grid, d.eqlnum()
    # the vector the driver installed = the restatement applied to the deck's initial state
    want_max, _, det = ref.compute_max_dp(oracle, g, sim.tables, sim.state0, eq, 3, g.n_face_conn, details=True)
    assert ref.well_conditioned(det) == []
    want = ref.threshold_pressures(g, eq, d.thpres(), want_max, g.n_face_conn)
    th = sim.threshold_pressures
    atol = ATOL_REL * max(np.abs(det["p1"]).max(), np.abs(det["p2"]).max())
    print("max |threshold - ref| = %.3e Pa (atol %.3e)" % (np.abs(th - want).max(), atol))
    assert th.shape == (g.nconn,) and np.array_equal(th == 0.0, want == 0.0) and np.allclose(th, want, rtol=RTOL, atol=atol)
    assert (th == 2.5 * decks.BAR).sum() == 6 and len(set(th.tolist())) == 4             # five open 1-2 faces and an NNC; 0, the explicit value, two computed ones
    assert _states_equal(sim.model.getState(), sim.state0)
    reps = sim.run()
    assert [r["days"] for r in reps] == [5.0, 15.0] and all(r["failed"] == 0 for r in reps)
    final = sim.model.getState()
    sim.close()

    # the deck without THPRES / EQLOPTS: no call to either entry point ...
    plain_deck = without_thpres(tmp_path)
    CountingModel.calls = 0
    plain = Simulator(plain_deck, model_factory=lambda grid, tables, params: CountingModel(grid, tables, params))
    assert plain.threshold_pressures is None
    plain.run()
    plain_final = plain.model.getState()
    plain.close()
    assert CountingModel.calls == 0
    assert not np.array_equal(plain_final.p, final.p)                                    # ... and the barriers matter to this run
    # ... and with the SAME vector given at creation it is the THPRES run, bit for bit

    def created_with(grid, tables, params):
        gt = decks.GridData(grid.nc, grid.conn_cells, grid.trans, grid.pv, grid.z, gravity=grid.gravity,
                            thpres=th, pvtnum=grid.pvtnum, satnum=grid.satnum, dims=grid.dims)
        return CountingModel(gt, tables, params)
    twin = Simulator(plain_deck, model_factory=created_with)
    twin.run()
    twin_final = twin.model.getState()
    twin.close()
    assert CountingModel.calls == 0
    assert _states_equal(twin_final, final)

    # a restarted run takes its thresholds from the DECK's initial state, not from the restart file's, and starts from the latter
    again = Simulator(DECK, restart=(base, 2))
    resumed = again.model.getState()
    assert np.array_equal(again.threshold_pressures, th)
    assert not np.array_equal(again.state0.p, sim.state0.p) and np.array_equal(resumed.p, again.state0.p)
    again.close()
