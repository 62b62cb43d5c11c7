"""CPU: the numpy restatement of computeMaxDp / thresholdPressures / thresholdPressuresNNC (tests/thpres_reference.py) against a case
worked by hand, its strict inequalities, and the conditioning of the cases the device is compared on (tests/thpres_cases.py): a strict
test must not hinge on the last bit of a potential or of a saturation, or the comparison in tests/test_gpu_thpres.py would test rounding."""
import numpy as np
import pytest

from opmgpu import capi, decks

import thpres_cases as cases
import thpres_reference as ref


def _two_cells(sw2, p2_bar=202.0):
    """two cells, one face, two regions; tests/fluid.data's fluid: every capillary pressure 0, Bw = 1 at every pressure (rho_w = 1000),
    Bo = 1 (rho_o = 800); gravity 10, cell 1 ten metres above cell 2"""
    g = decks.GridData(2, [[0, 1]], [1e-12], [100.0, 100.0], [1000.0, 1010.0], gravity=10.0)
    t = decks.fluid_data_tables()
    z = np.zeros(2)
    st = decks.State(np.array([200.0, p2_bar]) * decks.BAR, [[1.0, 0.0, 0.0], [sw2, 0.0, 0.0]], z, z, np.full(2, capi.HC_GAS_AND_OIL, np.int8))
    return g, t, st


def test_two_cells_worked_by_hand(oracle):
    g, t, st = _two_cells(1.0)
    smin = ref.sat_range_min(g, t)
    # SWOF of fluid.data runs from Sw = 0.12 to 1, SGOF from Sg = 0 to 0.88: water 0.12, gas 0, oil max(0, 1 - 1 - 0.88) = 0
    assert np.array_equal(smin, [[0.12, 0.0, 0.0]] * 2)
    p, rho, s = ref.phase_quantities(oracle, g, t, st)
    assert np.array_equal(p, np.array([[200.0] * 3, [202.0] * 3]) * decks.BAR)           # no capillary pressure
    assert np.array_equal(rho[:, 0], [1000.0, 1000.0]) and np.array_equal(rho[:, 1], [800.0, 800.0])
    # water: p1 = 200 bar, p2 = 202 bar + 1000 * 10 * (1000 - 1010) Pa = 201 bar > p1, and Sw(2) = 1 > 0.12: counts, |p1 - p2| = 1 bar.
    # oil: p2 = 202 bar - 0.8 bar > p1, but So(2) = 0 is not above its residual 0; gas likewise: neither counts
    max_dp, dp = ref.compute_max_dp(oracle, g, t, st, [1, 2], 2, 1)
    assert dp[0] == 1.0 * decks.BAR
    assert np.array_equal(max_dp, [[-1.0, 1.0 * decks.BAR], [1.0 * decks.BAR, -1.0]])
    # one region: nothing is a barrier, no pair is present
    max_dp, dp = ref.compute_max_dp(oracle, g, t, st, [1, 1], 2, 1)
    assert dp[0] == 0.0 and np.all(max_dp == -1.0)
    # the face taken as an NNC (n_face_conn = 0) is not scanned
    max_dp, dp = ref.compute_max_dp(oracle, g, t, st, [1, 2], 2, 0)
    assert dp[0] == 0.0 and np.all(max_dp == -1.0)
    # balanced potentials (p2 = 201 bar -> 200 bar at cell 1's depth): neither p1 > p2 nor p2 > p1 for water; oil and gas still do not count
    g, t, st = _two_cells(1.0, p2_bar=201.0)
    max_dp, dp = ref.compute_max_dp(oracle, g, t, st, [1, 2], 2, 1)
    assert dp[0] == 0.0 and max_dp[0, 1] == 0.0 and max_dp[1, 0] == 0.0


def test_inequalities_are_strict(oracle):
    """a saturation exactly AT its residual value does not count; one ulp above it does.  The pair stays present, with 0.0"""
    g, t, st = _two_cells(0.12)
    max_dp, dp = ref.compute_max_dp(oracle, g, t, st, [1, 2], 2, 1)
    assert dp[0] == 0.0 and np.array_equal(max_dp, [[-1.0, 0.0], [0.0, -1.0]])
    g, t, st = _two_cells(np.nextafter(0.12, 1.0))
    max_dp, dp = ref.compute_max_dp(oracle, g, t, st, [1, 2], 2, 1)
    assert dp[0] == 1.0 * decks.BAR and max_dp[0, 1] == 1.0 * decks.BAR
    # the low-potential side's saturation is not asked: cell 1 at its residual changes nothing
    st.sat[0, 0] = 0.12
    assert ref.compute_max_dp(oracle, g, t, st, [1, 2], 2, 1)[1][0] == 1.0 * decks.BAR


def test_threshold_vector_from_barriers():
    g = decks.GridData(4, [[0, 1], [1, 2], [2, 3], [0, 3], [0, 2]], [1e-12] * 5, [1.0] * 4, [0.0] * 4)       # three faces, two NNCs
    eq = [1, 2, 2, 3]
    max_dp = np.array([[-1.0, 5.0, -1.0], [5.0, -1.0, 7.0], [-1.0, 7.0, -1.0]])
    # explicit 1-2, defaulted 2-3; no barrier 1-3: its NNC takes 0
    th = ref.threshold_pressures(g, eq, {(1, 2): 3.0, (2, 3): None}, max_dp, 3)
    assert np.array_equal(th, [3.0, 0.0, 7.0, 0.0, 3.0])
    # a defaulted barrier on an NNC whose pair no face joins: the reference's maxDp.at() throws
    with pytest.raises(KeyError):
        ref.threshold_pressures(g, eq, {(1, 3): None}, max_dp, 3)
    # the same pair on a face (all five scanned as faces) takes 0
    assert np.array_equal(ref.threshold_pressures(g, eq, {(1, 3): None}, max_dp, 5), np.zeros(5))


@pytest.mark.parametrize("case", cases.THREE_PHASE_CASES)
def test_three_phase_cases_are_well_conditioned(oracle, case):
    (g, t, eq, nreg, nface, st), max_dp, dp, det = cases.reference(oracle, "wog", case)
    assert ref.well_conditioned(det) == []
    assert g.nconn % 64 != 0 and g.nconn % 256 != 0 and nface % 64 != 0
    assert (g.nconn > nface) == (case[2] > 0)
    assert sorted(set(eq.tolist())) == [1, 2, 3, 4]
    # the pairs: 1 touches 2 only, and that pair never counts; the others count
    assert max_dp[0, 1] == 0.0 and max_dp[0, 2] == -1.0 and max_dp[0, 3] == -1.0
    assert max_dp[1, 2] > 0 and max_dp[1, 3] > 0 and max_dp[2, 3] > 0 and np.array_equal(max_dp, max_dp.T)
    if case[2] > 0:          # NNCs join regions 1 and 3 / 4, and cross other barriers: none of them is scanned
        e = eq[g.conn_cells[nface:]]
        assert ((e.min(1) == 1) & (e.max(1) >= 3)).any() and (e[:, 0] != e[:, 1]).sum() > 5 and np.all(dp[nface:] == 0.0)
    # the state: all hydrocarbon states; Rs above, at and below RsSat in each of them; residual copies
    rs_sat = oracle.pvt(t, "rsSat", st.p)[:, 0]
    for h in (capi.HC_GAS_ONLY, capi.HC_GAS_AND_OIL, capi.HC_OIL_ONLY):
        m = st.hc == h
        assert (st.rs[m] > rs_sat[m]).any() and (st.rs[m] == rs_sat[m]).any() and (st.rs[m] < rs_sat[m]).any()
    off = st.rs != rs_sat
    assert np.all(np.abs(st.rs - rs_sat)[off] > 1e-9 * rs_sat[off])                      # nowhere NEARLY at RsSat
    assert np.all(np.isin(st.p[~off], t.oil_psat[2:-1]))                                  # AT RsSat only on PVTO nodes (see thpres_cases)
    smin = det["smin"]
    assert (st.sat[:, 0] == smin[:, 0]).mean() > 0.05 and (st.sat[:, 2] == smin[:, 2]).mean() > 0.05
    # both branches of the gas PVT, and Rv nowhere nearly at RvSat
    A = oracle.cell_props(g, t, decks.State(st.p, st.sat, st.rs, st.rv, np.full(g.nc, capi.HC_GAS_AND_OIL, np.int8)))[:, :, 0]
    assert (st.rv >= A[:, ref.RV]).any() and (st.rv < A[:, ref.RV]).any() and np.all(np.abs(st.rv - A[:, ref.RV]) > 1e-12)
    # barrier faces that count and barrier faces that do not, in every pair that counts
    assert (dp[:nface][det["barrier"]] == 0.0).any() and (dp[:nface][det["barrier"]] > 0.0).any()


@pytest.mark.parametrize("case", cases.OIL_WATER_CASES)
def test_oil_water_cases_are_well_conditioned(oracle, case):
    (g, t, twin, eq, nreg, nface, st), max_dp, dp, det = cases.reference(oracle, "wo", case)
    assert ref.well_conditioned(det) == []
    assert det["nph"] == 2 and np.all(st.sat[:, 2] == 0.0)
    assert max_dp[0, 1] == 0.0 and max_dp[0, 2] == -1.0 and max_dp[1, 2] > 0 and np.array_equal(max_dp, max_dp.T)
    smin = det["smin"]
    assert (st.sat[:, 0] == smin[:, 0]).any() and (st.sat[:, 1] == smin[:, 1]).any()
    if case[1]:              # with end points SWU < 1: the two-phase oil minimum 1 - SWU is positive, and some cells lie below it
        assert np.all(smin[:, 1] > 0.0) and (st.sat[:, 1] < smin[:, 1]).any()
