"""SWATINIT in the EQUIL initialisation (opmgpu/equil.py) against the known answers of the reference's DeckWithSwatinit
(tests/test_equil_legacy.cpp:916-1060, transcribed to tests/golden/swatinit_known_answers.json).

The reference's deck capillarySwatinit.DATA is not in its tree.  It is the DeckWithCapillary input (rebuilt in tests/test_equil.py from
the vectors of the reference's CapillaryInversion case) run with g = 9.81 and SWATINIT = 0.1 in cells 0-4, 0.5 in cells 5-14 and 1.0 in
cells 15-19: that input reproduces all 60 unscaled saturations and, with the rule of include/opmgpu.h (opmgpu_set_swatinit_scaling), the
60 saturations with SWATINIT and the 12 scaled capillary pressures.  The rule itself is ours (EclMaterialLawManager::applySwatinit is
outside the reference tree); these numbers are what pins it.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opm-simulators-legacy_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from opmgpu import equil as E  # noqa: E402
from opmgpu.decks import BAR, FluidTables, GridData  # noqa: E402

import swatinit_reference as ref  # noqa: E402

KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "swatinit_known_answers.json")))
CAP_SWOF = ((0.2, 0, 1, 0.4), (1, 1, 0, 0.1))
CAP_SGOF = ((0, 0, 1, 0.2), (0.8, 1, 0, 0.5))
SWATINIT = np.r_[np.full(5, 0.1), np.full(10, 0.5), np.full(5, 1.0)]
GRAV = 9.81


def column_case(zgoc=20.0):
    """the 1 x 1 x 20 column of 5 m cells of DeckWithCapillary: dead oil, dry gas, SWOF / SGOF with capillary pressure"""
    pvdo, pvdg = ((100, 1.0, 1.0), (200, 0.9, 1.0)), ((100, 0.010, 0.1), (200, 0.005, 0.2))
    t = FluidTables(density_wog=[[1000.0, 700.0, 1.0]], pvtw=[[1.0, 1.0, 4.0e-5, 0.96, 0.0]], pvto=[[(0.0, [r]) for r in pvdo]],
                    pvtg=[[(r[0], [(0.0, r[1], r[2])]) for r in pvdg]], swof=[list(CAP_SWOF)], sgof=[list(CAP_SGOF)], rock=(1.0, 0.0),
                    disgas=False, vapoil=False)
    z = (np.arange(20) + 0.5) * 5.0
    g = GridData(20, np.zeros((0, 2), np.int32), np.zeros(0), np.ones(20), z, dims=(1, 1, 20))
    rec = E.EquilRecord(50, 150 * BAR, 50, 0.25 * BAR, zgoc, 0.35 * BAR)
    return g, t, rec


def equilibrated(swatinit=None):
    g, t, rec = column_case()
    return E.equilibrate(g, t, [rec], ztop=g.z - 2.5, zbot=g.z + 2.5, grav=GRAV, swatinit=swatinit)


@pytest.fixture(scope="module")
def runs():
    return equilibrated(), equilibrated(SWATINIT)


def check(value, expected, reltol=1e-3):
    """the reference test's CHECK(value, expected, 1e-3) as this repository reads it: 1e-3 relative, |value| < 1e-6 for an expected zero
    (the equilibrated saturations are in fact within 5e-14 of the vectors)"""
    if expected == 0:
        assert abs(value) < 1e-6, (value, expected)
    else:
        assert abs(value - expected) <= reltol * min(abs(value), abs(expected)), (value, expected)


def test_saturations_without_swatinit(runs):
    plain, _ = runs
    for ph in range(3):
        for i in range(20):
            check(plain.sat[i, ph], KNOWN["s"][ph][i])


def test_saturations_with_swatinit(runs):
    _, scaled = runs
    for ph in range(3):
        for i in range(20):
            check(scaled.sat[i, ph], KNOWN["swatinit"][ph][i])


def test_scaled_capillary_pressures(runs):
    """the host curve after scaling at the equilibrated saturations: the 12 truth values at 1e-4 relative (they carry 5-7 digits; the
    inputs reproduce them to 9e-6).  Cells 0-4: 150031.3 ... 97245.4, not the table's 40000: a saturation clamped to Swl is still scaled."""
    _, scaled = runs
    g, t, rec = column_case()
    truth = np.array(KNOWN["pc_scaled_truth"])
    err = np.abs(scaled.pcow[:12] / truth - 1.0)
    print("largest relative difference to pc_scaled_truth: %.2e" % err.max())
    assert err.max() <= 1e-4
    # the same numbers through a curve object of its own with the PCW the state reports, and through the restatement
    grid = GridData(20, np.zeros((0, 2), np.int32), np.zeros(0), np.ones(20), g.z, dims=(1, 1, 20), eps_v={"PCW": scaled.pcw})
    again = E.CapPress(t, grid, np.arange(20)).pcow(scaled.sat[:, 0])
    assert np.allclose(again, scaled.pcow, rtol=1e-14, atol=0)
    assert np.allclose(ref.Curves(grid, t).pcow(scaled.sat[:, 0]), scaled.pcow, rtol=1e-13, atol=0)
    assert np.all(scaled.pcw[:12] > 0.4 * BAR * 0.1) and not np.allclose(scaled.pcw[:12], 0.4 * BAR)


def test_unscaled_cells_stay(runs):
    plain, scaled = runs
    assert np.array_equal(scaled.sat[12:], plain.sat[12:])                  # po - pw < 0 there: Swu, nothing scaled
    assert np.array_equal(scaled.sat[:, 2], plain.sat[:, 2])                # the whole gas column
    assert np.array_equal(scaled.pcw[12:], np.full(8, 0.4 * BAR))           # the table maximum
    assert np.array_equal(plain.pcw, np.full(20, 0.4 * BAR))
    assert np.array_equal(scaled.phase_pressure[12:], plain.phase_pressure[12:])


def test_idempotence():
    """a second application with pcow equal to the scaled curve at the saturation the first one left changes nothing (what the call at
    FlowMain.hpp:683-690 amounts to when both property objects share one law manager); a second one with the SAME target compounds
    only where the first did not reach it (nowhere: the ratio is 1)"""
    g, t, rec = column_case()
    cp = E.CapPress(t, g, np.arange(20))
    rng = np.random.default_rng(3)
    target = rng.uniform(-0.2, 2.0, 20) * BAR
    sw_in = rng.uniform(0.0, 1.0, 20)
    sw1 = cp.apply_swatinit(None, target, sw_in)
    pcw1 = cp.pcw.copy()
    assert np.any(pcw1 != 0.4 * BAR) and np.all(pcw1[target < 0] == 0.4 * BAR) and np.all(sw1[target < 0] == 1.0)
    assert np.all(sw1[target >= 0] == np.clip(sw_in, 0.2, 1.0)[target >= 0])
    hit = target >= 0
    assert np.allclose(cp.pcow(sw1)[hit], target[hit], rtol=1e-14, atol=0)
    sw2 = cp.apply_swatinit(None, cp.pcow(sw1), sw1)
    assert np.array_equal(sw2, sw1) and np.allclose(cp.pcw, pcw1, rtol=1e-15, atol=0)
    # the restatement applies the same rule
    r = ref.Curves(g, t)
    swr, scaled = r.apply_swatinit(sw_in, target)
    assert np.array_equal(swr, sw1) and np.allclose(r.pcw, pcw1, rtol=1e-14, atol=0) and np.array_equal(scaled, hit)


def test_overlapping_transition_zones():
    """No reference vectors: structural.  With the gas-oil contact at 42 m the gas-oil and oil-water transition zones overlap in the top
    cells (sg + sw > 1): the reference re-applies SWATINIT with pcgw = pg - pw and then lets satFromSumOfPcs overwrite sw
    (initStateEquil_impl.hpp:678-688), so afterwards sw + sg = 1 and pcow(sw) + pcgo(sg) = pg - pw on the SCALED curve, to the root
    finder's tolerance: 1e-6 in saturation (EquilibrationHelpers.hpp:646-652) times the steepest slope of the sum of the two curves."""
    g, t, rec = column_case(zgoc=42.0)
    reg = E.EquilReg(rec, E.NoMixing(), E.NoMixing(), E.HostPvt(t))
    out = {}
    for key, swi in (("plain", None), ("swatinit", np.full(20, 0.6))):
        press = E.phase_pressures(g.z, (0.0, 100.0), reg, GRAV)
        cp = E.CapPress(t, g, np.arange(20))
        s = E.phase_saturations(g.z, reg, cp, press, True, swi)
        out[key] = (s, press, cp)
    (s, press, cp), (s0, _, _) = out["swatinit"], out["plain"]
    over = np.flatnonzero((s[1] == 0.0) & (s[2] > 0.0) & (s[0] > 0.2 + 1e-6) & (s[0] < 1.0 - 1e-6))
    assert over.size >= 4 and np.all(s0[1][over] == 0.0)                     # (the plain run has no oil there either)
    assert np.allclose((s[0] + s[2])[over], 1.0, rtol=0, atol=1e-15)
    assert np.all(cp.pcw[over] > 0.4 * BAR)                                  # rescaled (twice: with pcow, then with pcgw)
    slope = cp.pcw[over] / 0.8 + 0.3 * BAR / 0.8
    miss = np.abs(cp.pcow(s[0])[over] + cp.pcgo(s[2])[over] - (press[2] - press[0])[over])
    print("largest |pcow + pcgo - (pg - pw)| in the overlap cells: %.3e Pa (bound %.3e)" % (miss.max(), (1e-6 * slope).min()))
    assert np.all(miss <= 1e-6 * slope)
    assert np.all(np.abs(s[0][over] - 0.6) > 1e-3)                          # "fails to honour swat_init", as the reference notes


def test_oil_water_branch():
    """No reference vectors: structural.  A table set without a gas phase goes through the gas_active = False branch: the imposed
    saturation is honoured where Swl < sw < Swu and po - pw > 0, sg = 0, and po - pw equals the scaled curve there."""
    swof = [(0.15, 0.0, 0.9, 0.5), (0.3, 0.05, 0.55, 0.3), (0.5, 0.2, 0.25, 0.15), (0.75, 0.5, 0.0, 0.05), (1.0, 1.0, 0.0, 0.0)]
    t = FluidTables(density_wog=[[1030.0, 820.0]], pvtw=[[250.0, 1.02, 4.0e-5, 0.5, 1.0e-4]],
                    pvto=[[(0.0, [r]) for r in ((1.0, 1.062, 1.0), (200.0, 1.03, 1.17), (600.0, 0.982, 1.6))]], pvtg=None, swof=[swof],
                    sgof=None, rock=(250.0, 5.0e-5), phases="wo")
    z = 2500.0 + (np.arange(12) + 0.5) * 4.0
    g = GridData(12, np.zeros((0, 2), np.int32), np.zeros(0), np.ones(12), z, dims=(1, 1, 12))
    rec = E.EquilRecord(2500.0, 250 * BAR, 2540.0, 0.0, 2500.0, 0.0)
    swi = np.linspace(0.05, 0.95, 12)
    plain = E.equilibrate(g, t, [rec], ztop=z - 2.0, zbot=z + 2.0)
    st = E.equilibrate(g, t, [rec], ztop=z - 2.0, zbot=z + 2.0, swatinit=swi)
    pp = st.phase_pressure
    inside = (swi > 0.15) & (swi < 1.0) & ((plain.phase_pressure[:, 1] - plain.phase_pressure[:, 0]) > 0)
    assert inside.sum() >= 6 and np.array_equal(st.sat[inside, 0], swi[inside])
    assert np.all(st.sat[:, 2] == 0.0) and np.allclose(st.sat.sum(1), 1.0, rtol=0, atol=1e-15)
    assert np.allclose((pp[:, 1] - pp[:, 0])[inside], st.pcow[inside], rtol=1e-12, atol=0)
    assert np.all(st.pcw[inside] != 0.5 * BAR) and np.array_equal(plain.pcw, np.full(12, 0.5 * BAR))
    below = z > 2540.0                                                        # po - pw < 0 below the contact (pcow(woc) = 0)
    assert below.any() and np.all(st.sat[below, 0] == 1.0) and np.all(st.pcw[below] == 0.5 * BAR)
