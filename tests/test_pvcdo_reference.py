"""CPU: the numpy restatement of the PVCDO rule (tests/pvcdo_reference.py) against closed forms, and the derived error bounds of the
dense-PVDO twin (tests/pvcdo_cases.py) against the twin itself, evaluated by the unchanged oracle."""
import numpy as np
import pytest

import pvcdo_cases as cases
import pvcdo_reference as ref

P = np.linspace(cases.P_LO, cases.P_HI, 1101) * ref.BAR


@pytest.mark.parametrize("row", cases.rows_si().tolist())
def test_at_the_reference_pressure(row):
    b, _ = ref.inv_b(row, row[0])
    mu, _ = ref.viscosity(row, row[0])
    bm, _ = ref.inv_bmu(row, row[0])
    assert b == 1.0 / row[1] and mu == pytest.approx(row[3], rel=1e-15) and bm == 1.0 / (row[1] * row[3])


@pytest.mark.parametrize("row", cases.rows_si().tolist())
def test_constant_viscosity_and_constant_product(row):
    """The two closed forms of the viscosibility.  C_v = 0 (Y = X): 1 / (B_o mu_o) = (1 / B_o) / mu_ref, the viscosity is mu_ref at every
    pressure.  C_v = C_o (Y = 0): the product B_o mu_o is B_ref mu_ref at every pressure.  (The product is NOT constant with C_v = 0: it
    follows B_o.)"""
    r = list(row); r[4] = 0.0
    b, _ = ref.inv_b(r, P)
    mu, dmu = ref.viscosity(r, P)
    bm, _ = ref.inv_bmu(r, P)
    assert np.allclose(mu, r[3], rtol=1e-15, atol=0.0) and np.allclose(bm * r[3], b, rtol=1e-15, atol=0.0)
    assert np.abs(dmu).max() <= 1e-15 * r[3] * r[2]
    r[4] = r[2]
    b, db = ref.inv_b(r, P)
    mu, dmu = ref.viscosity(r, P)
    bm, dbm = ref.inv_bmu(r, P)
    assert np.all(bm == 1.0 / (r[1] * r[3])) and np.all(dbm == 0.0)
    assert np.allclose(mu / b, r[1] * r[3], rtol=1e-15, atol=0.0) and np.allclose(dmu, db * (r[1] * r[3]), rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("row", cases.rows_si().tolist())
def test_derivatives_against_complex_steps(row):
    h = 1e-30
    for f in (ref.inv_b, ref.inv_bmu, ref.viscosity):
        v, dv = f(row, P)
        cs = np.imag(f(row, P + 1j * h)[0]) / h
        assert np.allclose(dv, cs, rtol=1e-12, atol=0.0), f.__name__
        assert np.allclose(v, np.real(f(row, P + 1j * h)[0]), rtol=1e-15, atol=0.0)
    assert np.all(ref.inv_b(row, P)[1] > 0.0)                                   # the oil is compressible: 1 / B_o grows with p


def test_the_cases_stay_inside_what_the_issue_allows():
    for r in cases.ROWS:
        assert 0.0 < r[2] <= 1.5e-4 and 0.0 < r[4] <= 6.0e-4
    assert cases.H == 0.25 and cases.c_max() == pytest.approx(4.5e-4)
    assert cases.value_bound() == pytest.approx((0.25 * 4.5e-4) ** 2 / 8) and cases.tol_value() == 10 * cases.value_bound()
    assert cases.slope_bound() == pytest.approx(0.25 * 4.5e-4 / 2 / (1 - 4.5e-4 * 370.0)) and cases.tol_slope() == 2 * cases.slope_bound()


@pytest.mark.parametrize("form", ["default", "ow"])
def test_the_twin_is_within_its_bounds(oracle, form):
    """the oracle on the dense-PVDO twin against the rule: 1 / B_o and 1 / (B_o mu_o) within the value bound, their slopes within the slope bound"""
    g = cases.grid()
    _, twin = cases.tables(form)
    st = cases.state(g, form)
    props = oracle.cell_props(g, twin, st)
    nm = oracle.PROP_NAMES
    rows = ref.rows_of(cases.rows_si(), g.pvtnum)
    b, db = ref.inv_b(rows, st.p)
    bm, dbm = ref.inv_bmu(rows, st.p)
    ob, omu = props[:, nm.index("b_o")], props[:, nm.index("mu_o")]
    obm = ob[:, 0] / omu[:, 0]
    dobm = (ob[:, 1] - obm * omu[:, 1]) / omu[:, 0]                              # d (b / mu) / d p
    round_off = 1e-14
    ev, es = np.abs(ob[:, 0] / b - 1).max(), np.abs(ob[:, 1] / db - 1).max()
    evm, esm = np.abs(obm / bm - 1).max(), np.abs(dobm / dbm - 1).max()
    print("1/B: value %.2e slope %.2e; 1/(B mu): value %.2e slope %.2e; bounds %.2e / %.2e" % (ev, es, evm, esm, cases.value_bound(), cases.slope_bound()))
    # (H c)^2 / 8 bounds the error of the interpolated polynomial; relative to 1 / B and 1 / (B mu) it is divided by the polynomial's
    # value, at least 1 - c max |p - p_ref| (cases.value_bound_relative); ten times the plain figure, the GPU tests' tolerance, covers it
    assert ev <= cases.value_bound_relative() + round_off and evm <= cases.value_bound_relative() + round_off
    assert cases.value_bound_relative() < 1.25 * cases.value_bound() < cases.tol_value()
    assert es <= cases.slope_bound() and esm <= cases.slope_bound()
    assert ev > 0.0 and es > 1e-7                                               # and the twin IS another function than the rule
