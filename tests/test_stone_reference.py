"""The numpy restatement of the Stone I / II rule (tests/stone_reference.py) against the properties the rule states for itself, on the
satfuncStandard tables (Swco = 0.1, krocw = krow(Swco) = krog(Sg = 0) = 1, Sowcr = Sogcr = 0.2 read off the tables)."""
import numpy as np
import pytest

import stone_reference as S
from opmgpu import decks

MODELS = [(S.STONE1, 1.0), (S.STONE1, 0.7), (S.STONE2, 1.0)]
SW = np.linspace(0.02, 0.98, 97)
SG = np.linspace(0.0, 0.9, 91)


@pytest.fixture(scope="module")
def cell():
    tab = decks.satfunc_standard_tables()
    c = S.Cell(S.Region(tab, 0))
    assert c.swco == 0.1 and c.krocw == 1.0 and c.som == pytest.approx(0.2, abs=1e-15)
    assert c.krog_of_so(1.0 - c.swco) == c.krocw            # the tables are consistent: krog(Sg = 0) = krocw
    return c


@pytest.mark.parametrize("model,eta", MODELS)
def test_no_gas_gives_krow(cell, model, eta):
    for sw in SW:
        assert S.kro(model, cell, sw, 0.0, eta) == pytest.approx(cell.krow(max(sw, cell.swco)), rel=1e-14, abs=1e-16)


@pytest.mark.parametrize("model,eta", MODELS)
def test_connate_water_gives_krog(cell, model, eta):
    """At Sw = Swco (and below it: Sw* = Swco).  Stone I is zero by its own rule for So* <= Som = 0.2, where this table's krog is still
    positive (it vanishes at So = 0.1), so its limit is checked above Som."""
    seen = 0
    for sw in (0.03, cell.swco):
        for sg in SG:
            if model == S.STONE1 and 1.0 - cell.swco - sg <= cell.som + 1e-12:
                continue
            seen += 1
            assert S.kro(model, cell, sw, sg, eta) == pytest.approx(cell.krog_of_so(1.0 - cell.swco - sg), rel=1e-13, abs=1e-16)
    assert seen > 100


def test_stone1_linear_exponent_without_gas_is_krow(cell):
    for sw in SW:
        assert S.kro(S.STONE1, cell, sw, 0.0, 1.0) == pytest.approx(cell.krow(max(sw, cell.swco)), rel=1e-14, abs=1e-16)


@pytest.mark.parametrize("eta", [1.0, 0.7, 2.5])
def test_stone1_vanishes_at_and_below_som(cell, eta):
    n = 0
    for sw in SW:
        for sg in SG:
            if 1.0 - max(sw, cell.swco) - sg <= cell.som:
                n += 1
                v, dw, dg = S.kro_and_derivatives(S.STONE1, cell, sw, sg, eta)
                assert v == 0.0 and dw == 0.0 and dg == 0.0
    assert n > 1000
    # just above Som it is positive, and finite in slope even for eta < 1 a hair above the switch
    v, dw, dg = S.kro_and_derivatives(S.STONE1, cell, 0.3, 1.0 - 0.3 - cell.som - 1e-6, eta)
    assert v > 0.0 and np.isfinite(dw) and np.isfinite(dg)


def test_stone2_clamp_engages_and_nothing_is_negative(cell):
    clamped = 0
    for sw in SW:
        for sg in SG:
            if sw + sg > 1.0:
                continue
            sws = max(sw, cell.swco)
            krw, krg, krow, krog = cell.krw(sw), cell.krg(sg), cell.krow(sws), cell.krog_of_so(1.0 - cell.swco - sg)
            raw = cell.krocw * ((krow / cell.krocw + krw) * (krog / cell.krocw + krg) - krw - krg)
            v, dw, dg = S.kro_and_derivatives(S.STONE2, cell, sw, sg)
            assert v >= 0.0
            if raw < 0.0:
                clamped += 1
                assert v == 0.0 and dw == 0.0 and dg == 0.0
            else:
                assert v == pytest.approx(raw, rel=1e-14, abs=1e-300)
    assert clamped > 0


def test_complex_step_matches_a_central_difference(cell):
    for model, eta in MODELS:
        for sw, sg in ((0.33, 0.21), (0.25, 0.05), (0.45, 0.15)):
            v, dw, dg = S.kro_and_derivatives(model, cell, sw, sg, eta)
            h = 1e-6
            fw = (S.kro(model, cell, sw + h, sg, eta) - S.kro(model, cell, sw - h, sg, eta)) / (2 * h)
            fg = (S.kro(model, cell, sw, sg + h, eta) - S.kro(model, cell, sw, sg - h, eta)) / (2 * h)
            assert v > 0 and dw == pytest.approx(fw, rel=1e-6, abs=1e-9) and dg == pytest.approx(fg, rel=1e-6, abs=1e-9)


def test_scaling_moves_the_end_points(cell):
    """Two-point scaling and the KRO maximum: krocw is the cell's KRO, Swco its SWL, Som the smaller of its SOWCR / SOGCR, and the scaled
    krow reaches zero at 1 - SOWCR - SGL."""
    eps = {"SWL": 0.12, "SWCR": 0.22, "SWU": 0.88, "SOWCR": 0.17, "SGL": 0.0, "SGCR": 0.08, "SGU": 0.85, "SOGCR": 0.23}
    c = S.Cell(cell.R, eps, kro_max=0.9)
    assert c.swco == 0.12 and c.krocw == pytest.approx(0.9, rel=1e-15) and c.som == 0.17
    assert c.krow(c.swco) == pytest.approx(0.9, rel=1e-15) and c.krog_of_so(1.0 - c.swco) == pytest.approx(0.9, rel=1e-15)
    assert c.krow(1.0 - 0.17 - 1e-9) > 0.0 and c.krow(1.0 - 0.17 + 1e-9) == 0.0
    for model, eta in MODELS:
        assert S.kro(model, c, c.swco, 0.0, eta) == pytest.approx(0.9, rel=1e-14)
