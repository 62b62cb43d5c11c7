"""SWATINIT on the host, from the deck: the keyword reader (Deck.swatinit), its refusals, and the equilibration of
tests/golden/decks/SWATINIT_SMALL.DATA (equil.from_deck) -- a hand-written deck with two saturation regions and a per-cell SWL.
No reference vectors exist for this deck: the checks are the defining properties of the rule (include/opmgpu.h)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opm-simulators-legacy_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from opmgpu import deck as deckmod, equil  # noqa: E402

import swatinit_reference as ref  # noqa: E402

DECK = os.path.join(ROOT, "tests", "golden", "decks", "SWATINIT_SMALL.DATA")
LAYERS = (0.05, 0.2, 0.25, 0.3, 0.4, 0.55, 0.8, 1.0)
SWATINIT_RECORD = "SWATINIT\n " + " ".join("36*%s" % v for v in ("0.05", "0.2", "0.25", "0.3", "0.4", "0.55", "0.8", "1.0")) + " /\n"


def deck_text():
    return open(DECK).read()


def variant(tmp_path, old, new, name="V.DATA"):
    text = deck_text()
    assert text.count(old) == 1
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write(text.replace(old, new))
    return path


def without_swatinit(tmp_path):
    return variant(tmp_path, SWATINIT_RECORD, "", "PLAIN.DATA")


@pytest.fixture(scope="module")
def ingested():
    d = deckmod.read_deck(DECK)
    t, g = d.tables(), d.grid()
    return d, t, g, d.initial_state(t)


def test_reader_returns_the_array(ingested, tmp_path):
    d, t, g, st = ingested
    sw = d.swatinit()
    assert g.nc == 288 and t.n_sat == 2 and sw.shape == (288,)
    assert np.array_equal(sw, np.repeat(LAYERS, 36))
    assert np.array_equal(np.unique(g.satnum), [0, 1]) and len(np.unique(g.eps[0])) == 2       # two regions, a per-cell SWL
    assert deckmod.read_deck(without_swatinit(tmp_path)).swatinit() is None


@pytest.mark.parametrize("old, new, what", [
    (SWATINIT_RECORD, SWATINIT_RECORD.replace("36*1.0", "35*1.0"), "holds 287 values"),             # not one value per cell
    (SWATINIT_RECORD, SWATINIT_RECORD.replace("36*1.0", "35*1.0 1*"), "every active cell"),          # an active cell left defaulted
    (SWATINIT_RECORD, SWATINIT_RECORD.replace("36*0.8", "36*1.2"), r"outside \[0, 1\]"),
    (SWATINIT_RECORD, SWATINIT_RECORD.replace("36*0.05", "35*0.05 -0.1"), r"outside \[0, 1\]"),
    ("EQUIL\n 2500 250 2530 0.0 2500 0.0 1 0 0 /\nRSVD\n 2500 100\n 2540 115 /\n",
     "PRESSURE\n 288*250 /\nSWAT\n 288*0.3 /\nSGAS\n 288*0 /\nRS\n 288*100 /\nRV\n 288*0 /\n", "needs EQUIL"),
    ("OIL\nWATER\nGAS\n", "OIL\nGAS\n", "water phase"),
])
def test_refusals_name_the_keyword(tmp_path, old, new, what):
    d = deckmod.read_deck(variant(tmp_path, old, new))
    with pytest.raises(ValueError, match="SWATINIT") as e:
        d.swatinit()
    assert __import__("re").search(what, str(e.value))


def test_from_deck_honours_the_imposed_saturation(ingested, tmp_path):
    d, t, g, st = ingested
    sw = d.swatinit()
    plain_deck = deckmod.read_deck(without_swatinit(tmp_path))
    plain_deck.grid()
    plain = plain_deck.initial_state(plain_deck.tables())
    swl, swu = g.eps[0], g.eps[2]
    pp0 = plain.phase_pressure
    pcow0 = pp0[:, 1] - pp0[:, 0]                           # po - pw of the hydrostatic columns: positive above the contact (pcow = 0 there)
    above = g.z < 2530.0
    free = above & (plain.sat[:, 0] < swu - 1e-6)           # the plain run's fix-up moved po where it found Sw at SWU (layer 5, region 1: below that table's smallest pcow)
    inside = (sw > swl) & (sw < swu) & above
    assert np.all(pcow0[above] > 0) and free.sum() == 5 * 36 + 18
    assert inside.sum() == 5 * 36                           # layers 1-5 (layer 0 is below SWL, layers 6-7 lie under the contact)
    assert np.array_equal(st.sat[inside, 0], sw[inside])
    assert np.abs(plain.sat[inside, 0] - sw[inside]).min() > 1e-3         # ... which the plain equilibration does not give
    assert np.array_equal(st.sat[:36, 0], swl[:36])         # below SWL: clamped (and still scaled)
    assert np.array_equal(st.sat[6 * 36:, 0], swu[6 * 36:]) and np.array_equal(st.sat[6 * 36:], plain.sat[6 * 36:])
    assert np.all(st.sat[:, 2] == 0.0) and np.allclose(st.sat.sum(1), 1.0, rtol=0, atol=1e-15)
    # the scaled curve carries the hydrostatic pressure difference in every scaled cell ...
    scaled = np.arange(288) < 6 * 36
    pp = st.phase_pressure
    assert np.allclose((pp[:, 1] - pp[:, 0])[scaled], st.pcow[scaled], rtol=1e-12, atol=0)
    assert np.allclose(st.pcow[free], pcow0[free], rtol=1e-12, atol=0)            # also in layer 0, clamped to SWL
    # ... PCW moved there and nowhere else, by region, and the restatement's curve with that PCW gives the same pressures
    tabmax = np.where(g.satnum == 0, 0.9e5, 0.7e5)
    assert np.all(st.pcw[scaled] != tabmax[scaled]) and np.array_equal(st.pcw[~scaled], tabmax[~scaled])
    assert np.array_equal(plain.pcw, tabmax)
    g.eps_v = {"PCW": st.pcw}
    try:
        assert np.allclose(ref.Curves(g, t).pcow(st.sat[:, 0]), st.pcow, rtol=1e-13, atol=0)
    finally:
        g.eps_v = None
