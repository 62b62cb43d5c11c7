"""CPU: EQLOPTS / THPRES / EQLNUM of the deck reader (opmgpu/deck.py) on tests/golden/decks/THPRES_SMALL.DATA: the regions, the barriers, the
count of grid-face connections, the threshold vector from a hand-made max_dp table (thresholdPressures / thresholdPressuresNNC,
opm/simulators/thresholdPressures.hpp:320-417) and every refusal."""
import os

import numpy as np
import pytest

from opmgpu import deck as deckmod
from opmgpu.decks import BAR

import thpres_reference as ref

DECK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decks", "THPRES_SMALL.DATA")
THPRES_RECORDS = "THPRES\n 1 2 2.5 /\n 1 3 /\n 2 3 1* /\n/\n"


def variant(tmp_path, *edits, name="V.DATA"):
    """the golden deck with (old, new) text replacements, each of which must apply exactly once"""
    text = open(DECK).read()
    for old, new in edits:
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(text)
    return path


def without_thpres(tmp_path):
    return variant(tmp_path, (THPRES_RECORDS, ""), ("EQLOPTS\n 'THPRES' /\n", ""), name="NOTHPRES.DATA")


def _expected_eqlnum():
    k, j, i = np.unravel_index(np.arange(120), (4, 5, 6))
    return np.where(i < 3, 1, np.where((j < 3) & (k < 2), 2, 3))


def test_regions_barriers_and_face_count():
    d = deckmod.read_deck(DECK)
    g = d.grid()
    assert np.array_equal(d.eqlnum(), _expected_eqlnum()) and d.eqlnum().dtype == np.int32
    assert d.thpres() == {(1, 2): 2.5 * BAR, (1, 3): None, (2, 3): None}
    # 5*5*4 + 6*4*4 + 6*5*3 = 286 faces, one of them closed by MULTX = 0 (dropped with the zero-transmissibility filter), two NNCs
    assert g.nconn == 287 and g.n_face_conn == 285
    cell = lambda i, j, k: (i - 1) + 6 * ((j - 1) + 5 * (k - 1))      # noqa: E731
    assert g.conn_cells[285:].tolist() == [[cell(1, 1, 1), cell(5, 1, 1)], [cell(2, 5, 4), cell(5, 5, 3)]]
    assert [cell(3, 2, 2), cell(4, 2, 2)] not in g.conn_cells.tolist() and [cell(3, 2, 1), cell(4, 2, 1)] in g.conn_cells.tolist()
    # every pair of regions is joined by faces, and the boundaries cut all three directions
    e = d.eqlnum()[g.conn_cells[:285]]
    k, j, i = np.unravel_index(g.conn_cells[:285], (4, 5, 6))
    cut = e[:, 0] != e[:, 1]
    for axis in (i, j, k):
        assert (cut & (axis[:, 0] != axis[:, 1])).any()
    assert {tuple(sorted(p)) for p in e[cut].tolist()} == {(1, 2), (1, 3), (2, 3)}


def test_threshold_vector_from_a_max_dp_table():
    d = deckmod.read_deck(DECK)
    g, eq = d.grid(), _expected_eqlnum()
    max_dp = np.array([[-1.0, 9e5, 7e5], [9e5, -1.0, 3e5], [7e5, 3e5, -1.0]])
    th = d.threshold_pressures(g, max_dp)
    lo, hi = np.sort(eq[g.conn_cells], axis=1).T
    want = np.zeros(g.nconn)
    want[(lo == 1) & (hi == 2)] = 2.5 * BAR          # explicit: not the 9e5 of the table
    want[(lo == 1) & (hi == 3)] = 7e5
    want[(lo == 2) & (hi == 3)] = 3e5
    assert np.array_equal(th, want) and (th == 0.0).sum() > 150
    assert th[285] == 2.5 * BAR and th[286] == 7e5      # the NNCs: one across the explicit barrier, one across a defaulted one
    assert np.array_equal(th, ref.threshold_pressures(g, eq, d.thpres(), max_dp, g.n_face_conn))
    assert np.array_equal(th, d.threshold_pressures(g, {(1, 3): 7e5, (2, 3): 3e5}))        # the same table as a dict of ordered pairs
    # a defaulted pair absent from the table: its faces take 0 ...
    gone = max_dp.copy(); gone[1, 2] = gone[2, 1] = -1.0
    th0 = d.threshold_pressures(g, gone)
    assert np.all(th0[(lo == 2) & (hi == 3)] == 0.0) and np.array_equal(th0[(lo != 2) | (hi != 3)], want[(lo != 2) | (hi != 3)])
    # ... but an NNC across it is refused (the reference's maxDp.at throws)
    gone = max_dp.copy(); gone[0, 2] = gone[2, 0] = -1.0
    with pytest.raises(ValueError, match="THPRES"):
        d.threshold_pressures(g, gone)
    with pytest.raises(ValueError, match="THPRES"):      # defaulted barriers need the table
        d.threshold_pressures(g, None)


def test_later_record_wins_and_explicit_only(tmp_path):
    d = deckmod.read_deck(variant(tmp_path, (" 2 3 1* /\n/\n", " 2 3 1* /\n 3 1 4.0 /\n 3 2 0.5 /\n/\n")))
    assert d.thpres() == {(1, 2): 2.5 * BAR, (1, 3): 4.0 * BAR, (2, 3): 0.5 * BAR}
    g = d.grid()
    th = d.threshold_pressures(g)                    # nothing defaulted: no table needed
    assert sorted(set(th.tolist())) == [0.0, 0.5 * BAR, 2.5 * BAR, 4.0 * BAR]


def test_deck_without_thpres(tmp_path):
    d = deckmod.read_deck(without_thpres(tmp_path))
    g = d.grid()
    assert d.thpres() is None and d.threshold_pressures(g, None) is None
    assert np.array_equal(d.eqlnum(), _expected_eqlnum()) and g.n_face_conn == 285
    # no EQLNUM at all: one region
    src = open(DECK).read()
    a, b = src.index("EQLNUM\n 1 1 1"), src.index("SOLUTION\nEQUIL")
    d = deckmod.read_deck(variant(tmp_path, (src[a:b], ""), name="NOEQL.DATA"))
    assert np.array_equal(d.eqlnum(), np.ones(120, np.int32))
    # EQLOPTS THPRES without any THPRES record: no barrier
    d = deckmod.read_deck(variant(tmp_path, (THPRES_RECORDS, ""), name="OPTSONLY.DATA"))
    assert d.thpres() is None


@pytest.mark.parametrize("edits, word", [
    ([("EQLOPTS\n 'THPRES' /\n", "")], "EQLOPTS"),                                          # THPRES without EQLOPTS
    ([("EQLOPTS\n 'THPRES' /\n", "EQLOPTS\n 'QUIESC' /\n")], "EQLOPTS"),                    # ... or with EQLOPTS not naming it
    ([("EQLOPTS\n 'THPRES' /\n", "EQLOPTS\n 'THPRES' 'IRREVERS' /\n")], "IRREVERS"),
    ([(" 1 3 /\n", " 1 4 /\n")], "THPRES"),                                                 # above EQLDIMS item 1
    ([(" 1 3 /\n", " 0 3 /\n")], "THPRES"),                                                 # below 1
    ([("EQLDIMS\n 3 /\n", "")], "THPRES"),                                                  # EQLDIMS defaults to one region
    ([(" 1 3 /\n", " 3 3 /\n")], "THPRES"),                                                 # a region against itself
    ([(" 1 3 /\n", " 1 3 -1.0 /\n")], "THPRES"),
])
def test_refusals(tmp_path, edits, word):
    d = deckmod.read_deck(variant(tmp_path, *edits))
    with pytest.raises(ValueError, match=word):
        d.thpres()


def test_irrevers_is_refused_without_thpres_too(tmp_path):
    d = deckmod.read_deck(variant(tmp_path, (THPRES_RECORDS, ""), ("EQLOPTS\n 'THPRES' /\n", "EQLOPTS\n 'IRREVERS' /\n")))
    with pytest.raises(ValueError, match="IRREVERS"):
        d.thpres()


def test_defaulted_nnc_barrier_without_a_face(tmp_path):
    """regions 2 and 3 swapped for a deck in which an NNC is the only connection of a defaulted pair: region 3 reduced to one cell that
    touches region 1 by faces only, joined to region 2 by an NNC"""
    src = open(DECK).read()
    a, b = src.index("EQLNUM\n 1 1 1"), src.index("SOLUTION\nEQUIL")
    eq = np.where(np.arange(120) % 6 < 3, 1, 2)
    eq[0] = 3                                                                            # cell (1, 1, 1): neighbours all in region 1
    path = variant(tmp_path, (src[a:b], "EQLNUM\n " + " ".join(str(v) for v in eq) + " /\n"))
    d = deckmod.read_deck(path)
    g = d.grid()
    e = np.sort(d.eqlnum()[g.conn_cells], axis=1)
    assert e[285].tolist() == [2, 3] and not ((e[:285, 0] == 2) & (e[:285, 1] == 3)).any()
    max_dp = np.array([[-1.0, 9e5, 7e5], [9e5, -1.0, -1.0], [7e5, -1.0, -1.0]])
    with pytest.raises(ValueError, match="THPRES"):
        d.threshold_pressures(g, max_dp)
