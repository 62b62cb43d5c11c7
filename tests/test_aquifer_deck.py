"""Deck ingest of the analytic aquifers (AQUDIMS, AQUFETP, AQUCT, AQUTAB, AQUANCON -> Deck.aquifers): units, the Carter-Tracy constants,
face selection, merged faces, fractions, and every refusal."""
import os

import numpy as np
import pytest

from opmgpu import capi, deck as deckmod
from opmgpu.decks import BAR, CP, DAY, MD

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decks", "AQUIFER_SMALL.DATA")

HEAD = """RUNSPEC
DIMENS
 3 3 2 /
OIL
WATER
GAS
METRIC
TABDIMS
 1 1 /
AQUDIMS
 0 0 2 10 2 30 /
GRID
%(geometry)s
PORO
 18*0.2 /
PERMX
 18*100 /
%(actnum)s
PROPS
PVDO
 1 1.05 1.0  400 1.0 1.2 /
PVDG
 1 1.0 0.01  400 0.004 0.03 /
SWOF
 0.1 0 1 0  0.9 1 0 0 /
SGOF
 0 0 1 0  0.9 1 0 0 /
PVTW
 200 1.02 4.0E-5 0.5 1.0E-4 /
DENSITY
 800 1000 1 /
AQUTAB
 0.1 0.3  1.0 0.8  10.0 1.6 /
SOLUTION
PRESSURE
 18*200 /
SWAT
 18*0.2 /
"""
BLOCK = """DXV
 10 20 30 /
DYV
 3*10 /
DZV
 2 4 /
TOPS
 9*1000 /"""
FET = "AQUFETP\n 1 1003 210 1.0E6 1.0E-4 20 1 /\n/\n"
CT = "AQUCT\n 2 1001 220 150 0.25 2.0E-4 400 12 90 1 2 /\n/\n"


def read(tmp_path, body, actnum="", geometry=BLOCK):
    path = tmp_path / "A.DATA"
    path.write_text(HEAD % dict(actnum=actnum, geometry=geometry) + body + "SCHEDULE\nTSTEP\n 1 /\nEND\n")
    d = deckmod.read_deck(str(path))
    d.grid()
    return d


def test_golden_deck_units_and_connections():
    d = deckmod.read_deck(GOLDEN)
    g, t = d.grid(), d.tables()
    f, c = d.aquifers(t)
    assert (f.id, f.kind, c.id, c.kind) == (1, capi.AQUIFER_FETKOVICH, 2, capi.AQUIFER_CARTER_TRACY)
    assert f.p_a0 == 250 * BAR and f.datum == 2415.0 and c.p_a0 == 250 * BAR and c.datum == 2409.0
    assert f.CtV0 == pytest.approx(5.0e7 * 1.0e-4 / BAR, rel=1e-15) and f.J == pytest.approx(50.0 / (DAY * BAR), rel=1e-15)
    # the Carter-Tracy constants, written out: beta = 2 pi (theta / 360) h phi C_t r_o^2, T_c = mu_w phi C_t r_o^2 / k_a
    ct, ro = 1.0e-4 / BAR, 500.0
    assert c.beta == pytest.approx(2 * np.pi * 0.5 * 18 * 0.2 * ct * ro ** 2, rel=1e-14)
    pref, bref, cw, muref, cv = 240 * BAR, 1.01, 4.2e-5 / BAR, 0.45 * CP, 0.0
    X = cw * (c.p_a0 - pref)
    Y = (cw - cv) * (c.p_a0 - pref)
    mu = muref * bref * ((1 + X * (1 + X / 2)) / bref) / (1 + Y * (1 + Y / 2))
    assert c.Tc == pytest.approx(mu * 0.2 * ct * ro ** 2 / (200 * MD), rel=1e-14)
    assert np.array_equal(c.td, [0.01, 0.05, 0.1, 0.5, 1.0, 5.0, 10.0, 50.0, 100.0, 1000.0]) and c.pd[0] == 0.112 and c.pd[-1] == 3.860
    # K+ under the whole bottom layer, I- along the whole west side; they share the five cells of the bottom west edge
    assert np.array_equal(np.sort(f.cells), np.arange(60, 90)) and np.array_equal(np.sort(c.cells), np.arange(0, 90, 6))
    assert np.intersect1d(f.cells, c.cells).size == 5
    assert np.allclose(f.alpha, 1 / 30, rtol=1e-15) and np.allclose(c.alpha, 1 / 15, rtol=1e-15)
    for a in (f, c):
        assert abs(a.alpha.sum() - 1.0) <= 1e-12
    assert g.nc == 90


def test_water_viscosity_rule_with_viscosibility():
    w = np.array([200 * BAR, 1.02, 4.0e-5 / BAR, 0.5 * CP, 1.0e-4 / BAR])
    p = 260 * BAR
    X, Y = w[2] * (p - w[0]), (w[2] - w[4]) * (p - w[0])
    assert deckmod.water_viscosity(w, p) == pytest.approx(w[3] * (1 + X * (1 + X / 2)) / (1 + Y * (1 + Y / 2)), rel=1e-15)
    assert deckmod.water_viscosity(w, w[0]) == pytest.approx(w[3], rel=1e-15)


def test_default_coefficient_is_the_face_area_and_items_9_10(tmp_path):
    d = read(tmp_path, FET + "AQUANCON\n 1 1 3 1 3 2 2 K+ /\n/\n")
    (a,) = d.aquifers()
    area = np.tile([10.0, 20.0, 30.0], 3) * 10.0                     # DX * DY of the bottom layer
    assert np.array_equal(a.cells, np.arange(9, 18)) and np.allclose(a.alpha, area / area.sum(), rtol=1e-15)
    d = read(tmp_path, FET + "AQUANCON\n 1 1 1 1 3 1 2 'I-' 1* 2.0 /\n 1 3 3 1 3 1 2 I+ 50 0.5 /\n/\n")
    (a,) = d.aquifers()
    w = {c: 2.0 * 10.0 * dz for c, dz in ((0, 2.0), (3, 2.0), (6, 2.0), (9, 4.0), (12, 4.0), (15, 4.0))}
    w.update({c: 25.0 for c in (2, 5, 8, 11, 14, 17)})
    assert sorted(a.cells) == sorted(w)
    tot = sum(w.values())
    for c, al in zip(a.cells, a.alpha):
        assert al == pytest.approx(w[int(c)] / tot, rel=1e-15)


def test_faces_towards_inactive_cells_and_item_11(tmp_path):
    """ACTNUM holes: cell (2, 2, 2) and the whole column (3, 1, *) are inactive.  K+ over the TOP layer connects only (2, 2, 1), whose lower
    neighbour is the hole; with item 11 = YES every active cell of the box.  An inactive cell is never connected, and cells are numbered
    among the ACTIVE ones."""
    act = "ACTNUM\n 1 1 0  1 1 1  1 1 1   1 1 0  1 0 1  1 1 1 /"
    d = read(tmp_path, FET + "AQUANCON\n 1 1 3 1 3 1 1 K+ /\n/\n", actnum=act)
    (a,) = d.aquifers()
    newid = d._grid.active_index
    assert np.array_equal(a.cells, [newid[4]]) and a.alpha[0] == 1.0
    d = read(tmp_path, FET + "AQUANCON\n 1 1 3 1 3 1 1 K+ 1* 1* YES /\n/\n", actnum=act)
    (a,) = d.aquifers()
    assert np.array_equal(a.cells, newid[[0, 1, 3, 4, 5, 6, 7, 8]])
    # I+ over the whole grid: the east side, and the cells west of the inactive column and of the hole
    d = read(tmp_path, FET + "AQUANCON\n 1 1 3 1 3 1 2 I+ /\n/\n", actnum=act)
    (a,) = d.aquifers()
    assert sorted(a.cells) == sorted(newid[[1, 5, 8, 10, 12, 14, 17]])
    assert abs(a.alpha.sum() - 1.0) <= 1e-12


def test_faces_of_one_cell_merge_and_aquifers_may_share_cells(tmp_path):
    d = read(tmp_path, FET + CT + "AQUANCON\n 1 1 3 1 3 2 2 K+ /\n 1 1 1 1 3 1 2 I- /\n 2 1 1 1 3 1 2 I- /\n/\n")
    f, c = d.aquifers()
    assert len(set(f.cells.tolist())) == f.cells.size == 12          # 9 bottom cells + 3 upper west cells: the 3 corner cells once
    k = {int(cell): al for cell, al in zip(f.cells, f.alpha)}
    tot = 3 * 600.0 + 3 * 20.0 + 3 * 40.0                            # K+: DX DY of nine cells; I-: DY DZ of three cells per layer
    assert k[9] == pytest.approx((100.0 + 40.0) / tot, rel=1e-15) and k[10] == pytest.approx(200.0 / tot, rel=1e-15) and k[0] == pytest.approx(20.0 / tot, rel=1e-15)
    assert abs(f.alpha.sum() - 1.0) <= 1e-12 and abs(c.alpha.sum() - 1.0) <= 1e-12
    assert np.intersect1d(f.cells, c.cells).size == 6
    assert c.kind == capi.AQUIFER_CARTER_TRACY and c.beta == pytest.approx(2 * np.pi * 0.25 * 12 * 0.25 * (2.0e-4 / BAR) * 400.0 ** 2, rel=1e-14)


def test_deck_without_aquifers(tmp_path):
    assert read(tmp_path, "").aquifers() == []


ANCON = "AQUANCON\n 1 1 3 1 3 2 2 K+ /\n/\n"
ANCON2 = "AQUANCON\n 2 1 3 1 3 2 2 K+ /\n/\n"
CORNER = ("COORD\n" + " ".join("%g %g 1000 %g %g 1006" % (x, y, x, y) for y in (0, 10, 20, 30) for x in (0, 10, 30, 60)) + " /\nZCORN\n"
          + " 36*1000 36*1002 36*1002 36*1006 /")


@pytest.mark.parametrize("body, actnum, geometry, match", [
    ("AQUFETP\n 1 1003 1* 1.0E6 1.0E-4 20 1 /\n/\n" + ANCON, "", BLOCK, "AQUFETP item 3"),
    ("AQUCT\n 2 1001 1* 150 0.25 2.0E-4 400 12 90 1 2 /\n/\n" + ANCON2, "", BLOCK, "AQUCT item 3"),
    ("AQUCT\n 2 1001 220 150 0.25 2.0E-4 400 12 90 1 1 /\n/\n" + ANCON2, "", BLOCK, "AQUCT item 11"),
    ("AQUCT\n 2 1001 220 150 0.25 2.0E-4 400 12 90 /\n/\n" + ANCON2, "", BLOCK, "AQUCT item 11"),
    ("AQUCT\n 2 1001 220 150 0.25 2.0E-4 400 12 90 1 3 /\n/\n" + ANCON2, "", BLOCK, "AQUCT item 11"),
    (FET + ANCON, "", CORNER, "AQUANCON item 9"),
    (FET + "AQUANCON\n 3 1 3 1 3 2 2 K+ /\n/\n", "", BLOCK, "AQUANCON item 1"),
    (FET + CT + ANCON, "", BLOCK, "AQUCT item 1: aquifer 2 has no connections"),
    (FET + "AQUANCON\n 1 1 3 1 3 1 1 K+ /\n/\n", "", BLOCK, "AQUFETP item 1: aquifer 1 has no connections"),
    ("AQUFETP\n 1 1003 210 1.0E6 1.0E-4 20 1 0.1 /\n/\n" + ANCON, "", BLOCK, "AQUFETP item 8"),
    ("AQUCT\n 2 1001 220 150 0.25 2.0E-4 400 12 90 1 2 0.1 /\n/\n" + ANCON2, "", BLOCK, "AQUCT item 12"),
    (FET + ANCON + "AQUFLUX\n 3 1.0 /\n/\n", "", BLOCK, "AQUFLUX"),
    (FET + ANCON + "AQUNUM\n 3 1 1 1 1.0E6 1000 0.2 100 /\n/\n", "", BLOCK, "AQUNUM"),
    (FET + ANCON + "AQUCON\n 3 1 3 1 3 2 2 K+ /\n/\n", "", BLOCK, "AQUCON"),
    (FET + "AQUANCON\n 1 1 3 1 3 2 2 Q+ /\n/\n", "", BLOCK, "AQUANCON item 8"),
    (FET + "AQUANCON\n 1 1 4 1 3 2 2 K+ /\n/\n", "", BLOCK, "AQUANCON items 2-7"),
    (ANCON, "", BLOCK, "AQUANCON item 1"),
])
def test_refusals_name_keyword_and_item(tmp_path, body, actnum, geometry, match):
    d = read(tmp_path, body, actnum=actnum, geometry=geometry)
    with pytest.raises(ValueError, match=match):
        d.aquifers()


def test_explicit_coefficient_on_a_corner_point_grid_is_accepted(tmp_path):
    d = read(tmp_path, FET + "AQUANCON\n 1 1 3 1 3 2 2 K+ 100 /\n/\n", geometry=CORNER)
    (a,) = d.aquifers()
    assert a.cells.size == 9 and np.allclose(a.alpha, 1 / 9, rtol=1e-15)
