"""Self-checks of the rock-region restatement (rock_reference.py) and the census of the edge set (rock_cases.py): CPU only.  The GPU tests
compare the device with these cells, so the census is asserted HERE: they cannot pass by leaving a branch out."""
import numpy as np
import pytest

import cell_reference as R
import rock_cases as RC
import rock_reference as K

U = 2.0 ** -52
PVM = R.NAMES.index("pvm")
ACC = [R.NAMES.index(n) for n in ("accum_w", "accum_o", "accum_g")]
MOB = [R.NAMES.index(n) for n in ("mob_w", "mob_o", "mob_g")]


@pytest.mark.parametrize("form", RC.FORMS)
def test_census_of_the_edge_set(form):
    C = RC.load(form)
    n = RC.census(C)
    print(form, C.nc, "cells:", n)
    for name in RC.CENSUS:
        assert n[name] >= RC.MIN_CELLS, (name, n[name])
    assert n["table lengths"] == [2, 3, 17]
    assert n["interior nodes hit"] == {1: [1], 2: list(range(1, 16))}           # every interior node of both tables that have one
    assert set(np.unique(C.rocknum)) == {0, 1, 2, 3}                              # three table regions and the ROCK form
    assert np.any(np.diff(C.rocknum) < 0) and np.any(np.diff(C.rocknum) > 0)      # shuffled
    assert C.regions.mode == K.IRREVERSIBLE


def test_history_is_the_running_minimum():
    inf = float("inf")
    p_min = np.array([inf, 2.0e7, 2.0e7, 2.0e7, inf])
    p = np.array([1.5e7, 2.5e7, 2.0e7, np.nextafter(2.0e7, 0.0), 3.0e7])
    h = K.history(p_min, p)
    assert np.array_equal(h, [1.5e7, 2.0e7, 2.0e7, np.nextafter(2.0e7, 0.0), 3.0e7])
    assert np.array_equal(K.history(h, p), h)                                     # idempotent


@pytest.mark.parametrize("form", RC.FORMS)
def test_multipliers_against_the_50_digit_cells(form):
    """the float64 restatement of the two look-ups against the 50-digit pvm (value and d/dp): within 2 ulp of the look-up's magnitude --
    its two rounded operations --, the slope within its one rounded division (relative 2 ulp: the differences are rounded too), and
    exactly 0 off the curve in BOTH"""
    C = RC.load(form)
    pv, tr, dpv, dtr, mpv, mtr = K.multipliers(C.regions, C.rocknum, C.state.p, C.p_min)
    tab = np.array([b["form"] == "table" for b in C.rock_recs])
    on = np.array([b["on_curve"] for b in C.rock_recs])
    ref = C.ref[:, PVM]
    assert np.all(np.abs(pv - ref[:, 0])[tab] <= 2 * U * mpv[tab])
    assert np.all(np.abs(pv - ref[:, 0])[~tab] <= 4 * U)                          # 1 + X + X^2 / 2, three roundings next to 1
    assert np.all(np.abs(dpv - ref[:, 1])[on] <= 4 * U * np.abs(ref[:, 1])[on] + 1e-300)
    assert np.all(dpv[tab & ~on] == 0.0) and np.all(ref[tab & ~on, 1] == 0.0)
    assert np.all(ref[:, 2:] == 0.0)                                              # no multiplier depends on Sw or X
    assert np.all(tr[~tab] == 1.0) and np.all(dtr[~on] == 0.0)
    assert (tab & ~on).sum() >= 3 * RC.MIN_CELLS


def test_a_cell_off_its_curve_is_the_plain_cell_times_two_constants():
    """accumulation and mobility of an off-curve cell against the cell WITHOUT any rock (cell_reference alone) times the float64
    multipliers: values and all three derivatives, to the few ulp of the float64 products"""
    C = RC.load("wog")
    pv, tr, _, _, _, _ = K.multipliers(C.regions, C.rocknum, C.state.p, C.p_min)
    plain = K._View(C.ref_tab, rocktab_n=0, rock_pref=0.0, rock_comp=0.0)
    off = [c for c, b in enumerate(C.rock_recs) if b["form"] == "table" and not b["on_curve"]][:12]
    for c in off:
        s = C.state
        o, _ = R.cell(plain, int(C.pvtnum[c]), int(C.satnum[c]), s.p[c], s.sat[c, 0], s.sat[c, 2], s.rs[c], s.rv[c], int(s.hc[c]))
        assert o[PVM, 0] == 1.0
        for idx, f in ((ACC, pv[c]), (MOB, tr[c])):
            want, got = o[idx] * f, C.ref[c][idx]
            assert np.all(np.abs(got - want) <= 8 * U * np.abs(want)), (c, got, want)


def test_tie_and_its_upper_neighbour():
    """p == p_min is on the curve (the slope), the next float above is off it (slope 0): the values agree to the step of one ulp of p,
    the derivatives do not"""
    C = RC.load("wog")
    p = C.state.p
    ties = [c for c, b in enumerate(C.rock_recs) if b["form"] == "table" and b["tie"] and b["search"].side == 0 and b["search"].at < 0]
    assert len(ties) >= RC.MIN_CELLS
    n = 0
    for c in ties:
        mates = np.flatnonzero((C.p_min == C.p_min[c]) & (C.rocknum == C.rocknum[c]) & (p == np.nextafter(p[c], np.inf)))
        for d in mates:
            n += 1
            assert C.rock_recs[c]["on_curve"] and not C.rock_recs[d]["on_curve"]
            assert C.ref[c, PVM, 1] != 0.0 and C.ref[d, PVM, 1] == 0.0
            assert abs(C.ref[c, PVM, 0] - C.ref[d, PVM, 0]) <= 2 * U * abs(C.ref[c, PVM, 0])
    assert n >= RC.MIN_CELLS


def test_reversible_is_the_curve_everywhere():
    C = RC.load("wog")
    ref, recs = RC.reversible(C)
    assert all(b["on_curve"] for b in recs)
    off = np.array([b["form"] == "table" and not b["on_curve"] for b in C.rock_recs])
    same = np.all(ref == C.ref, axis=(1, 2))
    assert np.all(same[~off]) and not np.any(same[off])
    # a ROCK-form region is elastic whatever the mode
    rock = np.array([b["form"] == "rock" for b in C.rock_recs])
    assert rock.sum() >= RC.MIN_CELLS and np.all(same[rock])


def test_on_curve_cell_is_the_cell_of_a_single_rocktab():
    """a region's cell on its curve against cell_reference alone on a FluidTables built with that region's table as THE rocktab"""
    from opmgpu import decks
    import cell_edge_cases as E
    C = RC.load("wog")
    for r in (0, 1, 2):
        tab = decks.FluidTables(**dict(_fluid_kwargs(), rocktab=RC.TABLES[r]))
        cells_ = [c for c, b in enumerate(C.rock_recs) if b["region"] == r and b["on_curve"]][:6]
        assert len(cells_) == 6
        for c in cells_:
            s = C.state
            o, br = R.cell(tab, int(C.pvtnum[c]), int(C.satnum[c]), s.p[c], s.sat[c, 0], s.sat[c, 2], s.rs[c], s.rv[c], int(s.hc[c]))
            assert np.array_equal(o, C.ref[c]) and br["rocktab"] == C.rock_recs[c]["search"]
    assert E.tables("base").rocktab_n == 0


def _fluid_kwargs():
    import cell_edge_cases as E
    pvto1 = [(0.9 * rs + 2, [(1.07 * p + 3, 1.02 * B, 0.95 * mu) for p, B, mu in col]) for rs, col in E._PVTO[:-1]]
    pvtg1 = [(1.05 * pg + 4, [(0.9 * rv, 1.03 * B, 0.97 * mu) for rv, B, mu in col]) for pg, col in E._PVTG]
    return dict(density_wog=[[1000.0, 700.0, 1.0], [1020.0, 740.0, 0.9]], pvtw=[[100.0, 1.02, 4.0e-5, 0.45, 2.0e-5], [150.0, 1.01, 4.5e-5, 0.5, 1.5e-5]],
                pvto=[E._PVTO, pvto1], pvtg=[E._PVTG, pvtg1], swof=E._SWOF, sgof=E._SGOF, rock=(100.0, 5.0e-5))
