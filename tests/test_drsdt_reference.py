"""CPU: the restatement of the dissolution limits (drsdt_reference.py) against what it must reduce to.
  - caps of +inf: the capped cell IS cell_reference's cell, exactly, and the NumPy state update IS the oracle's update_state;
  - a capped cell with free gas and oil: rs is the cap with zero derivative slots, and the oil's b and mu (value and p-derivative) are
    those of cell_reference's OIL_ONLY cell at X = cap -- the undersaturated oil the rule says it holds, evaluated by code this helper
    does not share its branch logic with; the same for Rv against the GAS_ONLY cell;
  - a cap above the saturated ratio, and a tie, change nothing;
  - the caps of a time step: one addition, +inf where stated."""
import numpy as np
import pytest

import cell_edge_cases as E
import cell_reference as R
import drsdt_reference as D
from opmgpu import capi, decks

N = R.NAMES.index
GO, OO, GG = R.GAS_AND_OIL, R.OIL_ONLY, R.GAS_ONLY
# a few cells of every hydrocarbon state in both regions of both table sets that have caps to apply (no ROCKTAB needed for the rule)
CELLS = [dict(preg=0, sreg=0, p=E.P0, sw=E.SW0, sg=E.SG0, rs=E.RS0, rv=E.RV0, hc=GO),
         dict(preg=1, sreg=1, p=212.7 * E.BAR, sw=0.31, sg=0.22, rs=E.RS0, rv=E.RV0, hc=GO),
         dict(preg=0, sreg=1, p=E.P0, sw=E.SW0, sg=0.0, rs=E.RS0, rv=E.RV0, hc=OO),
         dict(preg=1, sreg=0, p=188.0 * E.BAR, sw=0.41, sg=0.0, rs=31.0, rv=E.RV0, hc=OO),
         dict(preg=0, sreg=1, p=E.P0, sw=E.SW0, sg=0.0, rs=E.RS0, rv=E.RV0, hc=GG),
         dict(preg=1, sreg=0, p=231.9 * E.BAR, sw=0.27, sg=0.0, rs=E.RS0, rv=0.7e-4, hc=GG)]


@pytest.mark.parametrize("tset", ["base", "vap"])
def test_infinite_caps_are_the_uncapped_cell(tset):
    tab = E.tables(tset)
    for c in CELLS:
        so_max = 0.7 if tset == "vap" else 0.0
        want, _ = R.cell(tab, so_max=so_max, **c)
        got, br = D.cell(tab, so_max=so_max, **c)
        assert not br["capped_s"] and not br["capped_v"]
        assert np.array_equal(got, want), c


@pytest.mark.parametrize("tset", ["base", "vap"])
@pytest.mark.parametrize("frac", [0.3, 0.9])
def test_capped_rs_is_the_undersaturated_oil_at_the_cap(tset, frac):
    tab = E.tables(tset)
    so_max = 0.7 if tset == "vap" else 0.0
    for c in CELLS[:2]:
        free, _ = R.cell(tab, so_max=so_max, **c)
        cap = frac * free[N("rsSat"), 0]
        got, br = D.cell(tab, so_max=so_max, rs_cap=cap, **c)
        assert br["capped_s"] and not br["capped_v"] and br["oil"] == "under"
        assert got[N("rs"), 0] == cap and np.all(got[N("rs"), 1:] == 0.0)
        assert got[N("rsSat"), 0] == cap and np.all(got[N("rsSat"), 1:] == 0.0)
        # the independent check: cell_reference's OIL_ONLY cell at X = cap (same p; its saturations differ, b_o and mu_o do not depend on them)
        oo = dict(c, hc=OO, rs=cap, sg=0.0)
        want, wbr = R.cell(tab, so_max=so_max, **oo)
        assert wbr["oil"] == "under"
        for name in ("b_o", "mu_o"):
            assert got[N(name), 0] == want[N(name), 0] and got[N(name), 1] == want[N(name), 1], (name, got[N(name)], want[N(name)])
            assert got[N(name), 2] == 0.0 and got[N(name), 3] == 0.0          # a constant rs: nothing through the third variable
        # and the cap changed the oil: it is not the saturated oil of the uncapped cell
        assert got[N("b_o"), 0] != free[N("b_o"), 0]
        # the gas side is untouched
        for name in ("b_g", "mu_g", "rv", "rvSat", "kr_g", "p_g"):
            assert np.array_equal(got[N(name)], free[N(name)]), name


@pytest.mark.parametrize("frac", [0.3, 0.9])
def test_capped_rv_is_the_undersaturated_gas_at_the_cap(frac):
    """saturation region 1 has zero capillary pressure: p_g == p in the capped cell and in the GAS_ONLY cell it is compared with"""
    tab = E.tables("base")
    for c in (dict(CELLS[0], sreg=1), CELLS[1]):
        free, _ = R.cell(tab, **c)
        cap = frac * free[N("rvSat"), 0]
        got, br = D.cell(tab, rv_cap=cap, **c)
        assert br["capped_v"] and not br["capped_s"] and br["gas"] == "under"
        assert got[N("rv"), 0] == cap and np.all(got[N("rv"), 1:] == 0.0)
        assert got[N("rvSat"), 0] == cap and np.all(got[N("rvSat"), 1:] == 0.0)
        gg = dict(c, hc=GG, rv=cap, sg=0.0)
        want, wbr = R.cell(tab, **gg)
        assert wbr["gas"] == "under" and want[N("p_g"), 0] == got[N("p_g"), 0]
        for name in ("b_g", "mu_g"):
            assert got[N(name), 0] == want[N(name), 0] and got[N(name), 1] == want[N(name), 1], (name, got[N(name)], want[N(name)])
            assert got[N(name), 3] == 0.0
        assert got[N("b_g"), 0] != free[N("b_g"), 0]
        for name in ("b_o", "mu_o", "rs", "rsSat"):
            assert np.array_equal(got[N(name)], free[N(name)]), name


def test_a_cap_above_the_curve_and_a_tie_do_not_bind():
    tab = E.tables("base")
    for c in CELLS:
        free, _ = R.cell(tab, **c)
        for f in (1.1, 1.0):          # 1.0: the cap equals the saturated ratio -- strict comparison, not capped
            got, br = D.cell(tab, rs_cap=f * free[N("rsSat"), 0], rv_cap=f * free[N("rvSat"), 0], **c)
            assert not br["capped_s"] and not br["capped_v"]
            assert np.array_equal(got, free)


def test_oil_only_cell_keeps_its_primary_variable():
    """an OIL_ONLY cell's rs is X whatever the cap; the cap shows in RSSAT alone"""
    tab = E.tables("base")
    c = CELLS[2]
    free, _ = R.cell(tab, **c)
    cap = 0.3 * free[N("rsSat"), 0]
    got, br = D.cell(tab, rs_cap=cap, **c)
    assert br["capped_s"] and got[N("rs"), 0] == c["rs"] and got[N("rs"), 3] == 1.0
    assert got[N("rsSat"), 0] == cap
    rest = [i for i, n in enumerate(R.NAMES) if n != "rsSat"]
    assert np.array_equal(got[rest], free[rest])


def test_caps_of_a_time_step():
    rng = np.random.default_rng(2)
    n = 50
    sg = np.where(rng.random(n) < 0.4, 0.0, rng.random(n) * 0.3)
    st = decks.State(np.full(n, 2e7), np.stack([np.full(n, 0.2), 0.8 - sg, sg], 1), rng.uniform(10, 150, n), rng.uniform(0, 4e-4, n), np.full(n, GO, np.int8))
    dt = 3.7 * decks.DAY
    rs_cap, rv_cap = D.caps(st, dt)
    assert np.all(np.isinf(rs_cap)) and np.all(np.isinf(rv_cap))
    rs_cap, rv_cap = D.caps(st, dt, drsdt=2.5e-7, drvdt=1e-12)
    assert np.array_equal(rs_cap, st.rs + 2.5e-7 * dt) and np.array_equal(rv_cap, st.rv + 1e-12 * dt)
    rs_cap, rv_cap = D.caps(st, dt, drsdt=0.0, free_only=True)
    assert np.array_equal(rs_cap[sg > 0], st.rs[sg > 0]) and np.all(np.isinf(rs_cap[sg == 0])) and (sg == 0).any() and np.all(np.isinf(rv_cap))


def test_update_state_without_caps_is_the_oracles(oracle):
    for tab, grid, prm, st, dx, _, _ in D.update_cases():
        zero = np.zeros(grid.nc, np.int32)
        g = D.update_state(tab, zero, zero, prm, dx, st)
        o = oracle.update_state(grid, tab, prm, dx, st)
        assert np.array_equal(g.hc, o.hc)
        assert np.allclose(g.p, o.p, rtol=1e-14, atol=0) and np.allclose(g.sat, o.sat, rtol=0, atol=1e-14)
        assert np.allclose(g.rs, o.rs, rtol=1e-13, atol=1e-13) and np.allclose(g.rv, o.rv, rtol=1e-13, atol=1e-18)


def test_update_state_with_caps_holds_the_caps():
    """with caps no cell ends above them -- switched to the capped saturated ratio, or left single-phase and limited --, some cells' outcome differs from the uncapped update's, and the cells within
    1e-9 of a tie (which the device test leaves out) are at most 1 % in every case: how CAP_SEED was chosen"""
    for tab, grid, prm, st, dx, rs_cap, rv_cap in D.update_cases():
        zero = np.zeros(grid.nc, np.int32)
        free = D.update_state(tab, zero, zero, prm, dx, st)
        got, margin = D.update_state(tab, zero, zero, prm, dx, st, rs_cap, rv_cap, with_margins=True)
        assert np.all(got.rs <= rs_cap) and np.all(got.rv <= rv_cap)               # every cell, whatever state it ends in
        kept = (got.hc == capi.HC_OIL_ONLY) & (st.hc == capi.HC_OIL_ONLY)
        n_limited = int((kept & (got.rs == rs_cap) & (st.rs < rs_cap)).sum())       # cells left OIL_ONLY whose rs rose to the cap and stopped there
        print("cells left OIL_ONLY and limited to their cap: %d" % n_limited)
        assert n_limited > 0
        assert (got.hc != free.hc).any() and (got.rs != free.rs).any() and (got.rv != free.rv).any()
        assert np.array_equal(got.p, free.p)
        print("cells within 1e-9 of a tie: %d of %d" % ((margin < 1e-9).sum(), grid.nc))
        assert (margin < 1e-9).mean() <= 0.01
