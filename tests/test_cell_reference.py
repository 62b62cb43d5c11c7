"""The 50-digit cell reference (cell_reference.py) against answers worked by hand, and the CPU oracle against the reference over the
edge-case cells (cell_edge_cases.py), slot by slot.  No GPU.  Run with -s to see the census and the error table."""
import numpy as np
import pytest

import cell_edge_cases as E
import cell_reference as R
from opmgpu import capi, decks

BAR = decks.BAR


def one(tab, preg, sreg, **kw):
    a = dict(p=E.P0, sw=E.SW0, sg=E.SG0, rs=E.RS0, rv=E.RV0, hc=E.GO, so_max=0.0)
    a.update(kw)
    out, br = R.cell(tab, preg, sreg, a["p"], a["sw"], a["sg"], a["rs"], a["rv"], a["hc"], a["so_max"])
    return {n: out[k] for k, n in enumerate(R.NAMES)}, br


def test_reference_known_answers():
    """Cells of cell_edge_cases.tables() worked by hand from the deck numbers (PVT region 0; B in rm3/sm3, p in bar; ib(B) = 1 / B).

    1. Saturated oil ON a node: free gas, p = 140 bar = node 2 of the six saturated pressures 50, 90, 140, 185, 235, 300.  A node belongs to
       the segment it starts, so d b_o / d p is the RIGHT slope (ib(1.21) - ib(1.15)) / 45 bar = -9.58198586657e-9 / Pa and not the left one
       (ib(1.15) - ib(1.09)) / 50 bar = -9.57319505385e-9 / Pa; the value is ib(1.15) either way.
       The exception is node 1: p = 90 bar is still segment 0, slope (ib(1.09) - ib(1.05)) / 40 bar = -8.73743993010e-9 / Pa (the right one
       would be -9.57319505385e-9).
    2. Undersaturated oil: oil only, rs = 67.5 = half way between the nodes rs = 55 and 80, p = 250 bar.  Column of rs = 55 (140, 190, 260,
       350, 420 bar): segment 190..260, s1 = ib(1.143) + (ib(1.135) - ib(1.143)) * 60 / 70.  Column of rs = 80 (185, 240, 300, 390 bar):
       segment 240..300, s2 = ib(1.203) + (ib(1.196) - ib(1.203)) * 10 / 60.  b_o = (s1 + s2) / 2, d b_o / d rs = (s2 - s1) / 25,
       d b_o / d p = ((ib(1.135) - ib(1.143)) / 70 bar + (ib(1.196) - ib(1.203)) / 60 bar) / 2.
    3. Saturated gas: free oil, saturation region 1 (no capillary pressure: p_g = p), p = 140 bar = half way between 110 and 170 bar:
       b_g = (ib(0.0108) + ib(0.0070)) / 2, rv = rvSat = (0.00020 + 0.00031) / 2, d rv / d p = 0.00011 / 60 bar.
    4. Undersaturated gas: gas only, the same pressure, rv = 0.0001.  Column of 110 bar (rv = 0, 0.00005, 0.00012, 0.0002): segment
       0.00005..0.00012, s1 = ib(0.0112) + (ib(0.0110) - ib(0.0112)) * 5 / 7.  Column of 170 bar (0, 0.00015, 0.00031): segment 0..0.00015,
       s2 = ib(0.0074) + (ib(0.0072) - ib(0.0074)) / 1.5.  b_g = (s1 + s2) / 2, d b_g / d p = (s2 - s1) / 60 bar.
    5. The interpolated blend zone: saturation region 1 (Swco = 0, krow falls with slope -1 from 1, krog with slope -2 from 1), Sw = 0,
       Sg = 7.5e-6, so d = Sg = 0.75 eps.  kow = 1 - 7.5e-6, kgo = 1 - 1.5e-5, k2 = (kow + kgo) / 2 = 1 - 1.125e-5, k1 = Sg kgo / d = kgo,
       al = (eps - d) / (eps / 2) = 1 / 2:  kro = (k2 + k1) / 2 = 1 - 1.3125e-5.  d / d Sg: k2' = -1.5, k1' = -2, al' = -2e5, so
       kro' = k2' al + k1' (1 - al) + (k2 - k1) al' = -0.75 - 1 + 3.75e-6 * (-2e5) = -2.5.  d / d Sw = 0: Sw is not above Swco.
    """
    tab = E.tables()
    ib = lambda B: 1.0 / B
    close = lambda a, b: a == pytest.approx(b, rel=1e-12, abs=0.0)
    # 1
    q, br = one(tab, 0, 0, p=140 * BAR)
    assert br["psat"].at == 2 and br["psat"].seg == 2 and br["oil"] == "sat"
    assert close(q["b_o"][0], ib(1.15)) and close(q["b_o"][1], (ib(1.21) - ib(1.15)) / (45 * BAR)) and q["b_o"][2] == 0 and q["b_o"][3] == 0
    assert abs(q["b_o"][1] / ((ib(1.15) - ib(1.09)) / (50 * BAR)) - 1) > 5e-4          # the two slopes are told apart
    q, br = one(tab, 0, 0, p=90 * BAR)
    assert br["psat"].at == 1 and br["psat"].seg == 0
    assert close(q["b_o"][0], ib(1.09)) and close(q["b_o"][1], (ib(1.09) - ib(1.05)) / (40 * BAR))
    # 2
    q, br = one(tab, 0, 0, p=250 * BAR, rs=67.5, hc=E.OO)
    assert br["oil"] == "under" and br["rs_node"].seg == 2 and [c.seg for c in br["oil_col"]] == [1, 1]
    s1 = ib(1.143) + (ib(1.135) - ib(1.143)) * 60 / 70
    s2 = ib(1.203) + (ib(1.196) - ib(1.203)) * 10 / 60
    assert close(q["b_o"][0], (s1 + s2) / 2) and close(q["b_o"][3], (s2 - s1) / 25)
    assert close(q["b_o"][1], ((ib(1.135) - ib(1.143)) / (70 * BAR) + (ib(1.196) - ib(1.203)) / (60 * BAR)) / 2)
    assert q["rs"].tolist() == [67.5, 0, 0, 1]
    # 3
    q, br = one(tab, 0, 1, p=140 * BAR)
    assert br["gas"] == "sat" and br["pg"].seg == 1 and q["p_g"][0] == 140 * BAR
    assert close(q["b_g"][0], (ib(0.0108) + ib(0.0070)) / 2) and close(q["rv"][0], 0.000255) and close(q["rv"][1], 0.00011 / (60 * BAR))
    # 4
    q, br = one(tab, 0, 1, p=140 * BAR, rv=0.0001, hc=E.GG)
    assert br["gas"] == "under" and [c.seg for c in br["gas_col"]] == [1, 0]
    s1 = ib(0.0112) + (ib(0.0110) - ib(0.0112)) * 5 / 7
    s2 = ib(0.0074) + (ib(0.0072) - ib(0.0074)) / 1.5
    assert close(q["b_g"][0], (s1 + s2) / 2) and close(q["b_g"][1], (s2 - s1) / (60 * BAR))
    assert q["rv"].tolist() == [0.0001, 0, 0, 1]
    # 5
    q, br = one(tab, 0, 1, sw=0.0, sg=7.5e-6)
    assert br["blend"] == "interp" and not br["above_swco"] and br["d"] == 7.5e-6
    assert close(q["kr_o"][0], 1 - 1.3125e-5) and q["kr_o"][1] == 0 and q["kr_o"][2] == 0
    assert q["kr_o"][3] == pytest.approx(-2.5, rel=1e-9)       # (3.75e-6 is formed from numbers next to 1: 1e-16 / 3.75e-6 of it is lost by hand too)


def test_oracle_against_reference(oracle, capsys):
    """oracle.cell_props within 1e-12 of the reference in every (property, slot) of every group of cell_edge_cases.hc_groups, over the whole
    edge-case set (plain double arithmetic with divisions), except in the EXPLAINED slots of the interpolated blend zone, bounded at
    what cell_edge_cases.oracle_limits derives.  Prints the census and the tables (DESIGN section 7a has the figures)."""
    sets, cen = E.load()
    names = R.NAMES[:oracle.NPROP]
    with capsys.disabled():
        print("\ncensus (cells in region 0, region 1 by the reference's branch record):")
        for k, v in cen.items():
            print("  %-26s %3d %3d" % (k, v[0], v[1]))
    tabs = {}
    for ts, C in sets.items():
        err, lim = E.error_table(C, E.oracle_props(oracle, C), names), E.oracle_limits(C, names)
        for g in err:
            tabs.setdefault(g, []).append(err[g])
            bad = np.argwhere(err[g] > lim[g])
            assert bad.size == 0, [(ts, g, names[i], R.SLOTS[s], err[g][i, s], lim[g][i, s]) for i, s in bad]
    with capsys.disabled():
        for g, t in tabs.items():
            print("\noracle against the reference, group '%s':\n%s" % (g, E.format_table(E.worst(t), names)))


def test_decimal_fallback_agrees(monkeypatch):
    """cell_reference.py falls back on the standard library's decimal where mpmath is missing: the same arithmetic at the same 50 digits.
    Every cell of the two small sets and every 7th of the large one agree between the two within 2 ulp of the slot's largest entry (the
    50-digit results differ in their last digits; rounding them to float64 can differ by one ulp of an entry)."""
    if R.mpmath is None:
        pytest.skip("mpmath is missing: the suite already runs on decimal")
    sets, _ = E.load()
    monkeypatch.setattr(R, "BACKEND", "decimal")
    for ts, C in sets.items():
        pick = np.arange(0, C.nc, 7 if C.nc > 100 else 1)
        st = decks.State(C.state.p[pick], C.state.sat[pick], C.state.rs[pick], C.state.rv[pick], C.state.hc[pick])
        ref, recs = R.cells(C.tab, C.pvtnum[pick], C.satnum[pick], st, C.so_max[pick])
        assert recs == [C.recs[c] for c in pick]
        s = np.abs(C.ref[pick]).max(0)
        assert (np.abs(ref - C.ref[pick]) <= 2 * 2.0 ** -52 * s).all(), ts


MAPPING_TOL = 1e-13


@pytest.mark.parametrize("tset", E.TSETS)
def test_oracle_assembly_of_isolated_cells(oracle, tset):
    """On a grid without connections the Jacobian is block diagonal: block (a, k) of cell c is matbalscale[a] * pv/dt * d accum_a / d(p, Sw,
    X)[k] and the residual pv/dt * (accum_a - accum0_a).  test_gpu_cell_edges.py checks the device's assembly against the reference
    through this mapping; here it is confirmed for the oracle's assemble, at the first assembly and at a second state, with the
    normalisation of the GPU test (per slot and group, cell_edge_cases.error_table) at 1e-13: the oracle's accumulation terms are within
    4e-15 of the reference and the mapping adds two multiplications and a division."""
    C = E.load()[0][tset]
    grid, dt = C.grid(), 3 * decks.DAY
    scale = np.asarray(capi.default_params().matbalscale[:])
    rowptr, col = oracle.pattern(grid)
    assert np.array_equal(col, np.arange(C.nc))
    names = ["accum_w", "accum_o", "accum_g"]
    acc = C.ref[:, [R.NAMES.index(n) for n in names]]                     # [nc][3][4]
    pvdt = np.asarray(grid.pv) / dt
    f = scale[None, :, None] * pvdt[:, None, None]
    st2, so_max2, perm = C.shifted()
    acc0 = None
    try:
        for st, so_max, src in ((C.state, C.so_max, np.arange(C.nc)), (st2, so_max2, perm)):       # cell i holds the state of cell src[i]
            def at_source(a):
                out = np.empty_like(a)
                out[src] = a
                return out
            oracle.set_sat_oil_max(so_max if tset == "vap" else None)
            r, val, acc0, _ = oracle.assemble(grid, C.tab, dt, st, rowptr, col, scale=tuple(scale), accum0=acc0)
            for g, e in E.error_table(C, at_source(val.reshape(-1, 3, 3) / f), names, (1, 2, 3)).items():
                assert e.max() < MAPPING_TOL, (g, e)
            excess = r.reshape(3, C.nc).T / pvdt[:, None] - (acc[src][:, :, 0] - acc[:, :, 0])
            if src is not perm:
                assert np.all(r == 0.0)
            for g, e in E.error_table(C, (acc[:, :, 0] + at_source(excess))[:, :, None], names, (0,)).items():
                assert e.max() < MAPPING_TOL, (g, e)
    finally:
        oracle.set_sat_oil_max(None)


def test_blend_bound_is_the_conditioning_of_the_rule():
    """The bound of the EXPLAINED slots (cell_edge_cases.oracle_limits) rests on a claim: ANY float64 evaluation of d kro / d Sg where the
    law divides by d < 2 eps is off by up to 2 ulp(1) * 2 / eps.  A third evaluation, plain float64 and ordered unlike the oracle's and
    the device's (kro = k1 + al (k2 - k1), the quotient rule written out), bears it out on the blend-zone cells: within the bound
    everywhere, and past 1e-12 of the slot's largest entry somewhere -- 1e-12 is not attainable there."""
    C = E.load()[0]["base"]
    zone = E.hc_groups(C)[E.BLEND_ZONE]
    T = R.Tables(C.tab)
    k = R.NAMES.index("kr_o")
    err = []
    for c in zone:
        b, S = C.recs[c], T.sat(int(C.satnum[c]))
        slope = lambda x, y, s: 0.0 if s.side != 0 else (y[s.seg + 1] - y[s.seg]) / (x[s.seg + 1] - x[s.seg])
        value = lambda x, y, s, v: y[0] if s.side < 0 else (y[-1] if s.side > 0 else y[s.seg] + slope(x, y, s) * (v - x[s.seg]))
        swco, sg, d = S["sw"][0], b["sg"], b["d"]
        swp = b["sw"] if b["above_swco"] else swco
        kow, skow = value(S["sw"], S["krow"], b["krow"], b["swow"]), slope(S["sw"], S["krow"], b["krow"])
        kgo, skgo = value(S["sg"], S["krog"], b["krog"], d), slope(S["sg"], S["krog"], b["krog"])
        k1 = (sg * kgo + (swp - swco) * kow) / d
        dk1 = (kgo + sg * skgo + (swp - swco) * skow - k1) / d
        dkro = dk1
        if b["blend"] == "interp":
            al = (E.EPS - d) / (E.EPS / 2)
            dkro = dk1 + (-2.0 / E.EPS) * ((kow + kgo) / 2 - k1) + al * ((skow + skgo) / 2 - dk1)
        err.append(abs(dkro - C.ref[c, k, 3]))
    scale = np.abs(C.ref[zone, k, 3]).max()
    assert max(err) <= E.BLEND_ABS, (max(err), E.BLEND_ABS)
    assert max(err) > E.ORACLE_TOL * scale, (max(err), scale)
    print("third float64 evaluation of d kro / d Sg in the blend zone: worst %.2e absolute, bound %.2e" % (max(err), E.BLEND_ABS))
