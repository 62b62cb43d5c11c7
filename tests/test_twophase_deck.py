"""Oil-water decks on the host: ingest of the golden deck (tests/golden/decks/OILWATER_SMALL.DATA), the refused keywords, EQUIL without a
gas phase, and the restart file of a two-phase state."""
import datetime

import numpy as np
import pytest

from opmgpu import capi, deck as deckmod, decks, eclio, equil, schedule as schedmod
from opmgpu import wells as W

import twophase as tp


def _read(tmp_path, text, name="T.DATA"):
    return deckmod.read_deck(tp.write_deck(tmp_path / name, text))


# ------------------------------------------------------------------------------------------------------------------------------------------
# C1: the golden deck parses
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_golden_deck_parses():
    d = deckmod.read_deck(tp.DECK)
    assert d.phases() == "wo"
    t, g = d.tables(), d.grid()
    s = t.struct()
    assert t.phases == "wo" and s.active_phases == capi.PHASES_OIL_WATER
    assert t.n_sat == 2 and t.n_pvt == 1 and not t.has_disgas and not t.has_vapoil
    assert not s.sgof_ptr and not s.gas_node_ptr and not hasattr(t, "sgof_sg") and not hasattr(t, "gas_pg")
    assert np.array_equal(t.surface_density, [[1030.0, 820.0, 0.0]])
    assert g.nc == 120 and set(g.satnum) == {0, 1}
    # end points: the deck's water / oil ones, the table's where the deck gives none (SWU), and no gas end point of the deck's own
    assert np.array_equal(g.eps[0][:30], np.full(30, 0.12)) and np.array_equal(g.eps[2], np.ones(120)) and np.all(g.eps[4] == 0.0)
    assert set(g.eps_v) == {"KRO"}
    st = d.initial_state(t)
    assert np.all(st.sat[:, 2] == 0.0) and np.all(st.rs == 0.0) and np.all(st.rv == 0.0) and np.all(st.hc == capi.HC_GAS_AND_OIL)
    assert np.array_equal(st.sat[:, 1], 1.0 - st.sat[:, 0])
    sched = schedmod.Schedule(d, g, perm_md=(d.array("PERMX"), d.array("PERMY")), dz=d._cell_sizes()[2].ravel(),
                              dxdy=(d._cell_sizes()[0].ravel(), d._cell_sizes()[1].ravel()))
    assert [s_[0] / decks.DAY for s_ in sched.steps] == [10.0, 10.0, 20.0] and sched.start == datetime.date(2021, 1, 1)
    wl = sched.wells(0)
    assert wl.name == ["INJ", "PROD"] and wl.type == [W.INJECTOR, W.PRODUCER]
    assert np.array_equal(wl.comp_frac[0], [1.0, 0.0, 0.0]) and all(c[2][2] == 0.0 for cl in wl.controls for c in cl)
    # the gas-only RPTRST mnemonics select nothing, DEN / VISC the two active phases
    rpt = sched.rptrst[0]
    assert rpt["BG"] > 0 and rpt["KRG"] > 0 and rpt["PBPD"] > 0
    assert eclio.rptrst_arrays(rpt, "wo") == ["1OVERBO", "WAT_DEN", "OIL_DEN", "WAT_VISC", "OIL_VISC", "OILKR"]
    assert "GAS_DEN" in eclio.rptrst_arrays(rpt) and "PBUB" in eclio.rptrst_arrays(rpt)


def test_explicit_initial_state_without_gas(tmp_path):
    text = tp.deck_text().replace("EQUIL\n 2500 250 2528 0 2500 0 /\n", "PRESSURE\n 120*250 /\nSWAT\n 60*0.3 60*0.5 /\n")
    d = _read(tmp_path, text)
    t = d.tables(); d.grid()
    st = d.initial_state(t)
    assert np.array_equal(st.sat[:, 0], [0.3] * 60 + [0.5] * 60) and np.array_equal(st.sat[:, 1], 1.0 - st.sat[:, 0])
    assert np.all(st.sat[:, 2] == 0.0) and np.all(st.hc == capi.HC_GAS_AND_OIL) and np.all(st.p == 250 * decks.BAR)


# ------------------------------------------------------------------------------------------------------------------------------------------
# C2: refused keywords
# ------------------------------------------------------------------------------------------------------------------------------------------
def _with(after, add):
    text = tp.deck_text()
    assert after in text
    return text.replace(after, after + add, 1)


EXPLICIT = "PRESSURE\n 120*250 /\nSWAT\n 120*0.3 /\n"
# case -> deck text; NAMED below: the fragment of the message that names what is refused (specific to the case: every two-phase
# refusal mentions GAS, so the bare keyword would prove nothing)
REFUSED = {
    "DISGAS": lambda: _with("\nWATER\n", "DISGAS\n"),
    "VAPOIL": lambda: _with("\nWATER\n", "VAPOIL\n"),
    "STONE1": lambda: _with("\nPROPS\n", "STONE1\n"),
    "STONE2": lambda: _with("\nPROPS\n", "STONE2\n"),
    "STONE": lambda: _with("\nPROPS\n", "STONE\n"),
    "VAPPARS": lambda: _with("\nPROPS\n", "VAPPARS\n 2.0 0.5 /\n"),
    "SATOPTS HYSTER": lambda: _with("\nWATER\n", "SATOPTS\n HYSTER /\n"),
    "SGAS": lambda: tp.deck_text().replace("EQUIL\n 2500 250 2528 0 2500 0 /\n", EXPLICIT + "SGAS\n 120*0.0 /\n"),
    "RS": lambda: tp.deck_text().replace("EQUIL\n 2500 250 2528 0 2500 0 /\n", EXPLICIT + "RS\n 120*0.0 /\n"),
    "RV": lambda: tp.deck_text().replace("EQUIL\n 2500 250 2528 0 2500 0 /\n", EXPLICIT + "RV\n 120*0.0 /\n"),
    "GAS": lambda: tp.deck_text().replace(" 'INJ' 'WATER' 'OPEN' 'RATE' 300 1* 400 /", " 'INJ' 'GAS' 'OPEN' 'RATE' 300 1* 400 /"),
    "GRAT": lambda: tp.deck_text().replace(" 'PROD' 'OPEN' 'BHP' 5* 235 /", " 'PROD' 'OPEN' 'BHP' 2* 5000 2* 235 /"),
    "THP": lambda: tp.deck_text().replace(" 'PROD' 'OPEN' 'BHP' 5* 235 /", " 'PROD' 'OPEN' 'BHP' 5* 235 30 1 /"),
    "WELTARG GRAT": lambda: _with(" 'PROD' 'OPEN' 'BHP' 5* 235 /\n/\n", "WELTARG\n 'PROD' 'GRAT' 1000 /\n/\n"),
    "OIL GAS": lambda: tp.deck_text().replace("\nWATER\n", "\nGAS\n", 1),
    "WATER GAS": lambda: tp.deck_text().replace("\nOIL\nWATER\n", "\nWATER\nGAS\n", 1),
    "OIL": lambda: tp.deck_text().replace("\nOIL\nWATER\n", "\nOIL\n", 1),
}


NAMED = {"DISGAS": "DISGAS in a deck", "VAPOIL": "VAPOIL in a deck", "STONE1": "STONE1 in a deck", "STONE2": "STONE2 in a deck", "STONE": "STONE in a deck",
         "VAPPARS": "VAPPARS in a deck", "SATOPTS HYSTER": "SATOPTS HYSTER in a deck", "SGAS": "SGAS in the SOLUTION", "RS": "RS in the SOLUTION",
         "RV": "RV in the SOLUTION", "GAS": "WCONINJE INJ: GAS in a deck", "GRAT": "WCONPROD PROD: GRAT in a deck", "THP": "WCONPROD PROD: THP in a deck",
         "WELTARG GRAT": "WELTARG PROD: GRAT in a deck", "OIL GAS": "names the phases OIL GAS:", "WATER GAS": "names the phases WATER GAS:",
         "OIL": "names the phases OIL:"}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_keywords_are_named(tmp_path, what):
    d = _read(tmp_path, REFUSED[what]())
    with pytest.raises(ValueError) as e:
        t = d.tables()
        g = d.grid()
        d.initial_state(t)
        schedmod.Schedule(d, g, perm_md=(d.array("PERMX"), d.array("PERMY")), dz=d._cell_sizes()[2].ravel(),
                          dxdy=(d._cell_sizes()[0].ravel(), d._cell_sizes()[1].ravel()))
    assert NAMED[what] in str(e.value), str(e.value)


def test_twin_deck_is_accepted(tmp_path):
    d = _read(tmp_path, tp.twin_deck_text())
    assert d.phases() == "wog" and d.tables().struct().active_phases == 0 and hasattr(d.tables(), "sgof_sg")


# ------------------------------------------------------------------------------------------------------------------------------------------
# C3: EQUIL without a gas phase
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_equil_oil_water(tmp_path):
    d = deckmod.read_deck(tp.DECK)
    t, g = d.tables(), d.grid()
    st = d.initial_state(t)
    pw, po, pg = st.phase_pressure.T
    z = g.z
    rec_zwoc = 2528.0
    pvt = equil.HostPvt(t, 0)
    # hydrostatic consistency, phase by phase, between the layers of every column (the tolerance of test_equil.py's pressure pins: 1e-8
    # relative on the pressure differences' scale is what RK4 with 2000 steps leaves; here against a midpoint-density estimate: 1e-6)
    nx, ny, nz = d.dims
    col = np.arange(nx * ny)
    for k in range(nz - 1):
        a, b = col + nx * ny * k, col + nx * ny * (k + 1)
        for ph, (pp, rho) in enumerate(((pw, lambda p: pvt.b_w(p) * pvt.rho_w), (po, lambda p: pvt.b_o(p, 0.0, True) * pvt.rho_o))):
            free = (st.sat[a, 0] < 1.0 - 1e-6) & (st.sat[b, 0] < 1.0 - 1e-6) & (st.sat[a, 0] > g.eps[0][a] + 1e-6)      # no pressure fix-up at a saturation limit
            if not free.any():
                continue
            dp = (pp[b] - pp[a])[free]
            mid = 0.5 * (pp[a] + pp[b])[free]
            ref = np.array([rho(m) for m in mid]) * g.gravity * (z[b] - z[a])[free]
            assert np.allclose(dp, ref, rtol=1e-6), (k, ph)
    # capillary equilibrium in the transition zone: pcow(Sw) = p_o - p_w; water-filled below it
    cp = equil.CapPress(t, g, np.arange(g.nc))
    sw = st.sat[:, 0]
    trans = (sw > cp.swl + 1e-6) & (sw < cp.swu - 1e-6)
    assert trans.sum() >= 60
    assert np.allclose(cp.pcow(sw)[trans], (po - pw)[trans], rtol=0, atol=1e-6 * np.abs(po - pw).max() + 1e-6 * 0.6e5)      # the root finder's 1e-6 in Sw
    below = z > rec_zwoc
    assert below.any() and np.all(sw[below] == 1.0) and np.all(sw[~below] < 1.0)
    assert np.array_equal(pg, po) and np.array_equal(st.p, po)
    # the twin deck through the unchanged three-phase path: the same pressures and saturations
    d3 = _read(tmp_path, tp.twin_deck_text())
    t3 = d3.tables(); d3.grid()
    s3 = d3.initial_state(t3)
    assert np.allclose(s3.p, st.p, rtol=1e-12) and np.allclose(s3.sat, st.sat, rtol=0, atol=1e-12) and np.all(s3.sat[:, 2] == 0.0)


# ------------------------------------------------------------------------------------------------------------------------------------------
# C5: restart file of a two-phase state
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_restart_file_without_gas(tmp_path):
    d = deckmod.read_deck(tp.DECK)
    t, g = d.tables(), d.grid()
    st = d.initial_state(t)
    base = str(tmp_path / "OW")
    out = eclio.EclOutput(base, d.dims, g.active_index, datetime.date(2021, 1, 1), phases="wo")
    sd = {name: np.full(g.nc, float(k + 1)) for k, name in enumerate(capi.SIMDATA_NAMES)}
    mn = {m: 1 for m in ("BO", "BG", "DEN", "VISC", "KRG", "RSSAT", "RVSAT", "PBPD")}
    out.write_restart(0.0, st, extra=eclio.restart_simulator_data(mn, sd, "wo"))
    arrs = eclio.read_arrays(base + ".UNRST")
    names = [a[0] for a in arrs]
    ih = next(a[2] for a in arrs if a[0] == "INTEHEAD")
    assert ih[14] == 3
    assert "SGAS" not in names and "RS" not in names and "RV" not in names
    assert names[names.index("STARTSOL") + 1:names.index("ENDSOL")] == ["PRESSURE", "SWAT", "1OVERBO", "WAT_DEN", "OIL_DEN", "WAT_VISC", "OIL_VISC"]
    r = eclio.read_restart(base, 1)
    assert np.allclose(r["PRESSURE"], st.p / decks.BAR, rtol=1e-6) and np.allclose(r["SWAT"], st.sat[:, 0], atol=1e-7)
    assert next(a[2] for a in eclio.read_arrays(base + ".INIT") if a[0] == "INTEHEAD")[14] == 3
    # a three-phase file is what it was
    out3 = eclio.EclOutput(str(tmp_path / "WOG"), d.dims, g.active_index, datetime.date(2021, 1, 1))
    out3.write_restart(0.0, st)
    a3 = eclio.read_arrays(str(tmp_path / "WOG") + ".UNRST")
    assert next(a[2] for a in a3 if a[0] == "INTEHEAD")[14] == 7 and [a[0] for a in a3][-6:] == ["PRESSURE", "SWAT", "SGAS", "RS", "RV", "ENDSOL"]
    # compare() on the keywords present
    assert eclio.compare(base, base, restart_keywords=("PRESSURE", "SWAT"), summary=False) == []
