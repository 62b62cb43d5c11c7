"""ROCKCOMP / ROCKNUM / ROCKOPTS in the deck reader (opmgpu/deck.py: rock_regions()), the RockRegions value class, the refusals, and the
report-step driver's handling of a model that cannot take rock regions: CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from opmgpu import capi, decks
from opmgpu.deck import read_deck
from opmgpu.decks import BAR

DECK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decks", "ROCKCOMP_SMALL.DATA")


def variant(tmp_path, subs=(), drop=(), name="V.DATA"):
    """the golden deck with regular-expression substitutions and whole keywords dropped"""
    text = open(DECK).read()
    for kw in drop:
        text, n = re.subn(r"(?ms)^%s\n.*?/\n(?=[A-Z])" % kw, "", text, count=1)
        assert n == 1, kw
    for a, b in subs:
        text, n = re.subn(a, b, text, count=1)
        assert n == 1, a
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(text)
    return path


def test_golden_deck_reaches_rock_regions():
    d = read_deck(DECK)
    g = d.grid()
    r = d.rock_regions()
    assert isinstance(r, decks.RockRegions) and r.mode == capi.ROCK_IRREVERSIBLE and r.nregions == 2
    assert r.rocknum.dtype == np.int32 and np.array_equal(r.rocknum, np.repeat([0, 1], [50, 25])) and r.rocknum.size == g.nc
    assert np.array_equal(r.tab_ptr, [0, 4, 7]) and r.tab_ptr.dtype == np.int32
    assert np.array_equal(r.tab_p, np.array([100.0, 200.0, 300.0, 400.0, 100.0, 300.0, 400.0]) * BAR)
    assert np.array_equal(r.tab_pvmult, [0.90, 0.94, 1.0, 1.02, 0.985, 1.0, 1.005])
    assert np.array_equal(r.tab_transmult, [0.50, 0.70, 1.0, 1.10, 0.95, 1.0, 1.02])
    assert np.array_equal(r.rock_pref, [300.0 * BAR] * 2) and np.array_equal(r.rock_comp, [4.0e-5 / BAR] * 2)
    loc = r.local([60, 3, 74])
    assert np.array_equal(loc.rocknum, [1, 0, 1]) and loc.tab_p is r.tab_p and loc.mode == r.mode


def test_defaults_region_array_and_rock_form(tmp_path):
    # REVERS is the default of item 1, 1 table of item 2; without ROCKOPTS the region array is PVTNUM (absent: every cell in region 1)
    d = read_deck(variant(tmp_path, [(r"IRREVERS 2 /", "/")], drop=("ROCKOPTS", "ROCKNUM")))
    r = d.rock_regions()
    assert r.mode == capi.ROCK_REVERSIBLE and r.nregions == 1 and np.all(r.rocknum == 0) and np.array_equal(r.tab_ptr, [0, 4])
    # SATNUM names the array; a region without a ROCKTAB record takes the ROCK form
    sat = "SATNUM\n 25*1 50*2 /\n"
    d = read_deck(variant(tmp_path, [(r"1\* 1\* ROCKNUM /", "PRESSURE NOSTORE SATNUM /"), (r"ROCKNUM\n 50\*1 25\*2 /\n", sat),
                                    (r"(?m)^   100\.  0\.985 0\.95\n   300\.  1\.00  1\.00\n   400\.  1\.005 1\.02 /\n", "")]))
    r = d.rock_regions()
    assert np.array_equal(r.rocknum, np.repeat([0, 1], [25, 50])) and np.array_equal(r.tab_ptr, [0, 4, 4])
    assert r.rock_comp[1] == 4.0e-5 / BAR and r.rock_pref[1] == 300.0 * BAR
    # ROCKNUM of the deck is not read unless ROCKOPTS names it
    d = read_deck(variant(tmp_path, drop=("ROCKOPTS",)))
    assert np.all(d.rock_regions().rocknum == 0)


def test_deck_without_rockcomp_reads_as_ever(tmp_path):
    """no ROCKCOMP: rock_regions() is None and tables() carries the FIRST ROCK / ROCKTAB record for every cell, whatever else is there"""
    d = read_deck(variant(tmp_path, drop=("ROCKCOMP",)))
    assert d.rock_regions() is None
    t = d.tables()
    assert t.rocktab_n == 4 and np.array_equal(t.rocktab_p, np.array([100.0, 200.0, 300.0, 400.0]) * BAR)
    assert np.array_equal(t.rocktab_pvmult, [0.90, 0.94, 1.0, 1.02]) and t.rock_pref == 300.0 * BAR and t.rock_comp == 4.0e-5 / BAR
    # and with it the tables are the same ones: the regions ride next to them
    t2 = read_deck(DECK).tables()
    assert t2.rocktab_n == 4 and np.array_equal(t2.rocktab_transmult, t.rocktab_transmult)
    other = os.path.join(os.path.dirname(DECK), "DRSDT_SMALL.DATA")
    assert read_deck(other).rock_regions() is None and read_deck(other).tables().rocktab_n == 0


@pytest.mark.parametrize("subs, match", [
    ([(r"IRREVERS 2 /", "HYSTER 2 /")], r"ROCKCOMP item 1.*HYSTER"),
    ([(r"IRREVERS 2 /", "BOBERG 2 /")], r"ROCKCOMP item 1.*BOBERG"),
    ([(r"IRREVERS 2 /", "REVLIMIT 2 /")], r"ROCKCOMP item 1.*REVLIMIT"),
    ([(r"IRREVERS 2 /", "PALM-MAN 2 /")], r"ROCKCOMP item 1.*PALM-MAN"),
    ([(r"IRREVERS 2 /", "ELASTIC 2 /")], r"ROCKCOMP item 1"),
    ([(r"IRREVERS 2 /", "IRREVERS 0 /")], r"ROCKCOMP item 2"),
    ([(r"IRREVERS 2 /", "IRREVERS 2 YES /")], r"ROCKCOMP item 3"),
    ([(r"1\* 1\* ROCKNUM /", "STRESS 1* ROCKNUM /")], r"ROCKOPTS item 1.*STRESS"),
    ([(r"1\* 1\* ROCKNUM /", "1* STORE ROCKNUM /")], r"ROCKOPTS item 2.*STORE"),
    ([(r"1\* 1\* ROCKNUM /", "1* 1* FIPNUM /")], r"ROCKOPTS item 3"),
    ([(r"50\*1 25\*2 /", "50*1 25*3 /")], r"ROCKNUM.*region 3.*ROCKCOMP item 2"),
    ([(r"50\*1 25\*2 /", "50*0 25*2 /")], r"ROCKNUM.*region 0"),
    ([(r"IRREVERS 2 /", "IRREVERS 3 /")], r"ROCK: no record for region 3"),
])
def test_refusals_name_keyword_and_item(tmp_path, subs, match):
    d = read_deck(variant(tmp_path, subs))
    with pytest.raises(ValueError, match=match):
        d.rock_regions()


def test_rock_regions_value_class():
    r = decks.RockRegions([1, 0, 2], [(100.0, 1e-5), (1.0, 0.0), (200.0, 2e-5)], [None, [(50.0, 0.9, 0.8), (150.0, 1.0, 1.0)], None], irreversible=True)
    assert r.nregions == 3 and np.array_equal(r.tab_ptr, [0, 0, 2, 2]) and r.mode == capi.ROCK_IRREVERSIBLE
    assert np.array_equal(r.tab_p, [50.0 * BAR, 150.0 * BAR]) and np.array_equal(r.rock_comp, [1e-5 / BAR, 0.0, 2e-5 / BAR])
    assert decks.RockRegions([0], [(1.0, 0.0)]).mode == capi.ROCK_REVERSIBLE
    with pytest.raises(ValueError):
        decks.RockRegions([0], [(1.0, 0.0)], [None, None])


def test_driver_installs_regions_and_refuses_a_model_that_cannot_take_them(oracle):
    """the report-step driver hands the regions to the model before the first step, seeds the history from the initial state, and refuses
    a model without setRockRegions -- the CPU oracle behind the host well model would run table 1 in every cell without a word"""
    from opmgpu.simulator import Simulator
    from util import OracleBackend

    class Model:
        """takes the driver's set-up calls; no step is run"""
        nc = 75

        def __init__(self):
            self.calls = []

        def prepareStep(self, dt, state=None):
            self.calls.append("prepare")

    class Taking(Model):
        def setRockRegions(self, regions):
            self.calls.append(("regions", regions))

        def updateRockHistory(self):
            self.calls.append("history")

    sim = Simulator(DECK, model_factory=lambda grid, tables, params: Taking())
    regs = [c for c in sim.model.calls if isinstance(c, tuple)]
    assert len(regs) == 1 and regs[0][1].mode == capi.ROCK_IRREVERSIBLE and regs[0][1].nregions == 2
    assert "prepare" in sim.model.calls[:sim.model.calls.index(regs[0])]          # behind the initial state
    assert "history" not in sim.model.calls                                       # (run() seeds it)
    with pytest.raises(ValueError, match="ROCKCOMP.*setRockRegions"):
        Simulator(DECK, model_factory=lambda grid, tables, params: Model())
    # the oracle-backed model of the host-well tests is such a model
    with pytest.raises(ValueError, match="ROCKCOMP.*setRockRegions"):
        Simulator(DECK, model_factory=lambda grid, tables, params: OracleBackend(oracle, grid, tables, params))


def test_capi_declares_the_entries():
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    want = {"opmgpu_set_rock_regions": [C.c_void_p, C.POINTER(capi.RockRegionsSpec)], "opmgpu_update_rock_history": [C.c_void_p],
            "opmgpu_get_rock_history": [C.c_void_p, dp], "opmgpu_set_rock_history": [C.c_void_p, dp],
            "opmgpu_get_rock_multipliers": [C.c_void_p, dp, dp]}
    for name, args in want.items():
        assert capi.SIGNATURES[name] == (C.c_int, args), name
    f = dict(capi.RockRegionsSpec._fields_)
    assert list(f) == ["nregions", "mode", "rocknum", "rock_pref", "rock_comp", "tab_ptr", "tab_p", "tab_pvmult", "tab_transmult"]
    assert f["nregions"] is C.c_int32 and f["rocknum"] is ip or f["rocknum"] == ip
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "opmgpu.h")).read()
    for name in want:
        assert re.search(r"\bint %s\(" % name, header), name
    assert (capi.ROCK_REVERSIBLE, capi.ROCK_IRREVERSIBLE) == (0, 1)
    assert "#define OPMGPU_ROCK_REVERSIBLE 0" in header and "#define OPMGPU_ROCK_IRREVERSIBLE 1" in header
