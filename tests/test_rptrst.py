"""RPTRST ingest and what it selects for the restart file (no GPU): the mnemonic list of SOLUTION and SCHEDULE (opmgpu/deck.py,
opmgpu/schedule.py), the mnemonic -> array selection of getRestartData (SimulatorFullyImplicitBlackoilOutput.hpp:585-845) and the
conversion of each array class to the deck's units (opmgpu/eclio.py)."""
import os
import re

import numpy as np

from opmgpu import deck as deckmod, eclio, schedule as schedmod
from opmgpu.decks import BAR, CP

DECK = os.path.join(os.path.dirname(__file__), "golden", "decks", "SCHEDULE_SMALL.DATA")
OFF = {k: 0 for k in deckmod.RPTRST_MNEMONICS}


def _deck(tmp_path, solution=None, schedule=()):
    """SCHEDULE_SMALL with an RPTRST record at the end of SOLUTION and others after the k-th report step of the SCHEDULE (k = 0: before
    the first DATES)"""
    text = open(DECK).read()
    if solution is not None:
        text = text.replace("SCHEDULE\n", "RPTRST\n %s /\nSCHEDULE\n" % solution, 1)
    for k, rec in schedule:
        kw = "RPTRST\n %s /\n" % rec
        if k == 0:
            text = text.replace("DATES\n", kw + "DATES\n", 1)
        elif k == 1:
            text = text.replace("TSTEP\n 10 20 /", kw + "TSTEP\n 10 20 /", 1)
        elif k == 2:
            text = text.replace("TSTEP\n 10 20 /", "TSTEP\n 10 /\n" + kw + "TSTEP\n 20 /", 1)
    path = str(tmp_path / "RPT.DATA")
    open(path, "w").write(text)
    return path


def _schedule(path):
    d = deckmod.read_deck(path)
    return d, schedmod.Schedule(d, d.grid())


def test_parse_mnemonics():
    on = lambda **kw: dict(OFF, **kw)      # noqa: E731
    assert deckmod.parse_rptrst([]) == OFF
    assert deckmod.parse_rptrst(["BASIC=2"]) == OFF                                   # BASIC is not kept
    assert deckmod.parse_rptrst(["BASIC=2", "DEN", "VISC", "KRW", "PBPD"]) == on(DEN=1, VISC=1, KRW=1, PBPD=1)
    assert deckmod.parse_rptrst(["BASIC=2", "den", "BO=3", "FLOWS", "ALLPROPS=1"]) == on(DEN=1, BO=3)      # unknown ones ignored
    assert deckmod.parse_rptrst(["BO", "BO=0", "KRG=0", "RSSAT=1"]) == on(RSSAT=1)    # NAME=0 switches a mnemonic off
    assert deckmod.parse_rptrst(["BASIC", "=", 2.0, "VWAT", "=", 1.0, "BG=", 2.0]) == on(VWAT=1, BG=2)     # blanks around '='
    assert deckmod.parse_rptrst([2.0, 0.0, 1.0]) == OFF                               # the positional integer form selects nothing
    assert set(deckmod.parse_rptrst(["DEN"])) == set(deckmod.RPTRST_MNEMONICS)


def test_deck_without_rptrst_selects_nothing(tmp_path):
    d, s = _schedule(_deck(tmp_path))
    assert d.rptrst() == OFF
    assert len(s.rptrst) == len(s.steps) == 3 and all(r == OFF for r in s.rptrst)
    assert all(eclio.rptrst_arrays(r) == [] for r in s.rptrst)


def test_solution_rptrst_holds_until_schedule_replaces_it(tmp_path):
    d, s = _schedule(_deck(tmp_path, "BASIC=2 BO DEN VISC KRW KRG RSSAT PBPD", [(1, "BASIC=2 BW")]))
    assert [st[0] / 86400.0 for st in s.steps] == [10.0, 10.0, 20.0]                  # the schedule itself is unchanged
    first = dict(OFF, BO=1, DEN=1, VISC=1, KRW=1, KRG=1, RSSAT=1, PBPD=1)
    assert d.rptrst() == first
    # a SCHEDULE RPTRST applies from its report step onwards and REPLACES the list (getRestartKeywords(reportStep)): no union with the old one
    assert s.rptrst == [first, dict(OFF, BW=1), dict(OFF, BW=1)]
    # the deck's LAST RPTRST (the SCHEDULE one) must not leak into the SOLUTION list
    assert d.rptrst()["BW"] == 0


def test_schedule_rptrst_positions_and_switching_off(tmp_path):
    _, s = _schedule(_deck(tmp_path, "DEN", [(0, "KRO VOIL=2"), (2, "KRO=0 BASIC=2")]))
    assert s.rptrst == [dict(OFF, KRO=1, VOIL=2), dict(OFF, KRO=1, VOIL=2), OFF]      # before the first step: the SOLUTION list never applies
    _, s = _schedule(_deck(tmp_path, None, [(2, "PBPD")]))
    assert s.rptrst == [OFF, OFF, dict(OFF, PBPD=1)]
    # the wells of a step do not depend on RPTRST being there
    _, s0 = _schedule(_deck(tmp_path))
    assert [sorted(st[1]) for st in s.steps] == [sorted(st[1]) for st in s0.steps]


def test_mnemonic_to_array_selection():
    sel = lambda *names: eclio.rptrst_arrays(dict(OFF, **{n: 1 for n in names}))      # noqa: E731
    assert sel() == []
    assert sel("BW") == ["1OVERBW"] and sel("BO") == ["1OVERBO"] and sel("BG") == ["1OVERBG"]
    assert sel("DEN") == ["WAT_DEN", "OIL_DEN", "GAS_DEN"]
    assert sel("VISC") == ["WAT_VISC", "OIL_VISC", "GAS_VISC"]
    assert sel("VWAT") == ["WAT_VISC"] and sel("VOIL") == ["OIL_VISC"] and sel("VGAS") == ["GAS_VISC"]
    assert sel("VISC", "VWAT") == ["WAT_VISC", "OIL_VISC", "GAS_VISC"]                # no array twice
    assert sel("VGAS", "VWAT") == ["WAT_VISC", "GAS_VISC"]
    assert sel("KRW") == ["WATKR"] and sel("KRO") == ["OILKR"] and sel("KRG") == ["GASKR"]
    assert sel("RSSAT") == ["RSSAT"] and sel("RVSAT") == ["RVSAT"] and sel("PBPD") == ["PBUB", "PDEW"]
    # file order = the order getRestartData inserts them in, whatever the order of the mnemonics
    assert sel("PBPD", "KRG", "DEN", "BO") == ["1OVERBO", "WAT_DEN", "OIL_DEN", "GAS_DEN", "GASKR", "PBUB", "PDEW"]
    assert eclio.rptrst_arrays(dict(OFF, DEN=0, BW=2)) == ["1OVERBW"]                 # positive = on
    every = eclio.rptrst_arrays({k: 1 for k in deckmod.RPTRST_MNEMONICS})
    from opmgpu import capi
    assert every == list(capi.SIMDATA_NAMES) and len(every) == capi.SIMDATA_K == 16


def test_unit_conversion_of_each_array_class():
    from opmgpu import capi
    si = {"1OVERBW": [0.99, 1.0, 1.01], "1OVERBO": [0.9, 0.8, 0.95], "1OVERBG": [90.0, 180.0, 200.0],
          "WAT_DEN": [1001.0, 1002.0, 1003.0], "OIL_DEN": [650.0, 700.0, 720.0], "GAS_DEN": [90.0, 120.0, 150.0],
          "WAT_VISC": [0.96e-3, 0.97e-3, 0.98e-3], "OIL_VISC": [1.1e-3, 1.2e-3, 0.94e-3], "GAS_VISC": [1e-5, 2e-5, 1.5e-5],
          "WATKR": [0.0, 0.25, 0.7], "OILKR": [1.0, 0.4, 0.0], "GASKR": [0.0, 0.1, 1.0],
          "RSSAT": [100.0, 125.5, 0.0], "RVSAT": [1e-4, 4e-4, 0.0], "PBUB": [200.0e5, 251.0e5, 0.0], "PDEW": [100.0e5, 0.0, 333.0e5]}
    assert set(si) == set(capi.SIMDATA_NAMES)
    sd = {k: np.array(v) for k, v in si.items()}
    for name in ("1OVERBW", "1OVERBO", "1OVERBG", "WATKR", "OILKR", "GASKR", "WAT_DEN", "OIL_DEN", "GAS_DEN", "RSSAT", "RVSAT"):
        assert np.array_equal(eclio.simdata_to_deck_units(name, sd[name]), sd[name]), name      # pure numbers, kg/m3, Sm3/Sm3: as they are
    for name in ("WAT_VISC", "OIL_VISC", "GAS_VISC"):
        assert np.array_equal(eclio.simdata_to_deck_units(name, sd[name]), sd[name] / CP), name  # Pa s -> cP
    assert np.allclose(eclio.simdata_to_deck_units("OIL_VISC", sd["OIL_VISC"]), [1.1, 1.2, 0.94], rtol=1e-15)
    for name in ("PBUB", "PDEW"):
        assert np.array_equal(eclio.simdata_to_deck_units(name, sd[name]), sd[name] / BAR), name  # Pa -> bar, like PRESSURE
    assert list(eclio.simdata_to_deck_units("PBUB", sd["PBUB"])) == [200.0, 251.0, 0.0]
    # the dict handed to write_restart: selected arrays only, converted, in file order; the input is left alone
    extra = eclio.restart_simulator_data(dict(OFF, PBPD=1, VOIL=1, BW=1), sd)
    assert list(extra) == ["1OVERBW", "OIL_VISC", "PBUB", "PDEW"]
    assert np.array_equal(extra["OIL_VISC"], sd["OIL_VISC"] / CP) and np.array_equal(extra["PDEW"], sd["PDEW"] / BAR)
    assert sd["PBUB"][0] == 200.0e5


def test_extra_arrays_sit_between_rv_and_endsol_in_order(tmp_path):
    from opmgpu.decks import State
    import datetime
    st = State(np.full(3, 250.0 * BAR), np.tile([0.25, 0.75, 0.0], (3, 1)), np.full(3, 100.0), np.zeros(3), np.full(3, 2, np.int8))
    out = eclio.EclOutput(str(tmp_path / "X"), (3, 1, 1), np.arange(3), datetime.date(2020, 1, 1))
    sd = {"OIL_VISC": np.array([1.1e-3, 1.2e-3, 0.94e-3]), "PBUB": np.array([200e5, 251e5, 0.0]), "PDEW": np.zeros(3), "1OVERBW": np.ones(3)}
    extra = eclio.restart_simulator_data(dict(OFF, PBPD=1, VOIL=1, BW=1), sd)
    extra["SOMAX"] = np.full(3, 0.75)
    out.write_restart(10.0, st, extra=extra)
    names = [a[0] for a in eclio.read_arrays(str(tmp_path / "X") + ".UNRST")]
    i = names.index("RV")
    assert names[i:] == ["RV", "1OVERBW", "OIL_VISC", "PBUB", "PDEW", "SOMAX", "ENDSOL"]
    got = eclio.read_restart(str(tmp_path / "X"), 1)
    assert np.array_equal(got["OIL_VISC"], np.float32(sd["OIL_VISC"] / CP)) and np.array_equal(got["PBUB"], np.float32([200.0, 251.0, 0.0]))
    assert all(re.fullmatch(r"[A-Z0-9_]{1,8}", n) for n in eclio._ARRAY_ORDER)         # every name fits an 8-character keyword
