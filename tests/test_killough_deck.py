"""CPU: EHYSTR's model (item 2) and Killough's curvature parameter (item 4) from the deck to Deck.hysteresis_model(), the refusals, the
simulator's refusal of a backend that knows Carlson only, and the C ABI's two new entries (opmgpu_set_hysteresis_model,
opmgpu_get_hysteresis_scanning), on the golden deck tests/golden/decks/KILLOUGH_SMALL.DATA."""
import os

import numpy as np
import pytest

from opmgpu import capi
from opmgpu import deck as deckmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = os.path.join(ROOT, "tests", "golden", "decks", "KILLOUGH_SMALL.DATA")
CARLSON_DECK = os.path.join(ROOT, "tests", "golden", "decks", "satfuncEPS_D.DATA")
EHYSTR = "EHYSTR\n 0.1 2 1.0 0.15 KR /\n"


def _edited(tmp_path, name, record):
    text = open(DECK).read()
    assert text.count(EHYSTR) == 1
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write(text.replace(EHYSTR, record))
    return path


def test_killough_is_read_with_and_without_item_4(tmp_path):
    d = deckmod.read_deck(DECK)
    assert d.hysteresis() is True and d.hysteresis_model() == (capi.HYST_KILLOUGH, 0.15)
    g = d.grid()
    assert np.array_equal(g.satnum, np.zeros(108, np.int32)) and np.array_equal(g.imbnum, np.ones(108, np.int32))
    assert d.tables().n_sat == 2
    for rec in ("EHYSTR\n 0.1 2 1.0 1* KR /\n", "EHYSTR\n 1* 2 2* KR /\n"):
        d = deckmod.read_deck(_edited(tmp_path, "DEFAULTED.DATA", rec))
        assert d.hysteresis() is True and d.hysteresis_model() == (capi.HYST_KILLOUGH, 0.1)
    assert (capi.HYST_CARLSON, capi.HYST_KILLOUGH) == (0, 2)             # EHYSTR's own numbers


def test_a_carlson_deck_reads_as_before(tmp_path):
    d = deckmod.read_deck(CARLSON_DECK)
    assert d.hysteresis() is True and d.hysteresis_model() == (capi.HYST_CARLSON, 0.1)
    d = deckmod.read_deck(_edited(tmp_path, "CARLSON.DATA", "EHYSTR\n 0.1 0 0.1 0.3 KR /\n"))
    assert d.hysteresis() is True and d.hysteresis_model() == (capi.HYST_CARLSON, 0.3)
    d = deckmod.read_deck(_edited(tmp_path, "NOKEYWORD.DATA", ""))       # SATOPTS HYSTER without EHYSTR: the default model
    assert d.hysteresis() is True and d.hysteresis_model() == (capi.HYST_CARLSON, 0.1)
    text = open(DECK).read().replace("SATOPTS\n 'HYSTER' /\n", "")
    path = str(tmp_path / "NOHYST.DATA")
    open(path, "w").write(text)
    assert deckmod.read_deck(path).hysteresis() is False


@pytest.mark.parametrize("record", ["EHYSTR\n 0.1 1 1.0 0.1 KR /\n", "EHYSTR\n 0.1 3 1.0 0.1 KR /\n", "EHYSTR\n 0.1 4 1.0 0.1 KR /\n",
                                    "EHYSTR\n 0.1 7 1.0 0.1 KR /\n", "EHYSTR\n 0.1 2 1.0 0.1 BOTH /\n", "EHYSTR\n 0.1 2 1.0 0.1 PC /\n",
                                    "EHYSTR\n 0.1 2 /\n", "EHYSTR\n 0.1 0 1.0 0.1 BOTH /\n"])
def test_each_refusal_names_the_keyword(tmp_path, record):
    d = deckmod.read_deck(_edited(tmp_path, "REFUSED.DATA", record))
    with pytest.raises(ValueError, match="EHYSTR"):
        d.hysteresis()
    with pytest.raises(ValueError, match="EHYSTR"):
        d.hysteresis_model()


def test_the_simulator_refuses_a_backend_without_the_setter(oracle, tmp_path):
    """the CPU oracle knows Carlson's model only: a Killough deck on it is refused, naming the keyword (the PVCDO precedent); the same deck
    with item 2 = 0 is taken"""
    from opmgpu.simulator import Simulator
    from util import OracleBackend

    def oracle_model(grid, tables, params):
        return OracleBackend(oracle, grid, tables, params)
    assert not hasattr(OracleBackend, "setHysteresisModel")
    with pytest.raises(ValueError, match="EHYSTR"):
        Simulator(DECK, params=capi.default_params(), model_factory=oracle_model)
    sim = Simulator(_edited(tmp_path, "CARLSON.DATA", "EHYSTR\n 0.1 0 1.0 0.15 KR /\n"), params=capi.default_params(), model_factory=oracle_model)
    assert sim.grid.imbnum is not None


def test_the_c_abi_declares_the_two_entries():
    from opmgpu.model import GpuBlackoilModel
    assert "opmgpu_set_hysteresis_model" in capi.SIGNATURES and "opmgpu_get_hysteresis_scanning" in capi.SIGNATURES
    assert hasattr(GpuBlackoilModel, "setHysteresisModel") and hasattr(GpuBlackoilModel, "getHysteresisScanning")
    lib = capi.load()                        # raises if the library lacks a declared symbol
    assert lib.opmgpu_set_hysteresis_model is not None and lib.opmgpu_get_hysteresis_scanning is not None
    # without a context: refused, no crash
    assert lib.opmgpu_set_hysteresis_model(None, capi.HYST_KILLOUGH, 0.1) == capi.EINVAL
    assert lib.opmgpu_get_hysteresis_scanning(None, None, None, None, None, None, None) == capi.EINVAL
    header = open(os.path.join(ROOT, "include", "opmgpu.h")).read()
    assert "#define OPMGPU_HYST_CARLSON  0" in header and "#define OPMGPU_HYST_KILLOUGH 2" in header
