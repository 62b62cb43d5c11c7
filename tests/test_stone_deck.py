"""The deck's three-phase model keywords (STONE1, STONE2 = STONE, STONE1EX) through opmgpu/deck.py into the table struct of the C ABI
(opmgpu_tables.threephase_model / stone1_exponent)."""
import ctypes as C

import numpy as np
import pytest

from opmgpu import capi, decks
from opmgpu.deck import read_deck

DECK = """
RUNSPEC
DIMENS
 2 2 1 /
OIL
WATER
GAS
METRIC
%(runspec)s
TABDIMS
 2 1 /
PROPS
%(model)s
SWOF
 0.1 0.0 1.0 0.9   0.3 0.1 0.6 0.7   0.8 0.6 0.0 0.2   0.9 0.7 0.0 0.1 /
 0.15 0.0 0.9 0.5  0.4 0.2 0.4 0.3   0.85 0.7 0.0 0.0 /
SGOF
 0.0 0.0 1.0 0.2   0.2 0.1 0.6 0.6   0.8 0.7 0.0 2.0   0.9 1.0 0.0 2.1 /
 0.0 0.0 0.9 0.0   0.3 0.2 0.3 0.1   0.75 0.8 0.0 0.3  0.85 0.9 0.0 0.4 /
PVDO
 1 1.0 1.2  400 0.95 1.3 /
PVDG
 1 1.0 0.01  400 0.005 0.03 /
PVTW
 1.0 1.0 4.0e-5 0.96 0.0 /
DENSITY
 700 1000 1 /
END
"""


def _tables(tmp_path, model="", runspec=""):
    path = tmp_path / "S.DATA"
    path.write_text(DECK % {"model": model, "runspec": runspec})
    return read_deck(str(path)).tables()


def _exponents(struct, n):
    return None if not struct.stone1_exponent else np.ctypeslib.as_array(struct.stone1_exponent, shape=(n,)).copy()


def test_no_keyword_is_the_default_model(tmp_path):
    t = _tables(tmp_path)
    assert t.n_sat == 2 and t.threephase_model == capi.KRO_DEFAULT == 0
    s = t.struct()
    assert s.threephase_model == 0 and not s.stone1_exponent


@pytest.mark.parametrize("kw", ["STONE2", "STONE"])
def test_stone2(tmp_path, kw):
    t = _tables(tmp_path, kw)                                     # (the struct points into the arrays `t` owns)
    s = t.struct()
    assert s.threephase_model == capi.KRO_STONE2 == 2 and not s.stone1_exponent
    assert s.n_sat_regions == 2 and s.swof_ptr[2] == 7            # the keyword is a flag: the tables behind it are read as before


def test_stone1_with_exponents(tmp_path):
    t = _tables(tmp_path, "STONE1\nSTONE1EX\n 1.0 /\n 0.7 /")
    s = t.struct()
    assert s.threephase_model == capi.KRO_STONE1 == 1
    assert np.array_equal(_exponents(s, 2), [1.0, 0.7])


def test_stone1_default_exponent(tmp_path):
    t = _tables(tmp_path, "STONE1")
    assert np.array_equal(_exponents(t.struct(), 2), [1.0, 1.0])
    t = _tables(tmp_path, "STONE1\nSTONE1EX\n 1* /\n 2.5 /")
    assert np.array_equal(_exponents(t.struct(), 2), [1.0, 2.5])


@pytest.mark.parametrize("model,runspec", [("STONE1\nSTONE2", ""), ("STONE\nSTONE1", ""), ("STONE2\nSTONE", ""),
                                           ("STONE2", "SATOPTS\n HYSTER /"), ("STONE1", "SATOPTS\n HYSTER /"),
                                           ("STONE1\nSTONE1EX\n 1.0 /", ""), ("STONE1\nSTONE1EX\n 1.0 /\n 0.0 /", ""),
                                           ("STONE1\nSTONE1EX\n 1.0 /\n -1.0 /", "")])
def test_refusals(tmp_path, model, runspec):
    with pytest.raises(ValueError):
        _tables(tmp_path, model, runspec)


def test_the_table_struct_ends_with_the_two_fields():
    names = [n for n, _ in capi.Tables._fields_]
    assert names[-2:] == ["threephase_model", "stone1_exponent"]
    assert names[-3] == "rocktab_transmult"                       # appended: every earlier offset stays
    assert capi.Tables.threephase_model.offset == capi.Tables.rocktab_transmult.offset + 8
    assert capi.Tables.stone1_exponent.offset == capi.Tables.threephase_model.offset + 8
    assert C.sizeof(capi.Tables) == capi.Tables.stone1_exponent.offset + 8


def test_table_builders_leave_the_default():
    for t in (decks.satfunc_standard_tables(), decks.satfunc_standard_tables(regions=2), decks.fluid_data_tables()):
        s = t.struct()
        assert s.threephase_model == 0 and not s.stone1_exponent
    t = decks.satfunc_standard_tables(regions=2, threephase_model=capi.KRO_STONE1, stone1_exponent=[1.0, 0.7])
    assert t.struct().threephase_model == 1 and np.array_equal(_exponents(t.struct(), 2), [1.0, 0.7])
    with pytest.raises(ValueError):
        decks.satfunc_standard_tables(regions=2, stone1_exponent=[1.0])
