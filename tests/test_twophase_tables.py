"""Oil-water tables on the host: decks.FluidTables(phases="wo"), the ctypes view and the C header agree on opmgpu_tables.active_phases."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from opmgpu import capi, decks

import twophase as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "opmgpu.h")


def test_two_phase_tables_carry_the_flag_and_no_gas_arrays():
    t = tp.tables()
    s = t.struct()
    assert t.phases == "wo" and s.active_phases == capi.PHASES_OIL_WATER == 1
    assert s.has_disgas == 0 and s.has_vapoil == 0 and s.threephase_model == capi.KRO_DEFAULT
    for name, _ in capi.Tables._fields_:
        if name.startswith("gas_") or name.startswith("sgof_"):
            assert not getattr(s, name), name                      # NULL
            assert not hasattr(t, name), name
    assert s.swof_ptr and s.oil_node_ptr and s.pvtw
    assert np.all(t.surface_density[:, 2] == 0.0) and np.array_equal(t.surface_density[:, :2], tp.DENSITY_WO)


def test_three_phase_tables_are_unchanged():
    for t in (decks.satfunc_standard_tables(), decks.fluid_data_tables(), tp.twin_tables()):
        assert t.phases == "wog" and t.struct().active_phases == capi.PHASES_ALL == 0
    assert decks.satfunc_standard_tables().has_disgas == 1 and decks.fluid_data_tables().has_disgas == 0
    assert capi.Tables().active_phases == 0                          # a zero-initialised struct: water, oil and gas


@pytest.mark.parametrize("kw", [dict(phases="og"), dict(phases="wg"), dict(phases="o"), dict(phases="wo", disgas=True),
                                dict(phases="wo", vapoil=True), dict(phases="wo", vappars=(0.0, 0.5)),
                                dict(phases="wo", threephase_model=capi.KRO_STONE2), dict(phases="wo", sgof=[[(0, 0, 1, 0), (0.9, 1, 0, 0)]])])
def test_refused_table_sets(kw):
    base = dict(density_wog=tp.DENSITY_WO[:1], pvtw=tp.PVTW[:1], pvto=[tp._dead_oil(tp.PVDO[0])], pvtg=None, swof=tp.SWOF[:1], sgof=None,
                rock=tp.ROCK)
    base.update(kw)
    with pytest.raises(ValueError):
        decks.FluidTables(**base)


def test_ctypes_view_and_c_header_agree_on_active_phases(tmp_path):
    """the field lies between threephase_model and stone1_exponent, in the bytes alignment left free: compile the header and compare"""
    src = tmp_path / "off.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "opmgpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d\\n", offsetof(opmgpu_tables, threephase_model), offsetof(opmgpu_tables, active_phases),'
                   ' offsetof(opmgpu_tables, stone1_exponent), sizeof(opmgpu_tables), (int)OPMGPU_PHASES_OIL_WATER); return 0; }\n')
    exe = tmp_path / "off"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])          # (the compiler the library's own Makefile uses)
    o_model, o_phases, o_eta, size, flag = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert o_model == capi.Tables.threephase_model.offset and o_eta == capi.Tables.stone1_exponent.offset
    assert o_phases == capi.ACTIVE_PHASES_OFFSET == o_model + 4
    assert size == C.sizeof(capi.Tables)
    assert flag == capi.PHASES_OIL_WATER
    t = capi.Tables()
    t.active_phases = capi.PHASES_OIL_WATER
    assert bytes(t)[o_phases:o_phases + 4] == (1).to_bytes(4, sys.byteorder) and t.threephase_model == 0 and not t.stone1_exponent
    hdr = open(HEADER).read()
    assert re.search(r"int32_t\s+active_phases;", hdr) and "OPMGPU_PHASES_OIL_WATER = 1" in hdr


def test_create_with_the_flag_reaches_the_device_check():
    """without a GPU, opmgpu_create of a two-phase deck ends in OPMGPU_ENODEVICE like every other (with one it succeeds)"""
    lib = capi.load()
    g = tp.grid(3, 3, 2)
    ctx = C.c_void_p()
    prm = capi.default_params()
    st = lib.opmgpu_create(C.byref(ctx), 0, C.byref(g.struct()), C.byref(tp.tables().struct()), C.byref(prm))
    if lib.opmgpu_device_count() > 0:
        assert st == capi.OK and ctx
        lib.opmgpu_destroy(ctx)
    else:
        assert st == capi.ENODEVICE and not ctx
