"""CPU: DRSDT / DRVDT from the SCHEDULE section to the per-report-step limits (opmgpu/schedule.py), every refusal, the golden deck
tests/golden/decks/DRSDT_SMALL.DATA end to end, the report-step driver's hand-over to the model, and the new C entries' declarations."""
import ctypes as C
import os

import numpy as np
import pytest

from opmgpu import capi, schedule as schedmod
from opmgpu import deck as deckmod
from opmgpu.decks import DAY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = os.path.join(ROOT, "tests", "golden", "decks", "DRSDT_SMALL.DATA")
OILWATER = os.path.join(ROOT, "tests", "golden", "decks", "OILWATER_SMALL.DATA")


def _schedule(path):
    d = deckmod.read_deck(path)
    nx, ny, nz = d.dims
    n = nx * ny * nz
    dx, dy, dz = d._cell_sizes()
    kx = d.array("PERMX", n, np.zeros(n))
    return schedmod.Schedule(d, d.grid(), perm_md=(kx, d.array("PERMY", n, kx)), dz=dz.ravel(), dxdy=(dx.ravel(), dy.ravel()), ntg=np.ones(n))


def _edited(tmp_path, name, *subs, src=DECK):
    text = open(src).read()
    for a, b in subs:
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write(text)
    return path


def test_golden_deck_end_to_end():
    d = deckmod.read_deck(DECK)
    t, g = d.tables(), d.grid()
    assert g.nc == 240 and t.has_disgas == 1 and t.has_vapoil == 0
    st = d.initial_state(t)
    assert np.all(st.hc == capi.HC_OIL_ONLY) and np.all(st.rs == 70.0) and np.all(st.sat[:, 2] == 0.0)
    s = _schedule(DECK)
    assert [dt for dt, _ in s.steps] == [10 * DAY, 10 * DAY]
    # DRSDT 0 / from the first report step, DRSDT 1e-3 FREE / from the second; per day -> per second; no DRVDT
    assert s.dissolution == [(0.0, False, None), (1e-3 / DAY, True, None)]
    w = s.wells(0)
    assert w.nw == 2 and list(w.name) == ["GINJ", "PROD"]


def test_values_options_units_and_persistence(tmp_path):
    vapoil = ("DISGAS\n", "DISGAS\nVAPOIL\n")
    pvtg = ("PVDG\n    20   0.0600   0.0125\n    80   0.0148   0.0140\n   150   0.0078   0.0162\n   230   0.0052   0.0190\n"
            "   320   0.0039   0.0225\n   450   0.0031   0.0270 /\n",
            "PVTG\n   100   0.0001  0.0110  0.015\n         0.0     0.0114  0.015 /\n   300   0.0004  0.0040  0.022\n         0.0     0.0042  0.022 /\n/\n")
    path = _edited(tmp_path, "BOTH.DATA", vapoil, pvtg,
                   ("DRSDT\n 0 /\nDATES", "DRSDT\n 0.25 ALL /\nDRVDT\n 2e-5 /\nDATES"),
                   ("DRSDT\n 1e-3 FREE /\nTSTEP\n 10 /", "TSTEP\n 5 /\nDRSDT\n 1e-3 FREE /\nTSTEP\n 5 4 /\nDRVDT\n 0 /\nDRSDT\n 7 /\nTSTEP\n 1 /"))
    s = _schedule(path)
    assert len(s.steps) == 5
    assert s.dissolution[0] == (0.25 / DAY, False, 2e-5 / DAY)
    assert s.dissolution[1] == s.dissolution[0]                                 # holds until replaced
    assert s.dissolution[2] == (1e-3 / DAY, True, 2e-5 / DAY) == s.dissolution[3]
    assert s.dissolution[4] == (7.0 / DAY, False, 0.0)                          # a new DRSDT without option: ALL again
    # a deck without the keywords: no limits at any step
    none = _edited(tmp_path, "NONE.DATA", ("DRSDT\n 0 /\n", ""), ("DRSDT\n 1e-3 FREE /\n", ""))
    assert _schedule(none).dissolution == [(None, False, None)] * 2


@pytest.mark.parametrize("subs, match", [
    ((("DRSDT\n 0 /", "DRSDT\n -0.1 /"),), "DRSDT.*negative"),
    ((("DRSDT\n 0 /", "DRSDT\n 0 SOME /"),), "DRSDT.*option"),
    ((("DRSDT\n 0 /", "DRSDT\n /"),), "DRSDT.*rate"),
    ((("DRSDT\n 0 /", "DRVDT\n 0 /"),), "DRVDT.*VAPOIL"),
    ((("DISGAS\n", ""), ("RS\n 240*70 /\n", "")), "DRSDT.*DISGAS"),
    ((("DRSDT\n 0 /", "DRSDTR\n 0 /"),), "DRSDTR"),
    ((("DRSDT\n 0 /", "DRVDTR\n 0 /"),), "DRVDTR"),
    ((("DRSDT\n 0 /", "DRSDTCON\n 0.04 /"),), "DRSDTCON"),
], ids=["negative", "option", "missing", "drvdt-without-vapoil", "drsdt-without-disgas", "DRSDTR", "DRVDTR", "DRSDTCON"])
def test_refusals_name_the_keyword(tmp_path, subs, match):
    path = _edited(tmp_path, "BAD.DATA", *subs)
    with pytest.raises(ValueError, match=match):
        _schedule(path)


@pytest.mark.parametrize("kw", ["DRSDT", "DRVDT"])
def test_refused_in_an_oil_water_deck(tmp_path, kw):
    text = open(OILWATER).read()
    assert text.count("\nSCHEDULE\n") == 1
    path = str(tmp_path / "OW.DATA")
    with open(path, "w") as f:
        f.write(text.replace("\nSCHEDULE\n", "\nSCHEDULE\n%s\n 0 /\n" % kw))
    with pytest.raises(ValueError, match=kw + ".*without GAS"):
        _schedule(path)


def test_driver_installs_the_limits_of_each_step():
    """the report-step driver hands each step's limits to the model before the step runs, and refuses a model that cannot take them"""
    from opmgpu.simulator import Simulator

    class Model:
        def __init__(self):
            self.calls, self.st = [], None

        def prepareStep(self, dt, state=None):
            if state is not None:
                self.st = state
            self.calls.append(("prepare", dt))

        def getState(self):
            return self.st

        def saveState(self):
            pass

        def restoreState(self):
            pass

        def relativeChange(self):
            return 0.0

        def nonlinearIteration(self, it, nonlinear_solver=None):
            return True, 0

    class Taking(Model):
        def setDissolutionLimits(self, drsdt=None, free_only=False, drvdt=None):
            self.calls.append(("limits", drsdt, free_only, drvdt))

    class Wrapped:
        """a well model in front of the reservoir model, as the driver builds one per report step"""

        def __init__(self, m):
            self.m = m

        def __getattr__(self, name):
            return getattr(self.m, name)

    sim = Simulator(DECK, model_factory=lambda grid, tables, params: Taking(), well_model_factory=lambda m, wl, ws: Wrapped(m))
    sim.run()
    calls = sim.model.calls
    lim = [c for c in calls if c[0] == "limits"]
    assert lim == [("limits", 0.0, False, None), ("limits", 1e-3 / DAY, True, None)]
    # each before the first prepareStep of its report step
    first, second = calls.index(lim[0]), calls.index(lim[1])
    assert ("prepare", 1.0) in calls[:first] and any(c[0] == "prepare" for c in calls[first + 1:second]) and any(c[0] == "prepare" for c in calls[second + 1:])
    bad = Simulator(DECK, model_factory=lambda grid, tables, params: Model(), well_model_factory=lambda m, wl, ws: Wrapped(m))
    with pytest.raises(ValueError, match="DRSDT"):
        bad.run()


def test_capi_exports_the_entries():
    dp = C.POINTER(C.c_double)
    want = {"opmgpu_set_dissolution_limits": [C.c_void_p, C.c_double, C.c_int, C.c_double], "opmgpu_begin_dissolution_step": [C.c_void_p, C.c_double],
            "opmgpu_get_dissolution_caps": [C.c_void_p, dp, dp], "opmgpu_set_dissolution_caps": [C.c_void_p, dp, dp]}
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "opmgpu.h")).read()
    for name, args in want.items():
        assert capi.SIGNATURES[name] == (C.c_int, args), name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is C.c_int
        assert "int %s(opmgpu_ctx* ctx" % name in header
    assert lib.opmgpu_set_dissolution_limits(None, 0.0, 0, -1.0) == capi.EINVAL       # no context: refused before anything is touched
    assert lib.opmgpu_begin_dissolution_step(None, 1.0) == capi.EINVAL
    assert lib.opmgpu_get_dissolution_caps(None, None, None) == capi.EINVAL and lib.opmgpu_set_dissolution_caps(None, None, None) == capi.EINVAL
    from opmgpu.model import GpuBlackoilModel
    for m in ("setDissolutionLimits", "dissolutionCaps", "setDissolutionCaps"):
        assert callable(getattr(GpuBlackoilModel, m)), m
    host = open(os.path.join(ROOT, "opm-simulators-legacy_amd", "host", "opmgpu.hpp")).read()
    assert "setDissolutionLimits" in host and "beginDissolutionStep" in host


def test_partition_refuses_a_model_with_limits():
    from opmgpu import partition

    class M:
        dissolution_limits = (0.0, False, None)
    with pytest.raises(ValueError, match="DRSDT"):
        partition.attach_comm(M(), None, 0, 2, b"")
