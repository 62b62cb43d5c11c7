"""The defining properties of Killough's scanning curves (the rule stated in include/opmgpu.h at opmgpu_set_hysteresis_model) on the numpy
restatement tests/killough_reference.py, and the twin: at a frozen history Killough's curve in a cell is Carlson's with ZERO shift on a
twin imbibition table of that cell -- which the UNCHANGED oracle evaluates, so its krg and kro there are the restated ones."""
import numpy as np
import pytest

import killough_cases as kc
import killough_reference as kref
from opmgpu import decks
from test_satfunc_options import _hyst_tables

A = 0.1


def _grid(nc=1, **kw):
    return decks.GridData(nc, np.zeros((0, 2), np.int32), [], np.ones(nc), np.zeros(nc), satnum=np.zeros(nc, np.int32), imbnum=np.ones(nc, np.int32), **kw)


def _gas():
    return kref.cell_systems(_hyst_tables(), _grid(), 0)["go"]


def test_the_quoted_figures():
    s = _gas()
    assert (s.sncrd, s.sncri, s.snmax) == (0.1, 0.3, 0.9)
    sncrt, m, R = kref.scan(s, 1.0 - 0.6, A)
    assert sncrt == pytest.approx(0.272117, abs=5e-7) and m == pytest.approx(1.8299, abs=5e-5) and R == pytest.approx(0.5, rel=1e-14)
    sncrt, m, R = kref.scan(s, 1.0 - 0.9, A)
    assert sncrt == pytest.approx(0.3, rel=1e-14) and m == pytest.approx(1.0, rel=1e-14) and R == pytest.approx(1.0, rel=1e-14)
    ow = kref.cell_systems(_hyst_tables(), _grid(), 0)["ow"]
    assert (ow.sncrd, ow.sncri, ow.snmax) == (pytest.approx(0.2), pytest.approx(0.4), pytest.approx(0.9))


@pytest.mark.parametrize("system", ["go", "ow"])
def test_continuous_at_the_turning_point(system):
    s = kref.cell_systems(_hyst_tables(), _grid(), 0)[system]
    for shy in np.linspace(s.sncrd + 0.01, s.snmax, 41):
        mdc = 1.0 - shy
        below = kref.krn(s, mdc, A, shy - 1e-12)          # scanning side
        assert 1.0 - (shy - 1e-12) > mdc
        assert below == pytest.approx(s.krnd(shy), abs=1e-10), shy
        # at and beyond the turning point: the drainage curve itself
        assert kref.krn(s, mdc, A, min(shy + 0.05, 1.0)) == s.krnd(min(shy + 0.05, 1.0))


@pytest.mark.parametrize("system", ["go", "ow"])
def test_turning_at_snmax_gives_the_imbibition_curve(system):
    s = kref.cell_systems(_hyst_tables(), _grid(), 0)[system]
    mdc = 1.0 - s.snmax
    for sn in np.linspace(0.0, s.snmax - 1e-9, 37):
        assert kref.krn(s, mdc, A, sn) == pytest.approx(s.krni(sn), rel=1e-13, abs=1e-15)
    # a turning point recorded beyond Snmax is clamped to it
    assert kref.scan(s, 1.0 - (s.snmax + 0.05), A) == pytest.approx(kref.scan(s, mdc, A), rel=1e-15)


@pytest.mark.parametrize("system", ["go", "ow"])
def test_trapped_saturation(system):
    s = kref.cell_systems(_hyst_tables(), _grid(), 0)[system]
    last = s.sncrd
    for shy in np.linspace(s.sncrd + 0.005, s.snmax, 60):
        mdc = 1.0 - shy
        sncrt, m, R = kref.scan(s, mdc, A)
        assert s.sncrd <= sncrt <= s.sncri + 1e-15
        assert sncrt >= last                              # a deeper invasion never lowers the trapped saturation
        last = sncrt
        for sn in (0.0, 0.5 * sncrt, sncrt):
            assert kref.krn(s, mdc, A, sn) == 0.0
        if R > 0.0:
            assert kref.krn(s, mdc, A, sncrt + 0.5 * (shy - sncrt)) > 0.0
    # a larger curvature parameter traps less at the same turning point (the denominator grows)
    assert kref.scan(s, 0.5, 0.5)[0] < kref.scan(s, 0.5, 0.1)[0] < kref.scan(s, 0.5, 0.0)[0]


def test_each_guard():
    tab = _hyst_tables()
    s = kref.cell_systems(tab, _grid(), 0)["go"]
    # kd <= 0: the turning point lies in the drainage curve's zero run
    sncrt, m, R = kref.scan(s, 1.0 - 0.05, A)
    assert (m, R) == (0.0, 0.0) and kref.krn(s, 1.0 - 0.05, A, 0.03) == 0.0 and kref.in_guard(s, 1.0 - 0.05)
    # ki <= 0: an imbibition curve that is zero at Snmax
    z = kref.System(s.krnd, lambda sn: 0.0, s.sncrd, s.sncri, s.snmax)
    assert kref.scan(z, 0.4, A)[1:] == (0.0, 0.0) and kref.krn(z, 0.4, A, 0.5) == 0.0
    # Snmax <= Sncri
    z = kref.System(s.krnd, s.krni, s.sncrd, 0.9, 0.9)
    assert kref.scan(z, 0.4, A)[1:] == (0.0, 0.0)
    # Sncri <= Sncrd: no trapping, and (imbibition == drainage) turning at Snmax is the drainage curve
    z = kref.System(s.krnd, s.krnd, s.sncrd, s.sncrd, s.snmax)
    assert kref.scan(z, 0.4, A)[0] == s.sncrd
    same = kref.cell_systems(tab, decks.GridData(1, np.zeros((0, 2), np.int32), [], [1.0], [0.0], satnum=[0], imbnum=[0]), 0)["go"]
    assert kref.scan(same, 0.4, A)[0] == same.sncrd
    for sn in (0.2, 0.5, 0.8):
        assert kref.krn(same, 1.0 - same.snmax, A, sn) == pytest.approx(same.krnd(sn), rel=1e-14)
    # no history: the drainage curve, m = R = 1
    assert kref.scan(s, kref.NO_HISTORY, A) == (0.0, 1.0, 1.0) and kref.krn(s, kref.NO_HISTORY, A, 0.4) == s.krnd(0.4)


def _twin_case(nc, seed):
    """nc cells with random histories; the tables with one twin imbibition region per cell appended (regions 2 .. nc + 1)"""
    tab = _hyst_tables()
    rng = np.random.default_rng(seed)
    mdc_ow, mdc_go = rng.uniform(0.15, 0.85, nc), rng.uniform(0.1, 0.95, nc)
    mdc_go[0], mdc_ow[0] = 0.97, 0.85                     # a guard cell in both systems (turning point in the zero run)
    mdc_go[1] = kref.NO_HISTORY                           # a cell without a gas history
    grid = _grid(nc)
    twin_tab, twin_grid = kc.twin_deck(tab, grid, mdc_ow, mdc_go, A)
    return tab, grid, twin_tab, twin_grid, mdc_ow, mdc_go


def test_the_twin_on_the_unchanged_oracle(oracle):
    """Killough in cell c == Carlson with zero shift on cell c's twin imbibition table: the oracle, which knows Carlson only, evaluates
    the restated krg and kro on the twin (its history planes set, its shifts zero)."""
    nc = 24
    tab, grid, twin_tab, twin_grid, mdc_ow, mdc_go = _twin_case(nc, seed=11)
    rng = np.random.default_rng(12)
    h = oracle.Hysteresis(nc)
    h.mdc_ow[:], h.mdc_go[:] = mdc_ow, mdc_go              # d_ow = d_go = 0: zero shift
    oracle.set_hysteresis(h)
    try:
        scanning = 0
        for _ in range(6):
            sg = rng.uniform(0.0, 0.8, nc)
            sw = rng.uniform(0.05, 1.0, nc) * (1.0 - sg)
            s = np.stack([sw, 1.0 - sw - sg, sg], axis=1)
            kr, _ = oracle.relperm_eps(twin_tab, twin_grid, s, np.arange(nc))
            for c in range(nc):
                krg, kro = kref.kr_cell(tab, grid, c, mdc_ow[c], mdc_go[c], A, sw[c], sg[c])
                # the twin's own rounding: its abscissae (x - A0) / m carry 2 roundings of O(1) numbers, met by slopes R m y' <= ~10
                assert kr[c][2] == pytest.approx(krg, rel=1e-12, abs=1e-14), (c, sw[c], sg[c])
                assert kr[c][1] == pytest.approx(kro, rel=1e-12, abs=1e-14), (c, sw[c], sg[c])
                scanning += (1.0 - sg[c]) > mdc_go[c]
        assert scanning > nc
    finally:
        oracle.set_hysteresis(None)
