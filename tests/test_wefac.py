"""Well efficiency factors (WEFAC) without a GPU: the reference subclass against its parent, the host well model (opmgpu/wells.py) against
the reference subclass (tests/wefac_reference.py), and the SCHEDULE reader on tests/golden/decks/WEFAC_SMALL.DATA."""
import os

import numpy as np
import pytest

from opmgpu import capi, decks, deck as deckmod, schedule, wells as W
from test_wells_host import _setup
from util import OracleBackend
from wefac_reference import WefacOracleModel, arrays

DECK = os.path.join(os.path.dirname(__file__), "golden", "decks", "WEFAC_SMALL.DATA")
EFF = (0.8, 0.5)              # injector, producer of the _setup() deck


def with_factors(wl, eff):
    """the same Wells object carrying one efficiency factor per well"""
    wl.efficiency = [float(e) for e in eff]
    assert len(wl.efficiency) == wl.nw
    return wl


def seeded_state(wl, p):
    """WellState with a small rate in the pressure-controlled wells (the dead-well knife edge, as tests/test_oracle_wells.py starts)"""
    ws = W.WellState(wl, p)
    for w in range(wl.nw):
        if wl.ctrl_type[w] == W.BHP:
            ws.qs[w] = (1e-5 if wl.type[w] == W.INJECTOR else -1e-5) * np.asarray(wl.comp_frac[w])
    return ws


def test_reference_with_unit_factors_is_its_parent(oracle):
    """e_w = 1 for every well: 1 * x is exact, so the subclass walks its parent's Newton path bit for bit"""
    from oracle.wells import CoupledOracleModel
    grid, tab, st, wl = _setup()
    prm = capi.default_params()
    a = CoupledOracleModel(grid, tab, prm, wl, arrays(seeded_state(wl, st.p)))
    b = WefacOracleModel(grid, tab, prm, wl, arrays(seeded_state(wl, st.p)), np.ones(wl.nw))
    a.prepareStep(2 * decks.DAY, st); b.prepareStep(2 * decks.DAY, st)
    for it in range(2):
        a.assemble(it == 0); b.assemble(it == 0)
        assert np.array_equal(a.r, b.r) and np.array_equal(a.E, b.E), it
        assert a.getConvergence() == b.getConvergence()
        assert np.array_equal(a.solveJacobianSystem(), b.solveJacobianSystem()) and np.array_equal(a.dy, b.dy), it
        a.updateState(); b.updateState()
        assert np.array_equal(a.st.p, b.st.p) and np.array_equal(a.st.sat, b.st.sat) and np.array_equal(a.ws.bhp, b.ws.bhp) and np.array_equal(a.ws.qs, b.ws.qs)


def test_wells_keep_their_interface_and_refuse_bad_factors():
    grid, tab, st, wl = _setup()
    assert np.array_equal(wl.efficiency_factors(), [1.0, 1.0])
    cp, cells = wl.arrays()                                  # two arrays, as before
    assert cp.dtype == np.int32 and cells.dtype == np.int32 and cp.tolist() == [0, 3, 5]
    wl.add_well("P2", W.PRODUCER, 2500.0, [7], 1e-12, (0.0, 1.0, 0.0), (W.BHP, 200 * decks.BAR), efficiency=0.25)
    assert np.array_equal(wl.efficiency_factors(), [1.0, 1.0, 0.25])
    for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="efficiency"):
            W.Wells().add_well("X", W.PRODUCER, 2500.0, [0], 1e-12, (0.0, 1.0, 0.0), (W.BHP, 1e7), efficiency=bad)


def test_host_assembly_is_linear_in_the_factor(oracle):
    """At a fixed state the host model's cell-row terms (residual, explicit Schur complement, right-hand side) are e_w times the unweighted
    ones -- to 2 ulp of each entry: S = e Jcc - (e B) D^-1 C sums products of once-rounded e-multiples -- and the well rows are unchanged"""
    grid, tab, st, wl = _setup()
    be = OracleBackend(oracle, grid, tab, capi.default_params(), wells=wl.arrays())
    be.prepareStep(decks.DAY, st); be.assemble(True)
    pp = be.perfProps(wl.nperf).reshape(wl.nperf, 9, 4)
    out = {}
    for name, eff in (("one", (1.0, 1.0)), ("e", EFF)):
        w = with_factors(_setup()[3], eff)
        wh = W.StandardWellsHost(w, grid.z, tab.surface_density[0])
        ws = W.WellState(w, st.p)
        ws.qs[0] = [2000.0 / 86400.0, 0.0, 0.0]; ws.bhp[0] = 300 * decks.BAR
        ws.qs[1] = [0.0, -1e-3, 0.0]
        wh.compute_connection_pressures(pp, ws)
        out[name] = wh.assemble(pp, ws) + (wh.flux_eq.copy(), wh.ctrl_eq.copy(), ws.perf_rates.copy())
    one, e = out["one"], out["e"]
    e_perf = np.repeat(EFF, np.diff(wl.connpos))
    assert np.array_equal(e[0], -(e_perf[:, None] * -one[0]))                                 # resid_delta: one product, exact restatement
    assert np.array_equal(e[1], one[1])
    nblk = np.diff(wl.connpos) ** 2
    e_blk = np.repeat(EFF, nblk)
    tol = 8 * np.finfo(float).eps
    scale_blk = np.abs(one[2]).max(1, keepdims=True)
    assert np.all(np.abs(e[2] - e_blk[:, None] * one[2]) <= tol * e_blk[:, None] * scale_blk)
    assert np.all(np.abs(e[3] - e_perf[:, None] * one[3]) <= tol * np.abs(one[3]).max())
    assert np.array_equal(e[4], one[4]) and np.array_equal(e[5], one[5]) and np.array_equal(e[6], one[6])     # flux_eq, ctrl_eq, perf_rates
    assert np.abs(one[0]).max() > 0 and np.abs(one[2]).max() > 0


def test_host_well_model_matches_the_reference_with_factors(oracle):
    """opmgpu/wells.py (hand-written derivatives, explicit Schur complement, ILU0 + BiCGStab on the oracle) with factors 0.8 / 0.5 against the
    reference subclass (complex-step Jacobian, one coupled system, direct solve): two Newton iterations of one step on the _setup() deck at
    the tolerances of tests/test_gpu_wells.py::test_well_coupled_newton_parity.  The unweighted model is far outside them."""
    grid, tab, st, wl = _setup()
    with_factors(wl, EFF)
    prm = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500)
    dt = 2 * decks.DAY
    ref = WefacOracleModel(grid, tab, prm, wl, arrays(seeded_state(wl, st.p)), EFF)
    ob = OracleBackend(oracle, grid, tab, prm, wells=wl.arrays())
    mh = W.WellCoupledModel(ob, W.StandardWellsHost(wl, grid.z, tab.surface_density[0]), seeded_state(wl, st.p))
    plain = _setup()[3]
    ob1 = OracleBackend(oracle, grid, tab, prm, wells=plain.arrays())
    m1 = W.WellCoupledModel(ob1, W.StandardWellsHost(plain, grid.z, tab.surface_density[0]), seeded_state(plain, st.p))
    ref.prepareStep(dt, st); mh.prepareStep(dt, st); m1.prepareStep(dt, st)
    for it in range(2):
        cr = ref.nonlinearIteration(it)
        ch, _ = mh.nonlinearIteration(it, single_precision=False)
        m1.nonlinearIteration(it, single_precision=False)
        assert cr == ch, it
        a, b = ob.getState(), ref.st
        assert np.array_equal(a.hc, b.hc), it
        assert np.abs(a.p - b.p).max() <= 1e-6 * np.abs(b.p).max(), it
        assert np.abs(a.sat - b.sat).max() <= 1e-6, it
        assert np.allclose(mh.ws.bhp, ref.ws.bhp, rtol=1e-7) and np.allclose(mh.ws.qs, ref.ws.qs, rtol=1e-6, atol=1e-9 * np.abs(ref.ws.qs).max()), it
        assert np.allclose(ob.CNV, ref.CNV, rtol=1e-5, atol=1e-9) and np.allclose(mh.wh.flux_eq, ref.E[:, :3], rtol=1e-5, atol=1e-12), it
    assert mh.ws.qs[0, 0] > 0 and mh.ws.qs[1, 1] < 0
    off = np.abs(ob1.getState().p - ref.st.p).max() / np.abs(ref.st.p).max()
    assert off > 1e-4, off                                  # the factors matter on this deck: 100 x the bound above


# ---------------------------------------------------------------------------------------------------------------------------------------
# SCHEDULE
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sched(path=DECK):
    d = deckmod.read_deck(path)
    g = d.grid()
    n = 90
    dx, dy, dz = d._cell_sizes()
    return schedule.Schedule(d, g, perm_md=(d.array("PERMX", n), d.array("PERMY", n)), dz=dz.ravel(), dxdy=(dx.ravel(), dy.ravel()), ntg=np.ones(n))


def test_wefac_per_report_step():
    s = _sched()
    assert len(s.steps) == 3
    got = []
    for step in range(3):
        wl = s.wells(step)
        assert wl.name == ["INJ", "PROD1"]
        got.append(wl.efficiency_factors().tolist())
    # 'INJ' 0.8 and the template 'PROD*' 0.5 before the first date; 'PROD1' 0.9 before the second, in force until the end
    assert got == [[0.8, 0.5], [0.8, 0.9], [0.8, 0.9]]


def _variant(tmp_path, old, new, name="V.DATA"):
    src = open(DECK).read()
    assert src.count(old) == 1
    path = tmp_path / name
    path.write_text(src.replace(old, new))
    return str(path)


@pytest.mark.parametrize("record, text", [(" 'PROD1' 0.0 /", "outside"), (" 'PROD1' 1.2 /", "outside"), (" 'PROD1' -0.9 /", "outside"),
                                          (" 'NOBODY' 0.9 /", "unknown well"), (" 'X*' 0.9 /", "unknown well")])
def test_wefac_refusals_name_the_keyword(tmp_path, record, text):
    with pytest.raises(ValueError, match="WEFAC.*" + text):
        _sched(_variant(tmp_path, " 'PROD1' 0.9 /", record))


def test_gefac_is_refused(tmp_path):
    with pytest.raises(ValueError, match="GEFAC"):
        _sched(_variant(tmp_path, "WEFAC\n 'PROD1' 0.9 /\n/\n", "GEFAC\n 'G' 0.9 /\n/\n"))


def test_deck_without_wefac_has_unit_factors(tmp_path):
    path = _variant(tmp_path, "WEFAC\n 'INJ'   0.8 /\n 'PROD*' 0.5 /\n/\n", "")
    s = _sched(path)
    assert s.wells(0).efficiency_factors().tolist() == [1.0, 1.0] and s.wells(1).efficiency_factors().tolist() == [1.0, 0.9]


def test_summary_field_rates_are_weighted(tmp_path):
    """OURS: FOPR FWPR FGPR FWIR FGIR sum e_w times the well rate, the W* vectors stay the wells' own (values are stored as float32)"""
    import datetime
    from opmgpu import eclio
    grid, tab, st, wl = _setup()
    with_factors(wl, EFF)
    ws = W.WellState(wl, st.p)
    ws.qs[0] = [0.02, 0.0, 0.0]; ws.qs[1] = [-0.001, -0.01, -0.5]
    out = eclio.EclOutput(str(tmp_path / "S"), (10, 10, 3), np.arange(300), datetime.date(2020, 1, 1))
    out.write_summary(1.0, wl, ws, new_report_step=True)
    kws, wgn = out._vectors
    params = np.asarray(next(v for k, _, v in eclio.read_arrays(str(tmp_path / "S.UNSMRY")) if k.strip() == "PARAMS"), float)
    row = {(k, g): v for k, g, v in zip(kws, wgn, params)}
    day = decks.DAY
    f32 = lambda x: float(np.float32(x))          # noqa: E731
    assert row[("WOPR", "PROD")] == f32(0.01 * day) and row[("WWIR", "INJ")] == f32(0.02 * day)
    assert row[("FOPR", ":+:+:+:+")] == f32(0.5 * 0.01 * day) and row[("FWPR", ":+:+:+:+")] == f32(0.5 * 0.001 * day)
    assert row[("FGPR", ":+:+:+:+")] == f32(0.5 * 0.5 * day) and row[("FWIR", ":+:+:+:+")] == f32(0.8 * 0.02 * day)
