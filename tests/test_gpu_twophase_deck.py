"""GPU: the golden oil-water deck (tests/golden/decks/OILWATER_SMALL.DATA) end to end through the report-step driver, in the manner of
test_gpu_simulator.py, and diffed against the same run of its three-phase twin deck with the regression tolerances."""
import numpy as np
import pytest

from opmgpu import capi, decks, eclio
from opmgpu.simulator import Simulator

import twophase as tp

pytestmark = pytest.mark.gpu


def test_two_phase_deck_runs_and_matches_its_twin(gpu_lib, oracle, tmp_path):
    tight = dict(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, tolerance_mb=1e-9, tolerance_cnv=1e-5, tolerance_wells=1e-8, linear_solver_reduction=1e-9,
                 linear_solver_maxiter=400)
    base2, base3 = str(tmp_path / "OW"), str(tmp_path / "TWIN")
    sim = Simulator(tp.DECK, params=capi.default_params(**tight), output_base=base2)
    sim.model.max_single_precision_days = 0.0
    assert sim.tables.phases == "wo"
    names = oracle.PROP_NAMES
    sim3 = Simulator(tp.write_deck(tmp_path / "TWIN.DATA", tp.twin_deck_text()), params=capi.default_params(**tight), output_base=base3)
    sim3.model.max_single_precision_days = 0.0

    def in_place(state):          # water and oil in place, evaluated by the oracle on the twin's tables
        props = oracle.cell_props(sim3.grid, sim3.tables, state)
        return np.array([(props[:, names.index("accum_" + c), 0] * sim3.grid.pv).sum() for c in "wo"])
    v0 = in_place(sim.model.getState())
    reps = sim.run()
    assert [r["days"] for r in reps] == [10.0, 20.0, 40.0] and all(r["substeps"] >= 1 and r["failed"] == 0 for r in reps)
    final = sim.model.getState()
    assert np.all(final.sat[:, 2] == 0.0) and np.all(final.rs == 0.0) and np.all(final.rv == 0.0) and np.all(final.hc == capi.HC_GAS_AND_OIL)
    # fluid in place of every report step: no gas of any kind
    for r in reps:
        assert np.all(r["fip"][:, 2:5] == 0.0) and np.all(r["fip"][:, :2] > 0.0)
    # restart file: phase indicator 3, no gas arrays (the deck's RPTRST asks for BG KRG RSSAT PBPD: skipped), the last section = the state
    rst = eclio.read_arrays(base2 + ".UNRST")
    kws = [a[0] for a in rst]
    assert [a[2][0] for a in rst if a[0] == "SEQNUM"] == [1, 2, 3, 4]
    assert all(a[2][14] == 3 for a in rst if a[0] == "INTEHEAD")
    for gone in ("SGAS", "RS", "RV", "1OVERBG", "GAS_DEN", "GAS_VISC", "GASKR", "RSSAT", "PBUB", "PDEW"):
        assert gone not in kws, gone
    for there in ("1OVERBO", "WAT_DEN", "OIL_DEN", "WAT_VISC", "OIL_VISC", "OILKR"):
        assert kws.count(there) == 3, there
    assert np.allclose([a[2] for a in rst if a[0] == "PRESSURE"][-1], final.p / decks.BAR, rtol=1e-6)
    assert np.allclose([a[2] for a in rst if a[0] == "SWAT"][-1], final.sat[:, 0], atol=1e-6)
    # summary: the injector under its limits, the producer on its BHP, no gas rate anywhere
    sp = {a[0]: a[2] for a in eclio.read_arrays(base2 + ".SMSPEC")}
    kw, wg = list(sp["KEYWORDS"]), list(sp["WGNAMES"])
    idx = lambda k, g: next(i for i, (a, b) in enumerate(zip(kw, wg)) if a == k and b == g)      # noqa: E731
    rows = [a[2] for a in eclio.read_arrays(base2 + ".UNSMRY") if a[0] == "PARAMS"]
    assert len(rows) == 3
    for r in rows:
        assert r[idx("WBHP", "INJ")] <= 400.0 * (1 + 1e-6) and r[idx("WWIR", "INJ")] <= 300.0 * (1 + 1e-6)
        assert r[idx("WBHP", "PROD")] == pytest.approx(235.0, rel=1e-5) and r[idx("WOPR", "PROD")] > 0.0
        assert r[idx("FGPR", ":+:+:+:+")] == 0.0 and r[idx("FGIR", ":+:+:+:+")] == 0.0 and r[idx("FGIP", ":+:+:+:+")] == 0.0
    # material balance of water and oil, as test_gpu_simulator.py bounds it: water came in, oil went out
    dv = in_place(final) - v0
    assert dv[0] > 0 and dv[1] < 0 and sum(r[idx("FWIR", ":+:+:+:+")] for r in rows) > 0
    sim.close()
    # the same run of the twin deck (three phases, dummy gas): PRESSURE and SWAT within compare's defaults
    reps3 = sim3.run()
    sim3.close()
    assert [r["days"] for r in reps3] == [10.0, 20.0, 40.0]
    assert eclio.compare(base2, base3, restart_keywords=("PRESSURE", "SWAT"), summary=False) == []
    rst3 = eclio.read_arrays(base3 + ".UNRST")
    assert np.all(np.concatenate([a[2] for a in rst3 if a[0] == "SGAS"]) == 0.0)


def test_two_phase_run_restarts_from_its_own_file(gpu_lib, tmp_path):
    """the restart file of a deck without a gas phase holds no SGAS / RS / RV: a run restarted from it continues the full one"""
    prm = dict(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, linear_solver_reduction=1e-8, linear_solver_maxiter=400)
    full, part = str(tmp_path / "FULL"), str(tmp_path / "PART")
    sim = Simulator(tp.DECK, params=capi.default_params(**prm), output_base=full)
    sim.run()
    sim.close()
    sim = Simulator(tp.DECK, params=capi.default_params(**prm), output_base=part, restart=(full, 3))
    assert np.all(sim.state0.sat[:, 2] == 0.0) and np.all(sim.state0.hc == capi.HC_GAS_AND_OIL)
    sim.run()
    sim.close()
    # tests/run-restart-regressionTest.sh's tolerances (abs 2e-1, rel 4e-5), as test_gpu_simulator.py's restart test uses them
    assert eclio.compare(full, part, abs_tol=2e-1, rel_tol=4e-5, restart_keywords=("PRESSURE", "SWAT"), by_seqnum=True, summary=False) == []
