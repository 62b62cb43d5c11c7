"""CPU: the SCHEDULE reader's group keywords (GRUPTREE, GCONPROD, GCONINJE, WGRUPCON, WELSPECS item 2; opmgpu/schedule.py) on the hand-written
deck tests/golden/decks/GROUP_SMALL.DATA -- the tree, the members' slots, the initial current controls, every refusal with its message --
and the deck through the report-step driver with the host well model on the CPU oracle."""
import os

import numpy as np
import pytest

from opmgpu import capi, deck as deckmod, decks, schedule, wells as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = os.path.join(ROOT, "tests", "golden", "decks", "GROUP_SMALL.DATA")
DAY = decks.DAY


def _sched(path=DECK):
    d = deckmod.read_deck(path)
    g = d.grid()
    n = 108
    dx, dy, dz = d._cell_sizes()
    return schedule.Schedule(d, g, perm_md=(d.array("PERMX", n), d.array("PERMY", n)), dz=dz.ravel(), dxdy=(dx.ravel(), dy.ravel()), ntg=np.ones(n))


def _variant(tmp_path, old, new, name="V.DATA"):
    src = open(DECK).read()
    assert src.count(old) == 1, old
    path = tmp_path / name
    path.write_text(src.replace(old, new))
    return str(path)


def test_tree_slots_and_current_controls():
    s = _sched()
    assert len(s.steps) == 3 and len(s.groups) == 3
    for step in range(3):
        assert s.group_tree(step) == {"PROD": "FIELD", "INJ": "FIELD"}
        assert s.controlling_group(step, "PROD", "PROD") == ("FIELD", -1.0, 300.0 / DAY, (0.0, 1.0, 0.0))
        assert s.controlling_group(step, "INJ", "WATER") is None and s.controlling_group(step, "PROD", "GAS") is None
        wl = s.wells(step)
        assert wl.name == ["P1", "P2", "P3", "I1"]
        assert [s.steps[step][1][n].group for n in wl.name] == ["PROD", "PROD", "PROD", "INJ"]          # WELSPECS item 2 is kept
        (g,) = wl.groups
        assert (g.name, g.sign, g.target, g.wells) == ("FIELD", -1.0, 300.0 / DAY, [0, 1, 2]) and g.distr.tolist() == [0.0, 1.0, 0.0]
        assert g.guide[:2] == [0.002, 0.004] and np.isnan(g.guide[2])                                   # P3: from the potentials
        # the slot is the LAST control of every member: P1 (GRUP) has its BHP limit and the slot, P2 / P3 their ORAT, the BHP limit, the slot
        assert [[c[0] for c in cl] for cl in wl.controls] == [[W.BHP, W.SURFACE_RATE], [W.SURFACE_RATE, W.BHP, W.SURFACE_RATE],
                                                              [W.SURFACE_RATE, W.BHP, W.SURFACE_RATE], [W.SURFACE_RATE, W.BHP]]
        for w in range(3):
            typ, target, distr = wl.controls[w][-1][:3]
            assert typ == W.SURFACE_RATE and distr.tolist() == [0.0, 1.0, 0.0] and target == -300.0 / DAY
        assert wl.controls[1][0][1] == -80.0 / DAY and wl.controls[2][0][1] == -90.0 / DAY
        # P1's deck mode is GRUP: it starts on its slot; the others start on their own mode with the slot as a constraint
        assert wl.current0 == [1, 0, 0, 0]
        ws = W.WellState(wl, np.full(108, 250 * decks.BAR))
        assert ws.current.tolist() == [1, 0, 0, 0]


def test_groups_follow_the_report_steps(tmp_path):
    """a GCONPROD between two report steps holds from there on; mode NONE switches the target off again"""
    s = _sched(_variant(tmp_path, "TSTEP\n 10 10 20 /", "TSTEP\n 10 /\nGCONPROD\n 'FIELD' 'NONE' /\n 'PROD' 'LRAT' 3* 250 /\n/\nWCONPROD\n 'P1' 'OPEN' 'GRUP' 5* 150 /\n/\nTSTEP\n 10 20 /"))
    assert [g.name for g in s.wells(0).groups] == ["FIELD"]
    for step in (1, 2):
        (g,) = s.wells(step).groups
        assert (g.name, g.target, g.distr.tolist()) == ("PROD", 250.0 / DAY, [1.0, 1.0, 0.0])


def test_injection_group_and_unavailable_well(tmp_path):
    s = _sched(_variant(tmp_path, " 'P3' 'YES' 1* /", " 'P3' 'NO' /\n/\nGCONINJE\n 'FIELD' 'WATER' 'RATE' 350 /"))
    wl = s.wells(0)
    prod, inj = wl.groups
    assert (prod.name, prod.wells) == ("FIELD", [0, 1]) and len(wl.controls[2]) == 2                    # P3: no member, no slot
    assert (inj.name, inj.sign, inj.target, inj.wells) == ("FIELD", 1.0, 350.0 / DAY, [3]) and inj.distr.tolist() == [1.0, 0.0, 0.0]
    assert wl.controls[3][-1][0] == W.SURFACE_RATE and wl.current0 == [1, 0, 0, 0]


REFUSALS = [
    # GCONPROD modes
    ("'FIELD' 'ORAT' 300 /", "'FIELD' 'RESV' 300 /", "GCONPROD FIELD: item 2, control mode RESV"),
    ("'FIELD' 'ORAT' 300 /", "'FIELD' 'CRAT' 300 /", "GCONPROD FIELD: item 2, control mode CRAT"),
    ("'FIELD' 'ORAT' 300 /", "'FIELD' 'PRBL' 300 /", "GCONPROD FIELD: item 2, control mode PRBL"),
    # a rate limit other than the mode's own target
    ("'FIELD' 'ORAT' 300 /", "'FIELD' 'ORAT' 300 500 /", "GCONPROD FIELD: item 4, a WRAT limit next to control mode ORAT"),
    ("'FIELD' 'ORAT' 300 /", "'FIELD' 'ORAT' 300 2* 700 /", "GCONPROD FIELD: item 6, a LRAT limit next to control mode ORAT"),
    ("'FIELD' 'ORAT' 300 /", "'FIELD' 'ORAT' 300 10* 900 /", "GCONPROD FIELD: item 14, a RESV limit next to control mode ORAT"),
    ("'FIELD' 'ORAT' 300 /", "'FIELD' 'LRAT' 300 /", "GCONPROD FIELD: item 3, a ORAT limit next to control mode LRAT"),
    ("'FIELD' 'ORAT' 300 /", "'FIELD' 'ORAT' /", "GCONPROD FIELD: item 3, the ORAT target, is missing"),
    # exceed action
    ("'FIELD' 'ORAT' 300 /", "'FIELD' 'ORAT' 300 3* 'WELL' /", "GCONPROD FIELD: item 7, exceed action WELL"),
    # GCONINJE modes
    ("WGRUPCON\n", "GCONINJE\n 'INJ' 'WATER' 'RESV' 1* 300 /\n/\nWGRUPCON\n", "GCONINJE INJ: item 3, control mode RESV"),
    ("WGRUPCON\n", "GCONINJE\n 'INJ' 'WATER' 'REIN' 2* 1.0 /\n/\nWGRUPCON\n", "GCONINJE INJ: item 3, control mode REIN"),
    ("WGRUPCON\n", "GCONINJE\n 'INJ' 'WATER' 'VREP' 3* 1.0 /\n/\nWGRUPCON\n", "GCONINJE INJ: item 3, control mode VREP"),
    ("WGRUPCON\n", "GCONINJE\n 'INJ' 'OIL' 'RATE' 300 /\n/\nWGRUPCON\n", "GCONINJE INJ: item 2, phase 'OIL'"),
    # GEFAC stays refused
    ("WGRUPCON\n", "GEFAC\n 'PROD' 0.9 /\n/\nWGRUPCON\n", "GEFAC"),
]


@pytest.mark.parametrize("old, new, text", REFUSALS)
def test_refusals_name_keyword_and_item(tmp_path, old, new, text):
    import re
    with pytest.raises(ValueError, match=re.escape(text)):
        _sched(_variant(tmp_path, old, new))


def test_two_ancestors_with_a_target_are_refused(tmp_path):
    s = _sched(_variant(tmp_path, "'FIELD' 'ORAT' 300 /", "'FIELD' 'ORAT' 300 /\n 'PROD' 'ORAT' 200 /"))
    with pytest.raises(ValueError, match="GCONPROD: groups PROD and FIELD, one above the other, both have an active target"):
        s.wells(0)


def test_grup_without_a_controlling_group_is_refused(tmp_path):
    s = _sched(_variant(tmp_path, "GCONPROD\n 'FIELD' 'ORAT' 300 /\n/\n", ""))
    with pytest.raises(ValueError, match="WCONPROD P1: item 3, control mode GRUP, but the well has no controlling group"):
        s.wells(0)
    s = _sched(_variant(tmp_path, "'I1' 'WATER' 'OPEN' 'RATE' 400 1* 320 /", "'I1' 'WATER' 'OPEN' 'GRUP' 400 1* 320 /"))
    with pytest.raises(ValueError, match="WCONINJE I1: item 4, control mode GRUP, but the well has no controlling group"):
        s.wells(0)
    s = _sched(_variant(tmp_path, "'P1' 'YES' 0.002 /", "'P1' 'NO' /"))
    with pytest.raises(ValueError, match="WCONPROD P1: item 3, control mode GRUP.*WGRUPCON makes it unavailable"):
        s.wells(0)


def test_gas_groups_in_a_deck_without_gas_are_refused(tmp_path):
    src = open(os.path.join(ROOT, "tests", "golden", "decks", "OILWATER_SMALL.DATA")).read()
    assert "\nWELSPECS\n" in src and "\nGAS\n" not in src.split("GRID")[0]
    for block, text in (("GCONPROD\n 'FIELD' 'GRAT' 2* 1000 /\n/\n", "GCONPROD FIELD: item 2, GRAT, in a deck without GAS"),
                        ("GCONINJE\n 'FIELD' 'GAS' 'RATE' 1000 /\n/\n", "GCONINJE FIELD: item 2, GAS, in a deck without GAS")):
        path = tmp_path / "OW.DATA"
        path.write_text(src.replace("\nWELSPECS\n", "\n" + block + "WELSPECS\n", 1))
        d = deckmod.read_deck(str(path))
        nx, ny, nz = d.dims
        n = nx * ny * nz
        dx, dy, dz = d._cell_sizes()
        with pytest.raises(ValueError, match=text):
            schedule.Schedule(d, d.grid(), perm_md=(d.array("PERMX", n), d.array("PERMY", n, d.array("PERMX", n))), dz=dz.ravel(), dxdy=(dx.ravel(), dy.ravel()), ntg=np.ones(n))


def _summary(base):
    from opmgpu import eclio
    kws = wgn = None
    for k, _, v in eclio.read_arrays(base + ".SMSPEC"):
        if k.strip() == "KEYWORDS":
            kws = [str(x).strip() for x in v]
        if k.strip() == "WGNAMES":
            wgn = [str(x).strip() for x in v]
    rows = [np.asarray(v, float) for k, _, v in eclio.read_arrays(base + ".UNSMRY") if k.strip() == "PARAMS"]
    return [{(k, g): x for k, g, x in zip(kws, wgn, row)} for row in rows]


def host_run(oracle, deck, base, max_steps=None):
    """the deck through the report-step driver with the CPU oracle and the host well model; returns (reports, summary rows, last well state's
    current controls at the end of every report step)"""
    from opmgpu.simulator import Simulator
    from util import OracleBackend

    def oracle_model(grid, tables, params):
        return OracleBackend(oracle, grid, tables, params)

    currents = []

    def host_wells(model, wl, ws):
        if model.wells is None or list(model.wells[1]) != list(wl.arrays()[1]):
            model.wells = wl.arrays()
            model.rowptr, model.col = oracle.pattern(model.grid, *model.wells)
        currents.append(ws.current)               # (the array the model updates in place)
        return W.WellCoupledModel(model, W.StandardWellsHost(wl, model.grid.z, model.tab.surface_density[0], tolerance_wells=1e-7), ws)

    tight = dict(tolerance_mb=1e-9, tolerance_cnv=1e-5, tolerance_wells=1e-7, linear_solver_reduction=1e-9, linear_solver_maxiter=400)
    sim = Simulator(deck, params=capi.default_params(**tight), output_base=base, model_factory=oracle_model, well_model_factory=host_wells)
    reps = sim.run(max_steps)
    return reps, _summary(base), [c.tolist() for c in currents]


F = ":+:+:+:+"
# the summary file holds float32: the field rate is the sum of three wells' rates, each within tolerance_well_control (1e-7 m3/s = 0.00864
# m3/day) of its target, rounded once to float32 (2^-24 * 300 = 1.8e-5)
FOPR_TOL = 3 * 1e-7 * DAY + 2.0 ** -23 * 300.0


def test_golden_deck_with_the_host_well_model(oracle, tmp_path):
    reps, rows, currents = host_run(oracle, DECK, str(tmp_path / "HOST"))
    assert [r["days"] for r in reps] == [10.0, 20.0, 40.0] and len(rows) == 3
    for row in rows:
        assert abs(row[("FOPR", F)] - 300.0) <= FOPR_TOL, row[("FOPR", F)]
        assert abs(row[("WOPR", "P2")] - 80.0) <= FOPR_TOL and abs(row[("WOPR", "P3")] - 90.0) <= FOPR_TOL      # on their own rates ...
        assert abs(row[("WOPR", "P1")] - 130.0) <= FOPR_TOL                                                     # ... P1 takes what is left
    assert all(c[0] == 1 for c in currents)                                # the GRUP well stays on its slot


def test_variant_without_grup_is_capped_too(oracle, tmp_path):
    """P1 on its own oil rate of 200 sm3/day: 370 sm3/day with the others, which the reader used to let through (GCONPROD was skipped
    without a word).  The slot is a constraint of P1 now: its rate breaks it, P1 goes under group control and the field makes 300."""
    path = _variant(tmp_path, "'P1' 'OPEN' 'GRUP' 5* 150 /", "'P1' 'OPEN' 'ORAT' 200 4* 150 /")
    assert _sched(path).wells(0).current0 == [0, 0, 0, 0]
    reps, rows, currents = host_run(oracle, path, str(tmp_path / "VAR"))
    for row in rows:
        assert abs(row[("FOPR", F)] - 300.0) <= FOPR_TOL, row[("FOPR", F)]
        assert abs(row[("WOPR", "P1")] - 130.0) <= FOPR_TOL
    assert all(c[0] == 2 for c in currents)                                # at the end of every report step P1 is on the slot (its last control)
