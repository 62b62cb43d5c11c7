"""The cells of the rock-region tests: four rock regions -- tables of 2, 3 and 17 rows and one region in the ROCK form --, a shuffled
rocknum, and per branch of the rule (tests/rock_reference.py) at least eight cells, over the three-phase fluid of cell_edge_cases.py and
over the oil-water fluid of twophase.py (whose reference is that module's three-phase twin at Sg = 0, Sw >= Swco + 1e-3: the twin's water
and oil properties are the two-phase ones).

load(form) builds the cells, evaluates the 50-digit reference once per process and hands them out; census() counts the branches BY THE
REFERENCE'S RECORD -- not by what the input was meant to hit.  The cells are meant for OPMGPU_ROCK_IRREVERSIBLE; under REVERSIBLE every
cell is on its curve (reversible())."""
import numpy as np

import cell_edge_cases as E
import cell_reference as R
import rock_reference as K
import twophase as tp
from opmgpu import capi, decks

BAR = decks.BAR
GO, OO, GG = capi.HC_GAS_AND_OIL, capi.HC_OIL_ONLY, capi.HC_GAS_ONLY
INF = float("inf")
FORMS = ("wog", "wo")

# region 0: 2 rows; region 1: 3 rows; region 2: 17 rows, uneven spacing, a kink at every node; region 3: the ROCK form
_T2 = [(90.0, 0.93, 0.80), (410.0, 1.05, 1.12)]
_T3 = [(70.0, 0.95, 0.90), (180.0, 1.0, 1.0), (430.0, 1.04, 1.15)]
_T17 = [(60.0 + 21.0 * k + 3.0 * (k % 3), 0.90 + 0.008 * k + 0.002 * (k % 2) * k, 0.70 + 0.03 * k - 0.004 * (k % 4)) for k in range(17)]
ROCK = [(1.0, 0.0), (1.0, 0.0), (1.0, 0.0), (140.0, 6.0e-5)]
TABLES = [_T2, _T3, _T17, None]
NREG = 4
# an extra region nobody is in, with a table long enough to push the device's table blob past the 24 KiB that fit in LDS
_BIG = [(10.0 + 0.5 * k, 0.9 + 1e-4 * k, 0.8 + 2e-4 * k) for k in range(800)]


def regions(rocknum, irreversible=True, big=False):
    return decks.RockRegions(rocknum, ROCK + ([(1.0, 0.0)] if big else []), TABLES + ([_BIG] if big else []), irreversible=irreversible)


class CaseSet:
    """the cells of one fluid form: state, fluid regions, rock regions, history, tags, reference"""

    def __init__(self, form):
        self.form = form
        self.tab = E.tables("base") if form == "wog" else tp.tables(2)
        self.ref_tab = self.tab if form == "wog" else tp.twin_tables(2)
        self.rows, self.cat = [], []

    def add(self, cat, r, p, p_min, k):
        """cell number k of a category: the fluid state cycles through the hydrocarbon states and the fluid regions"""
        preg, sreg = k % 2, (k // 2) % 2
        if self.form == "wo":
            swco = float(R.Tables(self.ref_tab).sat(sreg)["sw"][0])
            self.rows.append((preg, sreg, p, max(E.SW0 + 0.07 * (k % 5), swco + 0.05), 0.0, 0.0, 0.0, GO, p_min, r))
        else:
            hc = (GO, OO, GG)[k % 3]
            self.rows.append((preg, sreg, p, E.SW0 - 0.02 * (k % 4), E.SG0 + 0.03 * (k % 3), E.RS0 - 4.0 * (k % 2), E.RV0, hc, p_min, r))
        self.cat.append(cat)

    def finish(self, seed=5):
        order = np.random.default_rng(seed).permutation(len(self.rows))         # rocknum (and everything else) shuffled
        a = np.array(self.rows)[order]
        self.cat = np.array(self.cat)[order]
        self.nc = a.shape[0]
        self.pvtnum, self.satnum = a[:, 0].astype(np.int32), a[:, 1].astype(np.int32)
        hc, sw = a[:, 7].astype(np.int8), a[:, 3]
        sg = np.where(hc == GO, a[:, 4], np.where(hc == GG, 1.0 - sw, 0.0))
        self.state = decks.State(a[:, 2].copy(), np.stack([sw, (1.0 - sw) - sg, sg], 1), a[:, 5].copy(), a[:, 6].copy(), hc)
        self.p_min, self.rocknum = a[:, 8].copy(), a[:, 9].astype(np.int32)
        self.regions = regions(self.rocknum)
        self.ref, self.rock_recs = K.cells(self.ref_tab, self.regions, self.rocknum, self.pvtnum, self.satnum, self.state, self.p_min)
        self.recs = [b["fluid"] for b in self.rock_recs]          # (what cell_edge_cases.hc_groups groups by)
        return self

    def grid(self, seed=3):
        """the cells as a grid WITHOUT connections (pore volumes varied)"""
        rng = np.random.default_rng(seed)
        return decks.GridData(self.nc, np.zeros((0, 2), np.int32), np.zeros(0), rng.uniform(20.0, 80.0, self.nc), np.full(self.nc, 2000.0),
                              pvtnum=self.pvtnum, satnum=self.satnum)

    def shifted(self):
        """a second arrangement of the same cells: cell i takes the state, the rock region and the history of cell perm[i] of its
        (preg, sreg, hc) group, so that the reference of the new arrangement is a permutation of the old one's"""
        perm = np.arange(self.nc)
        key = self.pvtnum * 100 + self.satnum * 10 + self.state.hc
        for k in np.unique(key):
            i = np.flatnonzero(key == k)
            perm[i] = np.roll(i, -1)
        s = self.state
        return decks.State(s.p[perm], s.sat[perm], s.rs[perm], s.rv[perm], s.hc[perm]), self.rocknum[perm], self.p_min[perm], perm


def _build(C):
    tabs = [(r, np.array(t)[:, 0] * BAR) for r, t in enumerate(TABLES) if t is not None]
    k = 0
    for r, x in tabs:
        inside = [0.5 * (x[0] + x[1]) + 1.3 * BAR, x[-1] - 0.31 * (x[-1] - x[-2]), x[0] + 0.77 * (x[1] - x[0])]
        for v in inside:
            C.add("on_curve_inside", r, v, v + 11.0 * BAR, k); k += 1
            C.add("tie", r, v, v, k); k += 1
            C.add("just_above", r, float(np.nextafter(v, np.inf)), v, k); k += 1
            C.add("fresh", r, v, INF, k); k += 1
            C.add("off_curve_inside", r, v + 23.0 * BAR, v, k); k += 1
        for d in (5.0, 31.0, 50.0):
            C.add("below_first", r, x[0] - d * BAR, x[0] + 3.0 * BAR, k); k += 1                        # on the curve
            C.add("below_first", r, x[0] + 20.0 * BAR, x[0] - d * BAR, k); k += 1                       # off it: x = p_min
            C.add("above_last", r, x[-1] + d * BAR, INF, k); k += 1
            C.add("above_last", r, x[-1] + (d + 9.0) * BAR, x[-1] + d * BAR, k); k += 1
        C.add("first_node", r, x[0], INF, k); k += 1
        C.add("last_node", r, x[-1], x[-1], k); k += 1
    for r, x in tabs:
        for node in x[1:-1]:
            for v in E.around(node):
                C.add("interior_node", r, v, INF, k); k += 1                                           # p on (next to) the node
            C.add("interior_node", r, node + 7.0 * BAR, node, k); k += 1                                # p_min on it
    for j in range(10):
        p0 = (95.0 + 27.0 * j) * BAR
        C.add("rock_form", 3, p0, (p0 - 12.0 * BAR, p0 + 12.0 * BAR, p0, INF)[j % 4], k); k += 1


# branch -> what the rock record of the reference must show (at least MIN_CELLS cells each)
MIN_CELLS = 8
CENSUS = {
    "on the curve, inside the table": lambda b: b["form"] == "table" and b["on_curve"] and not b["tie"] and not b["fresh"] and b["search"].side == 0,
    "p == p_min": lambda b: b["form"] == "table" and b["tie"] and b["on_curve"],
    "p == nextafter(p_min, +inf)": lambda b: b["form"] == "table" and not b["on_curve"] and b["just_above"],
    "p_min == +inf": lambda b: b["form"] == "table" and b["fresh"] and b["on_curve"],
    "off the curve": lambda b: b["form"] == "table" and not b["on_curve"],
    "x below the first node": lambda b: b["form"] == "table" and b["search"].side < 0,
    "x below the first node, off the curve": lambda b: b["form"] == "table" and b["search"].side < 0 and not b["on_curve"],
    "x above the last node": lambda b: b["form"] == "table" and b["search"].side > 0,
    "x above the last node, off the curve": lambda b: b["form"] == "table" and b["search"].side > 0 and not b["on_curve"],
    "x on an interior node": lambda b: b["form"] == "table" and 0 < b["search"].at < b["search"].n - 1,
    "x on an interior node, off the curve": lambda b: b["form"] == "table" and 0 < b["search"].at < b["search"].n - 1 and not b["on_curve"],
    "ROCK form under IRREVERSIBLE": lambda b: b["form"] == "rock",
}


def census(C):
    """{branch: number of cells} by the reference's records; plus the regions and table lengths in use"""
    recs = []
    for c, b in enumerate(C.rock_recs):
        b = dict(b)
        b["just_above"] = C.state.p[c] == np.nextafter(C.p_min[c], np.inf)
        recs.append(b)
    out = {name: sum(1 for b in recs if pred(b)) for name, pred in CENSUS.items()}
    out["table lengths"] = sorted({b["search"].n for b in recs if b["form"] == "table"})
    out["interior nodes hit"] = {r: sorted({b["search"].at for b in recs if b["form"] == "table" and b["region"] == r and 0 < b["search"].at < b["search"].n - 1})
                                 for r in (1, 2)}
    return out


_loaded = {}


def load(form="wog"):
    if form not in _loaded:
        C = CaseSet(form)
        _build(C)
        _loaded[form] = C.finish()
    return _loaded[form]


def reversible(C):
    """the reference of the same cells under OPMGPU_ROCK_REVERSIBLE: (ref[nc][26][4], rock records)"""
    if not hasattr(C, "_rev"):
        C._rev = K.cells(C.ref_tab, regions(C.rocknum, irreversible=False), C.rocknum, C.pvtnum, C.satnum, C.state, C.p_min)
    return C._rev
