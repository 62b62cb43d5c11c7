"""The cells at which a table evaluator goes wrong: every node of every table a cell searches, the floats next to it on both sides, the
table ends, the switches of the three-phase kro blend, VAPPARS and ROCKTAB -- a deterministic list of a few hundred cells, each tagged
with its category, over tables rich enough for every rule to matter (PVT nodes with 4- and 5-point columns at different pressures, two PVT
and two saturation regions with different tables so that every table offset is non-zero somewhere).

Saturation region 0 is the standard SWOF / SGOF; region 1 has zero capillary pressure (p_g == p exactly, so p_g can sit ON a gas node)
and Swco = 0, which makes Sg + Sw' - Swco exact: only there can the blend argument be exactly eps / 2 or eps (with Swco = 0.1 the
argument moves in steps of 1.4e-17 and the cells take the nearest float on each side instead).

load() builds the cells, evaluates the 50-digit reference (cell_reference.py) once per process and ASSERTS the census: every category is
present in both regions BY THE REFERENCE'S BRANCH RECORD -- not by what the input was meant to hit.
"""
import numpy as np

import cell_reference as R
from opmgpu import capi, decks

BAR = decks.BAR
GO, OO, GG = capi.HC_GAS_AND_OIL, capi.HC_OIL_ONLY, capi.HC_GAS_ONLY
P0, SW0, SG0, RS0, RV0 = 155.3 * BAR, 0.37, 0.13, 47.3, 0.4e-4          # a bland interior point: on no node of any table
EPS = R.EPS_BLEND

_PVTO = [(10, [(50, 1.05, 1.10), (120, 1.045, 1.13), (200, 1.040, 1.17), (320, 1.033, 1.24)]),
         (30, [(90, 1.09, 1.00)]),                                       # extended from the next node's column: 5 points
         (55, [(140, 1.15, 0.90), (190, 1.143, 0.93), (260, 1.135, 0.97), (350, 1.127, 1.02), (420, 1.12, 1.06)]),
         (80, [(185, 1.21, 0.82), (240, 1.203, 0.85), (300, 1.196, 0.88), (390, 1.187, 0.93)]),
         (110, [(235, 1.28, 0.75), (330, 1.268, 0.79)]),
         (150, [(300, 1.37, 0.68), (360, 1.361, 0.70), (450, 1.349, 0.74)])]
_PVTG = [(60, [(0.00012, 0.0200, 0.0140), (0.00006, 0.0203, 0.0138), (0.0, 0.0206, 0.0136)]),
         (110, [(0.00020, 0.0108, 0.0160), (0.00012, 0.0110, 0.0157), (0.00005, 0.0112, 0.0155), (0.0, 0.0113, 0.0153)]),
         (170, [(0.00031, 0.0070, 0.0185), (0.00015, 0.0072, 0.0180), (0.0, 0.0074, 0.0176)]),
         (250, [(0.00045, 0.0048, 0.0220), (0.0003, 0.0049, 0.0214), (0.00015, 0.0050, 0.0209), (0.0, 0.0051, 0.0205)]),
         (380, [(0.00062, 0.0033, 0.0275), (0.0003, 0.0034, 0.0262), (0.0, 0.0035, 0.0252)])]
# the standard tables (satfuncStandard.DATA, as decks.satfunc_standard_tables has them) and a zero-pc pair with Swco = 0
_SWOF = [[(0.1, 0.0, 1.0, 0.9), (0.2, 0.0, 0.8, 0.8), (0.3, 0.1, 0.6, 0.7), (0.4, 0.2, 0.4, 0.6), (0.7, 0.5, 0.1, 0.3), (0.8, 0.6, 0.0, 0.2),
          (0.9, 0.7, 0.0, 0.1)],
         [(0.0, 0.0, 1.0, 0.0), (0.15, 0.0, 0.85, 0.0), (0.3, 0.05, 0.6, 0.0), (0.5, 0.2, 0.3, 0.0), (0.75, 0.55, 0.05, 0.0), (1.0, 1.0, 0.0, 0.0)]]
_SGOF = [[(0.0, 0.0, 1.0, 0.2), (0.1, 0.0, 0.7, 0.4), (0.2, 0.1, 0.6, 0.6), (0.8, 0.7, 0.0, 2.0), (0.9, 1.0, 0.0, 2.1)],
         [(0.0, 0.0, 1.0, 0.0), (0.05, 0.0, 0.9, 0.0), (0.25, 0.1, 0.55, 0.0), (0.5, 0.35, 0.2, 0.0), (0.8, 0.8, 0.0, 0.0), (0.9, 1.0, 0.0, 0.0)]]
_ROCKTAB = [(80.0, 0.97, 0.94), (160.0, 1.0, 1.0), (260.0, 1.03, 1.07), (420.0, 1.06, 1.13)]
TSETS = ("base", "vap", "rock")


def tables(tset="base", copies=1):
    """the table set `tset`; copies > 1: the two regions of each kind repeated (region r + 2 j == region r), a larger device blob"""
    # PVT region 1: region 0's shape with other numbers and one node fewer (a different offset for everything behind it)
    pvto1 = [(0.9 * rs + 2, [(1.07 * p + 3, 1.02 * B, 0.95 * mu) for p, B, mu in col]) for rs, col in _PVTO[:-1]]
    pvtg1 = [(1.05 * pg + 4, [(0.9 * rv, 1.03 * B, 0.97 * mu) for rv, B, mu in col]) for pg, col in _PVTG]
    extra = {"vap": dict(vappars=(0.7, 1.3)), "rock": dict(rocktab=_ROCKTAB), "base": {}}[tset]
    return decks.FluidTables(density_wog=[[1000.0, 700.0, 1.0], [1020.0, 740.0, 0.9]] * copies,
                             pvtw=[[100.0, 1.02, 4.0e-5, 0.45, 2.0e-5], [150.0, 1.01, 4.5e-5, 0.5, 1.5e-5]] * copies,
                             pvto=[_PVTO, pvto1] * copies, pvtg=[_PVTG, pvtg1] * copies, swof=_SWOF * copies, sgof=_SGOF * copies,
                             rock=(100.0, 5.0e-5), **extra)


def around(v):
    return [float(np.nextafter(v, -np.inf)), float(v), float(np.nextafter(v, np.inf))]


def bracket(fn, x0, target, scale=0.0):
    """the floats x next to x0 at which fn(x) is the largest value < target, the largest <= target (== target where it can be reached)
    and the smallest > target.  scale: the size of the largest intermediate of fn (its spacing is the step in which fn moves)"""
    step = np.spacing(max(abs(x0), scale)) / 2
    c = sorted({(fn(x), x) for x in (float(x0 + k * step) for k in range(-256, 257))})
    lt = [x for f, x in c if f < target][-1]
    le = [x for f, x in c if f <= target][-1]
    gt = [x for f, x in c if f > target][0]
    return [lt, le, gt]


class CaseSet:
    """the cells of one table set: state arrays, regions, soMax, tags"""

    def __init__(self, tset):
        self.tset, self.tab = tset, tables(tset)
        self.rows, self.cat, self.region = [], [], []

    def add(self, cat, region, preg, sreg, p=P0, sw=SW0, sg=SG0, rs=RS0, rv=RV0, hc=GO, so_max=0.0):
        self.rows.append((preg, sreg, float(p), float(sw), float(sg), float(rs), float(rv), hc, float(so_max)))
        self.cat.append(cat); self.region.append(region)

    def finish(self):
        a = np.array(self.rows)
        self.nc = a.shape[0]
        self.pvtnum, self.satnum = a[:, 0].astype(np.int32), a[:, 1].astype(np.int32)
        hc = a[:, 7].astype(np.int8)
        sw = a[:, 3]
        sg = np.where(hc == GO, a[:, 4], np.where(hc == GG, 1.0 - sw, 0.0))
        self.state = decks.State(a[:, 2], np.stack([sw, (1.0 - sw) - sg, sg], 1), a[:, 5], a[:, 6], hc)
        self.so_max = a[:, 8].copy()
        self.cat, self.region = np.array(self.cat), np.array(self.region)
        self.ref, self.recs = R.cells(self.tab, self.pvtnum, self.satnum, self.state, self.so_max)
        return self

    def grid(self, copies=1, seed=3):
        """the cells as a grid WITHOUT connections (pore volumes varied); copies > 1 spreads the cells over the repeated regions of
        tables(tset, copies)"""
        rng = np.random.default_rng(seed)
        j = rng.integers(0, copies, (2, self.nc)) if copies > 1 else np.zeros((2, self.nc), int)
        return decks.GridData(self.nc, np.zeros((0, 2), np.int32), np.zeros(0), rng.uniform(20.0, 80.0, self.nc), np.full(self.nc, 2000.0),
                              pvtnum=self.pvtnum + 2 * j[0], satnum=self.satnum + 2 * j[1])

    def shifted(self):
        """a second state from the same cells: every cell takes the state of the next cell of its (preg, sreg, hc) group, so that the
        reference of the new state is a permutation of the old one's.  Returns (state, so_max, perm)."""
        perm = np.arange(self.nc)
        key = self.pvtnum * 100 + self.satnum * 10 + self.state.hc
        for k in np.unique(key):
            i = np.flatnonzero(key == k)
            perm[i] = np.roll(i, -1)
        s = self.state
        return decks.State(s.p[perm], s.sat[perm], s.rs[perm], s.rv[perm], s.hc[perm]), self.so_max[perm], perm


def _build_base(C):
    T = R.Tables(C.tab)
    for r in (0, 1):
        S = T.sat(r)
        xw, xg, swco = S["sw"], S["sg"], float(S["sw"][0])
        # Sw on every SWOF node, below the first, above the last
        # (region 1 has Swco = 0: "below the first node" and "Sw <= Swco" are then a NEGATIVE Sw -- no physical state, but what an
        # overshooting Newton update hands the evaluator, and the only way to reach those two clamps; these cells are on the connected
        # grid of test_gpu_cell_edges.py as well, where the flux terms take them like any other)
        for k, node in enumerate(xw):
            for v in around(node):
                C.add("sw_node", r, r, r, sw=v, sg=min(SG0, max(0.0, (1.0 - v) / 2)))
            C.add("sw_node", r, 1 - r, r, sw=node, sg=min(SG0, max(0.0, (1.0 - node) / 2)))       # pvtnum != satnum
        C.add("sw_below", r, r, r, sw=xw[0] - 0.03); C.add("sw_above", r, r, r, sw=xw[-1] + 0.02, sg=0.0)
        C.add("sw_interior", r, r, r); C.add("sw_interior", r, 1 - r, r, sw=0.61, sg=0.22)
        # Sg on every SGOF node (0 and the last one among them), beyond the last
        for node in xg:
            for v in around(node):
                C.add("sg_node", r, r, r, sg=v, sw=min(SW0, (1.0 - node) / 2))
            C.add("sg_node", r, 1 - r, r, sg=node, sw=min(SW0, (1.0 - node) / 2))
        C.add("sg_beyond", r, r, r, sg=xg[-1] + 0.03, sw=0.02)
        # sgeq = (Sg + Sw') - Swco on an SGOF node; Sw' = Sw above Swco and Swco below
        for node in xg[1:-1]:
            for sw in (swco + 0.13, swco - 0.05):
                swp = max(sw, swco)
                for sg in bracket(lambda s: (s + swp) - swco, node + swco - swp, float(node), 1.0):
                    if sg > 0.0:
                        C.add("sgeq_node", r, r, r, sw=sw, sg=sg)
        # Sg + Sw' on an SWOF node with Sg > 0
        for node in xw[1:]:
            sw = swco + 0.03
            for sg in bracket(lambda s: s + sw, node - sw, float(node), 1.0):
                C.add("swow_node", r, r, r, sw=sw, sg=sg)
        # the kro blend: d = (Sg + Sw') - Swco at 0, inside (0, eps/2), eps/2, inside (eps/2, eps), eps, just above; Sw <= Swco and Sw > Swco
        for above, sw in ((False, swco - 0.03), (False, swco), (True, swco + 2e-6)):
            swp = max(sw, swco)
            d = lambda s: (s + swp) - swco
            C.add("blend", r, r, r, sw=sw, sg=0.0)                                                  # d == 0 (or Sw - Swco)
            for t in (0.25 * EPS, 0.75 * EPS, 1.0001 * EPS, 1.3 * EPS):
                C.add("blend", r, r, r, sw=sw, sg=bracket(d, t + swco - swp, t, swp)[1])
            for t in (EPS / 2, EPS):
                for sg in bracket(d, t + swco - swp, t, swp):
                    C.add("blend", r, r, r, sw=sw, sg=sg)
            C.add("blend", r, 1 - r, r, sw=sw, sg=bracket(d, 0.75 * EPS + swco - swp, 0.75 * EPS, swp)[1])
    for r in (0, 1):
        O, G = T.oil(r), T.gas(r)
        # p on every node of the saturated oil curve (free gas: the saturated branch), below, above
        for node in O["psat"]:
            for v in around(node):
                C.add("p_node", r, r, r, p=v)
            C.add("p_node", r, r, 1 - r, p=node)
            C.add("p_node", r, r, r, p=node, hc=GG, rv=RV0)                                        # gas only: the oil PVT is saturated too
        C.add("p_below", r, r, r, p=O["psat"][0] - 7 * BAR); C.add("p_above", r, r, r, p=O["psat"][-1] + 30 * BAR)
        C.add("p_interior", r, r, r); C.add("p_interior", r, r, 1 - r, p=212.7 * BAR)
        # p_g on every node of the saturated gas curve: saturation region 1 (p_g == p)
        for node in G["pg"]:
            for v in around(node):
                C.add("pg_node", r, r, 1, p=v)
            C.add("pg_node", r, r, 1, p=node, hc=OO)                                               # oil only: the gas PVT is saturated too
        C.add("pg_below", r, r, 1, p=G["pg"][0] - 9 * BAR); C.add("pg_above", r, r, 1, p=G["pg"][-1] + 40 * BAR)
        C.add("pg_interior", r, r, 1); C.add("pg_interior", r, r, 0, p=231.9 * BAR)
        # oil only: rs on every node, below, above
        for node in O["rs"]:
            for v in around(node):
                C.add("rs_node", r, r, r, rs=v, hc=OO)
            C.add("rs_node", r, r, 1 - r, rs=node, hc=OO)
        C.add("rs_below", r, r, r, rs=O["rs"][0] - 3.0, hc=OO); C.add("rs_above", r, r, r, rs=O["rs"][-1] + 20.0, hc=OO)
        C.add("rs_interior", r, r, r, hc=OO)
        # oil only: p on the nodes of the lower bracketing column only and of the upper only (x[1] and x[2] of the 4-point columns
        # among them), below a column's first point, above its last
        for i in (0, 2):
            rs = 0.4 * O["rs"][i] + 0.6 * O["rs"][i + 1]
            lo, up = O["col_y"][i], O["col_y"][i + 1]
            for node in np.concatenate([lo, up]):
                for v in around(node):
                    C.add("oilcol_node", r, r, r, p=v, rs=rs, hc=OO)
            C.add("oilcol_below", r, r, r, p=min(lo[0], up[0]) - 10 * BAR, rs=rs, hc=OO)
            C.add("oilcol_above", r, r, r, p=max(lo[-1], up[-1]) + 20 * BAR, rs=rs, hc=OO)
            C.add("oilcol_interior", r, r, 1 - r, rs=rs, hc=OO)
        # gas only: rv on the column nodes (0 among them), above rvSat; p_g on a node
        i = 1
        p = 0.45 * G["pg"][i] + 0.55 * G["pg"][i + 1]
        for node in np.unique(np.concatenate([G["col_y"][i], G["col_y"][i + 1]])):
            for v in around(node):
                C.add("rv_node", r, r, 1, p=p, rv=v, hc=GG)
        C.add("rv_above", r, r, 1, p=p, rv=1.3 * max(G["col_y"][i][-1], G["col_y"][i + 1][-1]), hc=GG)
        C.add("rv_interior", r, r, 1, p=p, hc=GG); C.add("rv_interior", r, r, 0, p=p, hc=GG, sw=0.31)
        for node in G["pg"]:
            for v in around(node):
                C.add("rv_pg_node", r, r, 1, p=v, hc=GG)


def _build_vap(C):
    for r in (0, 1):
        so = lambda sg: (1.0 - SW0) - sg
        s0 = so(SG0)
        C.add("vap_equal", r, r, r, so_max=s0)                                                     # so == so_max: no factor
        C.add("vap_just_below", r, r, r, so_max=np.nextafter(s0, np.inf))
        C.add("vap_active", r, r, r, so_max=0.7); C.add("vap_active", r, 1 - r, r, so_max=0.8, hc=OO)
        C.add("vap_inactive", r, r, r, so_max=0.3)
        sg = bracket(so, 1.0 - SW0 - 0.005, 0.005, 1.0)[1]
        C.add("vap_guard_at", r, r, r, sg=sg, so_max=0.01)                                         # so_max == 0.01: no factor
        C.add("vap_guard_above", r, r, r, sg=sg, so_max=np.nextafter(0.01, np.inf))
        sg = bracket(lambda s: -so(s), 1.0 - SW0, 0.0, 1.0)[1]
        assert so(sg) == 0.0
        C.add("vap_so_zero", r, r, r, sg=sg, so_max=0.4)                                           # so == 0: the floor max(so, 1.49e-8)
        C.add("vap_so_zero", r, r, r, hc=GG, so_max=0.4)


def _build_rock(C):
    x = C.tab.rocktab_p
    for r in (0, 1):
        for node in x:
            for v in around(node):
                C.add("rocktab_node", r, r, r, p=v)
        C.add("rocktab_below", r, r, r, p=x[0] - 25 * BAR); C.add("rocktab_above", r, r, r, p=x[-1] + 35 * BAR)
        C.add("rocktab_interior", r, r, 1 - r); C.add("rocktab_interior", r, r, r, hc=OO); C.add("rocktab_interior", r, r, r, hc=GG)


# category -> (table set, what the branch record must show).  Node categories also list, per region, which nodes were hit.
def _col_only(which):
    return lambda b: b["oil"] == "under" and b["oil_col"][which].at >= 0 and b["oil_col"][1 - which].at < 0


CENSUS = {
    "sw_node": ("base", lambda b: b["swof"].at >= 0), "sw_below": ("base", lambda b: b["swof"].side < 0 and b["swof"].at < 0),
    "sw_above": ("base", lambda b: b["swof"].side > 0 and b["swof"].at < 0),
    "sg_node": ("base", lambda b: b["sgof"].at >= 0), "sg_beyond": ("base", lambda b: b["sgof"].side > 0 and b["sgof"].at < 0),
    "sgeq_node": ("base", lambda b: b["krog"].at > 0), "swow_node": ("base", lambda b: b["krow"].at > 0 and b["sg"] > 0),
    "blend:k2:below": ("base", lambda b: b["blend"] == "k2" and not b["above_swco"]),
    "blend:k2:above": ("base", lambda b: b["blend"] == "k2" and b["above_swco"]),
    "blend:interp:below": ("base", lambda b: b["blend"] == "interp" and not b["above_swco"]),
    "blend:interp:above": ("base", lambda b: b["blend"] == "interp" and b["above_swco"]),
    "blend:full:below": ("base", lambda b: b["blend"] == "full" and b["d"] < 2 * EPS and not b["above_swco"]),
    "blend:full:above": ("base", lambda b: b["blend"] == "full" and b["d"] < 2 * EPS and b["above_swco"]),
    "blend:d==0": ("base", lambda b: b["d"] == 0.0),
    "p_node": ("base", lambda b: b["psat"].at >= 0), "p_below": ("base", lambda b: b["psat"].side < 0), "p_above": ("base", lambda b: b["psat"].side > 0),
    "pg_node": ("base", lambda b: b["pg"].at >= 0), "pg_below": ("base", lambda b: b["pg"].side < 0), "pg_above": ("base", lambda b: b["pg"].side > 0),
    "rs_node": ("base", lambda b: b["oil"] == "under" and b["rs_node"].at >= 0),
    "rs_below": ("base", lambda b: b["oil"] == "under" and b["rs_node"].side < 0),
    "rs_above": ("base", lambda b: b["oil"] == "under" and b["rs_node"].side > 0),
    "oilcol_node:lower_only": ("base", _col_only(0)), "oilcol_node:upper_only": ("base", _col_only(1)),
    "oilcol_node:x1_of_4": ("base", lambda b: b["oil"] == "under" and any(c.at == 1 and c.n == 4 for c in b["oil_col"])),
    "oilcol_node:x2_of_4": ("base", lambda b: b["oil"] == "under" and any(c.at == 2 and c.n == 4 for c in b["oil_col"])),
    "oilcol_below": ("base", lambda b: b["oil"] == "under" and all(c.side < 0 for c in b["oil_col"])),
    "oilcol_above": ("base", lambda b: b["oil"] == "under" and all(c.side > 0 for c in b["oil_col"])),
    "rv_node": ("base", lambda b: b["gas"] == "under" and any(c.at > 0 for c in b["gas_col"])),
    "rv_node:zero": ("base", lambda b: b["gas"] == "under" and all(c.at == 0 for c in b["gas_col"])),
    "rv_above": ("base", lambda b: b["gas"] == "under" and all(c.side > 0 for c in b["gas_col"])),
    "rv_pg_node": ("base", lambda b: b["gas"] == "under" and b["pg"].at >= 0),
    "vap_equal": ("vap", lambda b: b["vap"] == ((False, False),) * 2), "vap_just_below": ("vap", lambda b: b["vap"] == ((True, False),) * 2),
    "vap_guard_at": ("vap", lambda b: b["vap"] == ((False, False),) * 2), "vap_guard_above": ("vap", lambda b: b["vap"] == ((True, False),) * 2),
    "vap_so_zero": ("vap", lambda b: b["vap"] == ((True, True),) * 2),
    "rocktab_node": ("rock", lambda b: b["rocktab"].at >= 0), "rocktab_below": ("rock", lambda b: b["rocktab"].side < 0),
    "rocktab_above": ("rock", lambda b: b["rocktab"].side > 0),
}
# the blend argument exactly ON eps / 2 and eps: reachable only with Swco = 0 (module docstring)
EXACT_ONLY_IN_REGION_1 = {"blend:d==eps/2": lambda b: b["d"] == EPS / 2, "blend:d==eps": lambda b: b["d"] == EPS}
# node categories -> the search whose every node must be hit, in both regions
ALL_NODES = {"sw_node": "swof", "sg_node": "sgof", "p_node": "psat", "pg_node": "pg", "rs_node": "rs_node", "rocktab_node": "rocktab"}


def census(sets):
    """{category: [cells in region 0, in region 1]} by the reference's branch record; asserts that none is empty and that the node
    categories hit every node"""
    out = {}
    for name, (tset, pred) in CENSUS.items():
        C = sets[tset]
        tag = name.split(":")[0]
        n = [sum(1 for c in np.flatnonzero((C.cat == tag) & (C.region == r)) if pred(C.recs[c])) for r in (0, 1)]
        assert min(n) > 0, "category %s is empty in a region: %r" % (name, n)
        out[name] = n
        if name in ALL_NODES:
            for r in (0, 1):
                hit = [C.recs[c][ALL_NODES[name]] for c in np.flatnonzero((C.cat == tag) & (C.region == r))]
                assert {s.at for s in hit if s.at >= 0} == set(range(hit[0].n)), (name, r)
    C = sets["base"]
    for name, pred in EXACT_ONLY_IN_REGION_1.items():
        n = [sum(1 for c in np.flatnonzero((C.cat == "blend") & (C.region == r)) if pred(C.recs[c])) for r in (0, 1)]
        assert n[0] == 0 and n[1] > 0, (name, n)
        out[name] = n
    return out


_loaded = None


def load():
    """{table set: CaseSet} with the reference evaluated, and the census (asserted)"""
    global _loaded
    if _loaded is None:
        sets = {}
        for tset, build in (("base", _build_base), ("vap", _build_vap), ("rock", _build_rock)):
            C = CaseSet(tset)
            build(C)
            sets[tset] = C.finish()
        _loaded = (sets, census(sets))
    return _loaded


BLEND_ZONE = "blend zone"


def hc_groups(C):
    """the groups over which an error is normalised: the cells of each hydrocarbon state, those where the three-phase law DIVIDES by
    d = (Sg + Sw') - Swco < 2 eps apart (the interpolated zone and the first floats of the plain law above it; all with gas and oil) --
    their d kro is ill-conditioned in float64 (oracle_limits below), and in a group of their own they do not set the yardstick of the
    node cells"""
    interp = np.array([b["blend"] != "k2" and b["d"] < 2 * EPS for b in C.recs])
    out = {name: np.flatnonzero((C.state.hc == hc) & ~interp) for name, hc in (("gas+oil", GO), ("oil", OO), ("gas", GG))}
    out[BLEND_ZONE] = np.flatnonzero(interp)
    return out


# Slots in which the ORACLE is not within 1e-12 of the reference, each with the bound its explanation gives:
# d kro / d(Sw, Sg) where the law divides by d in [eps / 2, 2 eps).  k1 = num / d has k1' = (num' - k1 d') / d: two terms next to 1 that
# cancel to O(d), over d; and in the interpolated zone kro = k2 al + k1 (1 - al) with al = (eps - d) / (eps / 2) has the two terms
# k2 al' and -k1 al', each |al'| = 2 / eps = 2e5 times a number next to 1, cancelling to O(1).  Each term carries one ulp(1) of rounding
# at least, so the derivative has an absolute error of 2 ulp(1) * 2 / eps = 8.9e-11 in ANY float64 evaluation of the rule as it is
# written; divided by the slot's largest entry in the zone.  mob_o = kro / mu_o inherits it.
ORACLE_TOL = 1e-12
BLEND_ABS = 2 * 2.0 ** -52 * (2.0 / EPS)
EXPLAINED = {("kr_o", 2), ("kr_o", 3), ("mob_o", 2), ("mob_o", 3)}           # in the BLEND_ZONE group only


def oracle_limits(C, names):
    """{group: limit[len(names)][4]} of the oracle's error: 1e-12, and in the EXPLAINED slots of the blend zone the bound stated above"""
    out = {}
    for g, idx in hc_groups(C).items():
        if idx.size:
            lim = np.full((len(names), 4), ORACLE_TOL)
            for n, s in EXPLAINED:
                if g == BLEND_ZONE and n in names:
                    scale = np.abs(C.ref[idx][:, R.NAMES.index(n), s]).max()
                    if n == "mob_o":      # the same absolute error of kro over the smallest viscosity of the group
                        scale = scale * np.abs(C.ref[idx][:, R.NAMES.index("mu_o"), 0]).min()
                    lim[names.index(n), s] = max(ORACLE_TOL, BLEND_ABS / scale)
            out[g] = lim
    return out


def oracle_props(orc, C):
    """oracle.cell_props of the cells of C: [nc][23][4] in the order of the first 23 names of cell_reference.NAMES"""
    assert orc.PROP_NAMES == R.NAMES[:orc.NPROP]
    orc.set_sat_oil_max(C.so_max if C.tab.vap1 > 0.0 or C.tab.vap2 > 0.0 else None)
    try:
        return orc.cell_props(C.grid(), C.tab, C.state)
    finally:
        orc.set_sat_oil_max(None)


def error_table(C, got, names, slots=(0, 1, 2, 3)):
    """{hc group: err[len(names)][len(slots)]}: err of a (property, slot) = max |got - ref| / max |ref| over the cells of the group (a slot
    the reference has identically zero must be identically zero: inf otherwise).  got: [nc][len(names)][len(slots)]."""
    k = [R.NAMES.index(n) for n in names]
    out = {}
    for g, idx in hc_groups(C).items():
        if idx.size:
            ref = C.ref[idx][:, k][:, :, list(slots)]
            d, s = np.abs(np.asarray(got)[idx] - ref).max(0), np.abs(ref).max(0)
            out[g] = np.where(s > 0, d / np.where(s > 0, s, 1.0), np.where(d > 0, np.inf, 0.0))
    return out


def worst(tables_):
    """the entrywise maximum of error tables of the same shape"""
    return np.maximum.reduce([np.asarray(t) for t in tables_])


def format_table(err, names, slots=(0, 1, 2, 3)):
    head = "%-8s " % "" + " ".join("%-8s" % R.SLOTS[s] for s in slots)
    return "\n".join([head] + ["%-8s " % n + " ".join("%-8.1e" % v for v in row) for n, row in zip(names, err)])


def connected(C, seed=11):
    """the cells of C shuffled onto a small Cartesian grid with gravity (the last layer filled up with the first cells again):
    (grid, state, so_max)"""
    nx = ny = 10
    nz = -(-C.nc // (nx * ny))
    g = decks.cartesian_grid(nx, ny, nz, lognormal_sigma=0.5)
    src = np.random.default_rng(seed).permutation(g.nc) % C.nc
    grid = decks.GridData(g.nc, g.conn_cells, g.trans, g.pv, g.z, gravity=g.gravity, dims=g.dims, pvtnum=C.pvtnum[src], satnum=C.satnum[src])
    s = C.state
    return grid, decks.State(s.p[src], s.sat[src], s.rs[src], s.rv[src], s.hc[src]), C.so_max[src]
