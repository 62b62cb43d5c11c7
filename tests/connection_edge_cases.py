"""The connection half of k_assemble_rows (csrc/blackoil.hip) at the places where a flux kernel makes a discrete choice: a handmade grid of
NC = 650 cells (three 256-row chunks, the last one partial, the last wave ragged), its states, and the per-connection measure of
tests/test_connection_cases.py (CPU: conditioning, census, controls) and tests/test_gpu_connection_edges.py (the device).

Tables (tables()): ONE table set with two saturation and two PVT regions.
    satnum 0   decks.satfunc_standard_tables();
    satnum 1   the same curves with pcow and pcgo zero at every node: p_w = p_o = p_g = p exactly;
    pvtnum 0   the standard PVT;  pvtnum 1: another water (B_w 1.03, mu_w 0.40 cP), Rs nodes times 0.6, Rv nodes times 2, other surface
               densities -- so that two cells of EQUAL pressure differ in U_w, RsSat and RvSat.
    copies > 1 repeats the four regions (a table blob past the 24 KiB the kernels stage in LDS).
kind "wo" is the same grid on an oil-water deck (tests/twophase.py's PVT, the standard SWOF and its zero-pc copy) with the three-phase
twin the oracle evaluates.

Named cases (PAIR_CASES, eight instances each): every instance is a connection (c1, c2) as the caller lists it; each case is listed
ascending and descending in caller numbering, and dealt to the candidate pairs of the graph so that it falls inside one 256-row chunk
and across two in both of the solver's numberings (_build; census: test_connection_cases.py).
    oil tie              satnum 0, z1 == z2, p1 == p2, both ends oil-only with different Sw and Rs; thp == 0 on a deck with thpres
    three-phase tie      satnum 1, z1 == z2, p1 == p2, pvtnum 0 | 1, gas and oil at both ends: U_w, U_o, U_g, rs and rv all differ;
                         the first two instances have no other connection (their residual after a first assembly is exactly 0)
    water tie by region  same satnum (0 and 1 in turn), Sw, Sg, p, z; pvtnum 0 | 1
    dh == +thp, dh == -thp   satnum 1, z1 == z2, p1 - p2 == +-1 bar == +-thp exactly (pressures are multiples of 2^-10 bar)
    one float below      the same with thp = nextafter(1 bar, inf): closed;  one float above: thp = nextafter(1 bar, 0): open by one ulp
    T == 0, T == 5e-324, T == 1e-300   ordinary states; the first two T == 0 instances join two cells that have nothing else
    hub                  one cell with 44 non-neighbour connections to cells all over the caller numbering
    leaf, isolated       cells with one connection and with none
    thp == 0, closed     ordinary connections that carry 0 and 200 bar on the deck with thpres
    ordinary             everything else: gravity, depth differences, random states of all three hydrocarbon states
Variants of the grid: "base" (gravity, thpres), "g0" (gravity == 0, depths scattered over 50 m, also at the ties), "nothp" (no thpres
array: the kernel's other branch; every threshold case is then an ordinary connection with |dh| = 1 bar).

The condition on the inputs (test_connection_cases.py checks it on the oracle's cell values, for every (connection, phase)):
    exact   gravity * (z1 - z2) == 0 and p_a1 - p_a2 is one IEEE subtraction of state values: the oil phase, any phase of satnum 1, or a
            phase whose pressure is evaluated from bit-identical inputs at both ends (same satnum, saturation and pressure: the water tie
            by region, the gas phase between the two oil-only cells of an oil tie) -- the phase pressures are then equal bit for bit;
    far     |dh| >= 1e-3 (|p1| + |p2|) and, with a threshold, ||dh| - thp| >= 1e-3 (|p1| + |p2|).
How the states meet it: the connected cells get pressures from a colouring of the graph, 8 bar per colour and less than 0.5 bar of
jitter; capillary pressures differ by at most 1.9 bar, depths by at most 5 m (0.5 bar), the threshold cases by 1 bar.
NOT pinned: near-hydrostatic vertical neighbours.  The device forms (g dz) * rho_avg, the oracle g * (rho_avg * dz); where that rounding
decides the upwind cell the two may differ legitimately, and such connections are deliberately left out of this fixture.
"""
import ctypes as C

import numpy as np

import twophase
from opmgpu import capi, decks

BAR = decks.BAR
NC = 650
CHUNK, SLICE = 256, 64
Q = BAR * 2.0 ** -10                 # every pressure is a multiple of 2^-10 bar: differences are exact
D_THP = 1024 * Q                     # 1 bar, the pressure difference of the threshold cases
RTOL_JAC = 1e-11                     # tests/test_gpu_assembly.py, tests/test_gpu_cell_edges.py; here per connection
RTOL_JAC_F32 = 2e-6                  # a float Jacobian
FAR = 1e-3
N_HUB = 44
MAX_DEG = 6                          # every row but the hub's has 1 to 7 entries
PAIR_CASES = ("oil tie", "three-phase tie", "water tie by region", "dh == +thp", "dh == -thp", "one float below", "one float above",
              "T == 0", "T == 5e-324", "T == 1e-300")
TIES = ("oil tie", "three-phase tie", "water tie by region")
AT_THP = ("dh == +thp", "dh == -thp")
T_CASES = {"T == 0": 0.0, "T == 5e-324": 5e-324, "T == 1e-300": 1e-300}
PER_CASE = 8                         # instances of a pair case, half of them listed descending
VARIANTS = ("base", "g0", "nothp")
NAMES = ["p_w", "p_o", "p_g", "b_w", "b_o", "b_g", "mu_w", "mu_o", "mu_g", "kr_w", "kr_o", "kr_g", "rho_w", "rho_o", "rho_g", "mob_w", "mob_o",
         "mob_g", "rs", "rv", "accum_w", "accum_o", "accum_g"]          # oracle.PROP_NAMES
SLOTS = ["d%s/d%s" % (e, v) for e in "wog" for v in ("p", "Sw", "X")]


# ------------------------------------------------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------------------------------------------------
def tables(copies=1, **extra):
    """the table set of the docstring, its four regions `copies` times over (region r of copy k is number 2 k + r)"""
    t = decks.satfunc_standard_tables(regions=2 * copies, **extra)
    for k in range(copies):
        s, r = 2 * k + 1, 2 * k + 1
        t.swof_pcow[t.swof_ptr[s]:t.swof_ptr[s + 1]] = 0.0
        t.sgof_pcgo[t.sgof_ptr[s]:t.sgof_ptr[s + 1]] = 0.0
        t.pvtw[r] = [1.0 * BAR, 1.03, 4.0e-5 / BAR, 0.40 * decks.CP, 0.0]
        t.surface_density[r] = [1020.0, 750.0, 1.2]
        t.oil_rs[t.oil_node_ptr[r]:t.oil_node_ptr[r + 1]] *= 0.6
        a, b = t.gas_node_ptr[r], t.gas_node_ptr[r + 1]
        t.gas_rvsat[a:b] *= 2.0
        t.gas_col_rv[t.gas_col_ptr[a]:t.gas_col_ptr[b]] *= 2.0
    return t


def _swof(copies):
    std = twophase.SWOF[0]
    return [std, [(a, b, c, 0.0) for a, b, c, _ in std]] * copies


def tables_wo(copies=1):
    """the oil-water deck: tests/twophase.py's two PVT regions, the standard SWOF and its zero-pc copy"""
    return decks.FluidTables(density_wog=twophase.DENSITY_WO * copies, pvtw=twophase.PVTW * copies,
                             pvto=[twophase._dead_oil(r) for r in twophase.PVDO] * copies, pvtg=None, swof=_swof(copies), sgof=None,
                             rock=twophase.ROCK, phases="wo")


def twin_wo(copies=1, gas=0):
    """its three-phase twin, built as twophase.twin_tables builds one"""
    swof = _swof(copies)
    sgof = [[(0.0, 0.0, t[0][2], 0.0), (1.0 - t[0][0], 0.0, 0.0, 0.0)] for t in swof]
    pvdg, rho_g = twophase.GASES[gas]
    return decks.FluidTables(density_wog=[d + [rho_g] for d in twophase.DENSITY_WO] * copies, pvtw=twophase.PVTW * copies,
                             pvto=[twophase._dead_oil(r) for r in twophase.PVDO] * copies,
                             pvtg=[[(p, [(0.0, B, mu)]) for p, B, mu in pvdg]] * (2 * copies), swof=swof, sgof=sgof, rock=twophase.ROCK,
                             disgas=False, vapoil=False)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the graph
# ------------------------------------------------------------------------------------------------------------------------------------------
class Fixture:
    """conn [nconn][2] (as the caller lists them), trans, thpres, z, pv, satnum, pvtnum, case [nconn] (name of every connection),
    hub / leaves / isolated (cells), tied (pairs whose pressures are related: (c1, c2, p1 - p2))"""


_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = _build()
    return _FIXTURE


N_SLOTS = 112                        # candidate pairs: the named cases take 80 of them, the others stay ordinary connections


def _pattern(conn):
    """BSR pattern of the graph, diagonal included and columns ascending (what oracle.pattern gives)"""
    a = np.concatenate([conn[:, 0], conn[:, 1], np.arange(NC)])
    b = np.concatenate([conn[:, 1], conn[:, 0], np.arange(NC)])
    o = np.lexsort((b, a))
    return np.concatenate([[0], np.cumsum(np.bincount(a, minlength=NC))]).astype(np.int32), b[o].astype(np.int32)


def _build(seed=2024):
    """The graph first: hub, leaves, isolated cells, N_SLOTS candidate pairs (the first eight with no other connection), a background of
    chains, strides and random non-neighbour connections, and up to three more connections of every candidate cell.  The cases are then
    dealt to the candidate pairs BY the solver's two numberings (the host-side planner: the sparsity pattern is all it reads), so that
    every case is found inside one 256-row chunk and across two in both; left to chance a connected pair of the multicolour order
    almost never shares a chunk.  Orientation, transmissibility, threshold, regions and depths follow from the case."""
    rng = np.random.Generator(np.random.PCG64(seed))
    F = Fixture()
    conn, trans, thp, case = [], [], [], []
    pairs, deg = set(), np.zeros(NC, int)
    satnum, pvtnum = rng.integers(0, 2, NC).astype(np.int32), rng.integers(0, 2, NC).astype(np.int32)
    F.tied, F.role = [], {}                  # role: cell -> (case, end 0 | 1, instance) of the special cells

    def ordinary_T():
        return 2e-13 * np.exp(0.8 * rng.standard_normal())

    def ordinary_thp():
        return float(rng.choice([0.0, 0.0, 0.2 * BAR, 0.7 * BAR, 1.5 * BAR, 200.0 * BAR]))

    def label(th):
        return "thp == 0" if th == 0.0 else ("closed" if th > 100 * BAR else "ordinary")

    def join(a, b, T, th, name, cap=True):
        key = (min(a, b), max(a, b))
        if a == b or key in pairs or (cap and (deg[a] >= MAX_DEG or deg[b] >= MAX_DEG)):
            return False
        pairs.add(key); deg[a] += 1; deg[b] += 1
        conn.append([a, b]); trans.append(T); thp.append(th); case.append(name)
        return True

    def ordinary(a, b, cap=True):
        if rng.random() < 0.5:
            a, b = b, a
        th = ordinary_thp()
        return join(a, b, ordinary_T(), th, label(th), cap)

    order = rng.permutation(NC).tolist()     # the special cells are spread over the whole caller numbering
    used = set()

    def take(src=order):
        while True:
            c = src.pop()
            if c not in used:
                used.add(c)
                return c

    F.hub = take()
    F.isolated = []
    while len(F.isolated) < 3:               # an isolated cell sits between connected ones in caller numbering
        c = take()
        if 0 < c < NC - 1 and not {c - 1, c + 1} & ({F.hub} | set(F.isolated)):
            F.isolated.append(c)
        else:
            used.discard(c)
    F.leaves = [take() for _ in range(4)]
    # (the multicolour order puts a connected pair into one chunk where a colour ends inside the chunk: the last rows of colour 0, which
    # are the LATE cells of the caller numbering, next to colour 1 -- so 30 pairs have both ends among the last 80 cells and few other
    # connections)
    top = [c for c in order if c >= NC - 80]
    slots, late = [], set()
    for i in range(N_SLOTS):
        if 8 <= i < 38 and len(top) > 4:
            a, b = take(top), take(top)
            late.update((a, b))
        else:
            a, b = take(), take()
        assert join(a, b, 0.0, 0.0, "candidate")
        slots.append(len(conn) - 1)
    alone_slots, alone = slots[:8], {c for f in slots[:8] for c in conn[f]}
    candidate_cells = sorted(c for f in slots for c in conn[f])
    background = sorted(set(range(NC)) - set(candidate_cells) - {F.hub} - set(F.isolated) - set(F.leaves))
    nb = len(background)
    # the hub first (its neighbours keep room for it), then chains, strides and random non-neighbour connections among the background
    for c in background[3::max(1, nb // N_HUB)][:N_HUB]:
        a, b = (F.hub, c) if rng.random() < 0.5 else (c, F.hub)
        assert join(a, b, ordinary_T(), ordinary_thp() if rng.random() < 0.5 else 0.0, "hub", cap=False)
    deg[F.hub] = 0                           # (the cap is for the other rows)
    for i in range(nb - 1):
        if rng.random() < 0.8:
            ordinary(background[i], background[i + 1])
    for i in range(nb - 23):
        if rng.random() < 0.5:
            ordinary(background[i], background[i + 23])
    for _ in range(60):
        ordinary(int(rng.choice(background)), int(rng.choice(background)))
    for c in F.leaves:
        while not ordinary(c, int(rng.choice(background))):
            pass
    for c in candidate_cells:                # 0 to 3 more connections of a candidate cell: its diagonal is first, last or in between
        if c not in alone:
            for _ in range(int(rng.integers(0, 2 if c in late else 4))):
                ordinary(c, int(rng.choice(background)))
    deg[F.hub] = N_HUB
    conn = np.array(conn, np.int32)
    # ---- deal the cases to the candidate pairs
    rowptr, col = _pattern(conn)
    same = np.stack([plan_position(rowptr, col, o)[conn[:, 0]] // CHUNK == plan_position(rowptr, col, o)[conn[:, 1]] // CHUNK
                     for o in (capi.ORDER_NATURAL, capi.ORDER_MULTICOLOR)], 1)
    free, alone_free = [f for f in slots if f not in alone_slots], list(alone_slots)
    for name in PAIR_CASES:
        mine = [alone_free.pop(0), alone_free.pop(0)] if name in ("three-phase tie", "T == 0") else []
        want = {(o, v) for o in (0, 1) for v in (False, True)} - {(o, bool(same[f, o])) for f in mine for o in (0, 1)}
        while len(mine) < PER_CASE:
            gain = [len(want & {(0, bool(same[f, 0])), (1, bool(same[f, 1]))}) for f in free]
            f = free.pop(int(np.argmax(gain)) if max(gain) > 0 else -1)     # (nothing left to cover: a pair from the end, not a late one)
            want -= {(0, bool(same[f, 0])), (1, bool(same[f, 1]))}
            mine.append(f)
        for k, f in enumerate(mine):
            a, b = conn[f].tolist()
            c1, c2 = (min(a, b), max(a, b)) if k % 2 == 0 else (max(a, b), min(a, b))
            conn[f] = (c1, c2)
            T, th = T_CASES.get(name, None), 0.0
            if T is None:
                T = ordinary_T()
            if name in AT_THP:
                th = D_THP
            elif name == "one float below":
                th = np.nextafter(D_THP, np.inf)
            elif name == "one float above":
                th = np.nextafter(D_THP, 0.0)
            elif name in T_CASES:
                th = [0.0, 0.3 * BAR][k % 2]
            trans[f], thp[f], case[f] = T, th, name
            F.role[c1], F.role[c2] = (name, 0, k), (name, 1, k)
            if name in TIES:
                F.tied.append((c1, c2, 0.0))
            elif name not in T_CASES:
                sign = -1.0 if name == "dh == -thp" or (name.startswith("one float") and k % 4 >= 2) else 1.0
                F.tied.append((c1, c2, sign * D_THP))
            # regions of the special cells (those of a T case stay as drawn)
            if name == "oil tie":
                satnum[[c1, c2]], pvtnum[[c1, c2]] = 0, 0
            elif name == "water tie by region":
                satnum[[c1, c2]] = k // 2 % 2
                pvtnum[c1], pvtnum[c2] = k % 4 // 2, 1 - k % 4 // 2
            elif name not in T_CASES:
                satnum[[c1, c2]] = 1
                pvtnum[c1], pvtnum[c2] = k % 4 // 2, 1 - k % 4 // 2
    for f in free + alone_free:              # the pairs nobody took
        trans[f], thp[f] = ordinary_T(), ordinary_thp()
        case[f] = label(thp[f])
    F.conn = conn
    F.trans, F.thpres, F.case = np.array(trans), np.array(thp), np.array(case)
    F.satnum, F.pvtnum, F.deg = satnum, pvtnum, deg
    F.alone = sorted(c for c in F.role if c in alone)
    F.pv = 40.0 * (0.5 + rng.random(NC))
    # depths: within 5 m; equal at the two ends of every tie and threshold case.  g0: scattered over 50 m, everywhere
    F.z = 2000.0 + 5.0 * rng.random(NC)
    for c1, c2, _ in F.tied:
        F.z[c2] = F.z[c1]
    F.z_scattered = 2000.0 + 50.0 * rng.random(NC)
    assert np.all(deg[np.array(F.isolated)] == 0) and np.all(deg[np.array(F.leaves)] == 1) and deg[F.hub] == N_HUB
    assert all(deg[c - 1] > 0 and deg[c + 1] > 0 for c in F.isolated)
    assert np.delete(deg, F.hub).max() <= MAX_DEG
    for v in vars(F).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return F


def cases(name):
    """connection numbers of a case"""
    return np.flatnonzero(fixture().case == name)


def grid(variant="base", copies=1, seed=0):
    """the GridData of a variant; copies > 1: the cells' regions drawn from the repeated table set (tables(copies))"""
    F = fixture()
    rng = np.random.Generator(np.random.PCG64(77 + seed))
    k_sat, k_pvt = (rng.integers(0, copies, NC), rng.integers(0, copies, NC)) if copies > 1 else (0, 0)
    return decks.GridData(NC, F.conn, F.trans, F.pv, F.z_scattered if variant == "g0" else F.z, gravity=0.0 if variant == "g0" else decks.GRAVITY,
                          thpres=None if variant == "nothp" else F.thpres, pvtnum=(F.pvtnum + 2 * k_pvt).astype(np.int32),
                          satnum=(F.satnum + 2 * k_sat).astype(np.int32))


def reversed_connection(g, f):
    """`g` with connection f listed the other way round: physically the same connection, but c1 and c2 change places"""
    conn = np.array(g.conn_cells)
    conn[f] = conn[f, ::-1]
    return decks.GridData(g.nc, conn, g.trans, g.pv, g.z, gravity=g.gravity, thpres=g.thpres, pvtnum=g.pvtnum, satnum=g.satnum)


def with_threshold(g, f, thp):
    th = np.array(g.thpres)
    th[f] = thp
    return decks.GridData(g.nc, g.conn_cells, g.trans, g.pv, g.z, gravity=g.gravity, thpres=th, pvtnum=g.pvtnum, satnum=g.satnum)


# ------------------------------------------------------------------------------------------------------------------------------------------
# states
# ------------------------------------------------------------------------------------------------------------------------------------------
def state(seed=1, kind="wog"):
    """a state that meets the condition of the docstring: pressures from a greedy colouring of the graph whose nodes are the cells, the two
    ends of a tie or threshold case taken as one node; saturations, Rs, Rv and the hydrocarbon state random but at the special cells"""
    F = fixture()
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    node = np.arange(NC)
    for c1, c2, _ in F.tied:
        node[c2] = c1
    adj = [set() for _ in range(NC)]
    for a, b in F.conn.tolist():
        if node[a] != node[b]:
            adj[node[a]].add(node[b]); adj[node[b]].add(node[a])
    colour = -np.ones(NC, int)
    for n in rng.permutation(np.unique(node)).tolist():
        used = {colour[m] for m in adj[n]}
        free = [k for k in range(len(used) + 1) if k not in used]
        colour[n] = free[int(rng.integers(0, min(2, len(free))))]           # the smallest or the next one: a few more pressures
    p = Q * (81920 + 8192 * colour[node] + rng.integers(0, 512, NC)[node])   # 80 bar + 8 bar per colour + less than 0.5 bar
    for c1, c2, d in F.tied:
        p[c2] = p[c1] - d
    # ordinary cells: tests/decks.random_state's recipe
    sw = 0.05 + 0.9 * rng.random(NC)
    sg = (1.0 - sw) * rng.random(NC)
    hc = rng.integers(0, 3, NC).astype(np.int8)
    k = rng.random(NC) < 0.1
    sw[k] = rng.choice(np.array([0.1, 0.2, 0.3, 0.4, 0.7, 0.8, 0.9]), k.sum())
    sg = np.minimum(sg, 1.0 - sw)
    rs, rv = 150.0 * rng.random(NC), 5e-4 * rng.random(NC)
    # the special cells: [end 0, end 1] of (Sw, Sg); the two ends change places from state to state
    ends = {"oil tie": [(0.2, 0.0), (0.7, 0.0)], "three-phase tie": [(0.22, 0.12), (0.45, 0.3)], "water tie by region": [(0.55, 0.2), (0.55, 0.2)]}
    swap = seed % 2
    for c, (name, end, inst) in F.role.items():
        if name in T_CASES:
            continue
        e = ends.get(name, ends["three-phase tie"])[end ^ swap]
        sw[c], sg[c] = e[0] + 0.01 * (inst % 4), e[1]
        if name == "water tie by region":
            sw[c] = e[0] + 0.01 * (inst // 2)                               # the same at both ends
        hc[c] = capi.HC_OIL_ONLY if name == "oil tie" else capi.HC_GAS_AND_OIL
        if name == "oil tie":
            rs[c] = [0.2, 0.4][end ^ swap] * p[c] / BAR                      # RsSat(p) = p / (2 bar) at the nodes: undersaturated
    sg[hc == capi.HC_OIL_ONLY] = 0.0
    so = 1.0 - sw - sg
    go = hc == capi.HC_GAS_ONLY
    sg[go] = 1.0 - sw[go]; so[go] = 0.0
    if kind == "wo":                        # the twin's range of validity: Sw >= Swco + 1e-3, no gas, nothing dissolved
        sw = np.maximum(sw, 0.12)
        return decks.State(p, np.stack([sw, 1.0 - sw, np.zeros(NC)], 1), np.zeros(NC), np.zeros(NC), np.full(NC, capi.HC_GAS_AND_OIL, np.int8))
    return decks.State(p, np.stack([sw, so, sg], 1), rs, rv, hc)


# ------------------------------------------------------------------------------------------------------------------------------------------
# what the oracle's cell values say about every connection (values only: conditioning, census, normalisation of the residual)
# ------------------------------------------------------------------------------------------------------------------------------------------
def connection_values(g, props):
    """per connection and phase, from oracle.cell_props: dict of dh0 (before the threshold), dh (after), open, up (0: c1), U [nconn][3][2]
    (b * mobility at c1, c2), G [nconn][3] (the mass fluxes with the rs / rv cross terms), psum (|p1| + |p2| of the phase pressures)"""
    i = NAMES.index
    c1, c2 = g.conn_cells[:, 0], g.conn_cells[:, 1]
    P = props[:, [i("p_w"), i("p_o"), i("p_g")], 0]
    rho = props[:, [i("rho_w"), i("rho_o"), i("rho_g")], 0]
    U = props[:, [i("b_w"), i("b_o"), i("b_g")], 0] * props[:, [i("mob_w"), i("mob_o"), i("mob_g")], 0]
    dz = (g.z[c1] - g.z[c2])[:, None]
    dh0 = (P[c1] - P[c2]) - g.gravity * ((0.5 * rho[c1] + 0.5 * rho[c2]) * dz)
    dh, is_open = dh0, np.ones_like(dh0, bool)
    if g.thpres is not None:
        is_open = np.abs(dh0) >= g.thpres[:, None]
        dh = np.where(is_open, dh0 - np.sign(dh0) * g.thpres[:, None], 0.0)
    up = np.where(dh >= 0.0, 0, 1)
    Uu = np.where(up == 0, U[c1], U[c2])
    Fl = Uu * (g.trans[:, None] * dh)
    rs = np.where(up[:, 1] == 0, props[c1, i("rs"), 0], props[c2, i("rs"), 0])
    rv = np.where(up[:, 2] == 0, props[c1, i("rv"), 0], props[c2, i("rv"), 0])
    G = np.stack([Fl[:, 0], Fl[:, 1] + rv * Fl[:, 2], Fl[:, 2] + rs * Fl[:, 1]], 1)
    return dict(dh0=dh0, dh=dh, open=is_open, up=up, U=np.stack([U[c1], U[c2]], 2), G=G, psum=np.abs(P[c1]) + np.abs(P[c2]), P1=P[c1], P2=P[c2],
                rs=np.stack([props[c1, i("rs"), 0], props[c2, i("rs"), 0]], 1), rv=np.stack([props[c1, i("rv"), 0], props[c2, i("rv"), 0]], 1))


def exact_by_construction(g, st, nph=3):
    """[nconn][3]: the (connection, phase) pairs whose head difference is one IEEE subtraction of state values (the docstring's rule)"""
    c1, c2 = g.conn_cells[:, 0], g.conn_cells[:, 1]
    flat = g.gravity * (g.z[c1] - g.z[c2]) == 0.0
    s1, s2 = g.satnum[c1] % 2, g.satnum[c2] % 2                  # (copies of the regions keep their parity)
    zero_pc = (s1 == 1) & (s2 == 1)
    same = g.satnum[c1] % 2 == g.satnum[c2] % 2
    tie = same & (st.p[c1] == st.p[c2])
    water = zero_pc | (tie & (st.sat[c1, 0] == st.sat[c2, 0]))
    gas = zero_pc | (tie & (st.sat[c1, 2] == st.sat[c2, 2])) | (nph == 2)
    return flat[:, None] & np.stack([water, np.ones_like(water), gas], 1)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the per-connection measure
# ------------------------------------------------------------------------------------------------------------------------------------------
def block_index(rowptr, col, rows, cols):
    """position of the blocks (rows[i], cols[i]) in a BSR pattern with ascending columns"""
    n = len(rowptr) - 1
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)) * n + col
    want = np.asarray(rows, np.int64) * n + np.asarray(cols, np.int64)
    pos = np.searchsorted(keys, want)
    assert np.array_equal(keys[pos], want)
    return pos


def connection_blocks(rowptr, col, conn, val):
    """[nconn][2][9]: the off-diagonal blocks (c1, c2) and (c2, c1) of every connection.  A pair is never joined twice, so these two blocks
    hold exactly one connection."""
    val = np.asarray(val, np.float64).reshape(-1, 9)
    return np.stack([val[block_index(rowptr, col, conn[:, 0], conn[:, 1])], val[block_index(rowptr, col, conn[:, 1], conn[:, 0])]], 1)


def connection_error(got, ref, both=False):
    """(err [nconn][9], norm [nconn][9]) of blocks from connection_blocks: per (equation, variable) slot, max |got - ref| over the two
    blocks and max |ref| over the same two (both = True: max of |got| and |ref|, the symmetric distance of the controls)"""
    err = np.abs(got - ref).max(1)
    norm = np.maximum(np.abs(ref), np.abs(got)).max(1) if both else np.abs(ref).max(1)
    return err, norm


def relative(err, norm):
    """err / norm; 0 where both are 0, inf where only the norm is"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(norm > 0, err / np.where(norm > 0, norm, 1.0), np.where(err > 0, np.inf, 0.0))


def subnormal_floor(cv, scale):
    """[nconn]: the absolute error allowed next to the relative one.  Where T is subnormal (T == 5e-324) every product with it is rounded
    to a multiple of 2^-1074, an ABSOLUTE error of up to 2^-1075 per operation, which the later factors -- U_up, rs or rv of the upwind
    cell, the scale -- multiply.  16 such roundings (about ten chained operations, twice for the cross terms) times those factors;
    for every T >= 1e-300 this is below 1e-310 and means nothing."""
    amp = np.maximum(1.0, cv["U"].max((1, 2))) * np.maximum(1.0, np.maximum(cv["rs"].max(1), cv["rv"].max(1))) * max(1.0, max(scale))
    return 16 * 2.0 ** -1074 * amp


def row_norms(rowptr, col, ref):
    """[nc][9]: per row and slot, the largest magnitude of the slot among the row's blocks"""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    out = np.zeros((len(rowptr) - 1, 9))
    np.maximum.at(out, rows, np.abs(np.asarray(ref).reshape(-1, 9)))
    return out


def residual_norms(g, cv, dt, accum=None, accum0=None):
    """[nc][3]: per row and equation, the largest of the residual's contributions: |G_a| of the row's connections and, where given, pv / dt
    times |accum_a| of the new and of the old state (a first assembly has accum == accum0 and no such part)"""
    out = np.zeros((g.nc, 3))
    for k in (0, 1):
        np.maximum.at(out, g.conn_cells[:, k], np.abs(cv["G"]))
    if accum is not None:
        pvdt = (g.pv / dt)[:, None]
        out = np.maximum(out, np.maximum(pvdt * np.abs(accum), pvdt * np.abs(accum0)))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# the solver's numbering (host-side planner): chunk relation of a connection, position of the diagonal in a row
# ------------------------------------------------------------------------------------------------------------------------------------------
def plan_position(rowptr, col, ordering):
    lib = capi.load()
    nb = len(rowptr) - 1
    pos, lev, nl = np.zeros(nb, np.int32), np.zeros(nb, np.int32), C.c_int32(0)
    assert lib.opmgpu_plan_ordering(nb, capi.iptr(rowptr), capi.iptr(col), ordering, capi.iptr(pos), capi.iptr(lev), C.byref(nl)) == capi.OK
    return pos


def diagonal_kind(conn, pos):
    """per cell: 'only' (no connection), 'first' (no neighbour before it in the solver's numbering), 'last' or 'middle'"""
    lower, n = np.zeros(NC, int), np.zeros(NC, int)
    for a, b in conn.tolist():
        n[a] += 1; n[b] += 1
        lower[a] += pos[b] < pos[a]; lower[b] += pos[a] < pos[b]
    return np.where(n == 0, "only", np.where(lower == 0, "first", np.where(lower == n, "last", "middle")))
