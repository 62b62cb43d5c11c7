"""The cases of the computeMaxDp tests (tests/test_gpu_thpres.py on the device, tests/test_thpres_reference.py for their conditioning on
the CPU): grid, tables, blocky equilibration regions and a state built to reach every branch of the rule.

    regions   1 | 2 | 3 are slabs in x with random cuts; region 4 is a box at high j and k inside the slabs of 2 and 3, one cell away
              from region 1.  So 1 touches 2 only: the pairs (1, 3) and (1, 4) expect -1 -- also on the grid with NNCs, which join cells of
              any two regions but are not scanned.
    state     random pressures, saturations, Rs, Rv and all three hydrocarbon states, the latter independent of everything else
              (computeMaxDp does not read them);
              Rs above / below RsSat at random; AT RsSat in ~10 % of the cells: those sit exactly on a PVTO node pressure (nodes 2 ..
              n - 2, where the device's segment rule returns the node value itself), with Rs the restatement's RsSat bit for bit.  At a
              node the saturated and the undersaturated 1/Bo coincide, so that a last-bit difference between two evaluations of RsSat,
              which may flip the branch there, cannot move the density (between nodes the two branches differ in the third digit);
              ~10 % of the water and ~10 % of the gas saturations are the cell's residual value bit for bit, some oil saturations 0;
              the cells of region 1 next to region 2 have the higher potential in every phase (pressures 395 .. 415 bar against
              80 .. 200 bar) and all three saturations at their residual values bit for bit -- they do not sum to one, which computeMaxDp,
              reading each saturation on its own, does not ask for: the pair (1, 2) is present with 0.0.
"""
import numpy as np

from opmgpu import capi, decks

import thpres_reference as ref
import twophase as tp


def blocky_eqlnum(dims, seed):
    nx, ny, nz = dims
    rng = np.random.Generator(np.random.PCG64(seed))
    c1 = int(rng.integers(1, nx - 2))                 # region 1: i < c1
    c2 = int(rng.integers(c1 + 2, nx))                # region 2: c1 <= i < c2 (at least two cells wide), region 3: i >= c2
    jc, kc = int(rng.integers(1, ny)), int(rng.integers(1, nz))
    k, j, i = np.unravel_index(np.arange(nx * ny * nz), (nz, ny, nx))
    eq = np.where(i < c1, 1, np.where(i < c2, 2, 3))
    eq[(i > c1) & (j >= jc) & (k >= kc)] = 4
    return eq.astype(np.int32)


def _finish(g, eq, st, smin, rng, nph):
    """residual copies, then the zero pair (1, 2)"""
    n = g.nc
    kw = rng.random(n) < 0.1
    st.sat[kw, 0] = smin[kw, 0]
    if nph == 3:
        kg = rng.random(n) < 0.1
        st.sat[kg, 2] = smin[kg, 2]
    st.sat[:, 1] = 1.0 - st.sat[:, 0] - st.sat[:, 2]
    ko = rng.random(n) < 0.05
    st.sat[ko, 1] = smin[ko, 1]
    c = g.conn_cells
    e1, e2 = eq[c[:, 0]], eq[c[:, 1]]
    hi = np.unique(np.concatenate([c[(e1 == 1) & (e2 == 2), 0], c[(e1 == 2) & (e2 == 1), 1]]))
    lo = np.unique(np.concatenate([c[(e1 == 1) & (e2 == 2), 1], c[(e1 == 2) & (e2 == 1), 0]]))
    lo = lo[eq[lo] == 2]                                  # (an NNC may join the two regions elsewhere: those cells keep their state)
    hi = hi[eq[hi] == 1]
    st.p[hi] = (395.0 + 20.0 * rng.random(hi.size)) * decks.BAR
    st.p[lo] = (80.0 + 120.0 * rng.random(lo.size)) * decks.BAR
    st.sat[hi] = smin[hi]
    return st


def three_phase(dims, endpoints, nnc_fraction=0.0, seed=5):
    """-> (grid, tables, eqlnum, nregions, n_face_conn, state)"""
    g = decks.cartesian_grid(*dims, lognormal_sigma=0.5, seed=seed)
    n_face = g.nconn
    if nnc_fraction > 0:
        g = decks.cartesian_grid(*dims, lognormal_sigma=0.5, seed=seed, nnc_fraction=nnc_fraction)
        assert np.array_equal(g.conn_cells[:n_face], decks.cartesian_grid(*dims, lognormal_sigma=0.5, seed=seed).conn_cells) and g.nconn > n_face
    if endpoints:
        g = decks.with_endpoints(g, decks.random_endpoints(g, seed=seed + 1))
    t = decks.satfunc_standard_tables()
    eq = blocky_eqlnum(dims, seed + 2)
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    n = g.nc
    p = (80.0 + 340.0 * rng.random(n)) * decks.BAR
    nodes = t.oil_psat[2:t.oil_psat.size - 1]
    at = rng.random(n) < 0.1
    p[at] = rng.choice(nodes, int(at.sum()))
    sw = 0.12 + 0.7 * rng.random(n)
    sg = np.where(rng.random(n) < 0.3, 0.0, (1.0 - sw) * rng.random(n))
    rs_sat = np.interp(p, t.oil_psat, t.oil_rs)
    rs = rs_sat * (0.3 + 1.4 * rng.random(n))
    rv = 1.2e-3 * rng.random(n)
    hc = rng.integers(0, 3, n).astype(np.int8)
    st = decks.State(p, np.stack([sw, 1.0 - sw - sg, sg], 1), rs, rv, hc)
    smin = ref.sat_range_min(g, t)
    st = _finish(g, eq, st, smin, rng, 3)
    # Rs AT RsSat, bit for bit the restatement's: after the pressures are final (the zero pair's cells were moved off their nodes)
    from oracle import oracle as orc
    at &= np.isin(st.p, nodes)
    st.rs[at] = orc.pvt(t, "rsSat", st.p[at])[:, 0]
    return g, t, eq, 4, n_face, st


def oil_water(dims, endpoints, seed=5):
    """-> (grid, two-phase tables, twin tables, eqlnum, nregions, n_face_conn, state)"""
    g = tp.grid(*dims, endpoints=endpoints, vertical=endpoints)
    eq = blocky_eqlnum(dims, seed + 2)
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    st = tp.state(g)
    st.p[:] = (150.0 + 200.0 * rng.random(g.nc)) * decks.BAR
    smin = ref.sat_range_min(g, tp.twin_tables(), phases="wo")
    st = _finish(g, eq, st, smin, rng, 2)
    st.hc[:] = capi.HC_GAS_AND_OIL
    return g, tp.tables(), tp.twin_tables(), eq, 4, g.nconn, st


THREE_PHASE_CASES = [((5, 7, 9), False, 0.0), ((5, 7, 9), True, 0.0), ((9, 8, 9), False, 0.05), ((9, 8, 9), True, 0.05)]
OIL_WATER_CASES = [((5, 7, 9), False), ((5, 7, 9), True)]
_cache = {}


def reference(oracle, kind, case):
    """the case and the restatement's answer for it, computed once per session and shared: (case tuple, max_dp, dp_conn, details)"""
    key = (kind, case)
    if key not in _cache:
        if kind == "wog":
            c = three_phase(*case)
            g, t, eq, nreg, nface, st = c
            out = ref.compute_max_dp(oracle, g, t, st, eq, nreg, nface, details=True)
        else:
            c = oil_water(*case)
            g, _, twin, eq, nreg, nface, st = c
            out = ref.compute_max_dp(oracle, g, twin, st, eq, nreg, nface, phases="wo", details=True)
        for a in out[:2]:
            a.setflags(write=False)
        _cache[key] = (c,) + out
    return _cache[key]
