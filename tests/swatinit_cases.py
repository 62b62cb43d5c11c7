"""The fixtures of the SWATINIT GPU tests (tests/test_gpu_swatinit.py, tests/test_gpu_swatinit_dist.py and its worker): a 7 x 5 x 9 grid
-- 315 cells in the box: more than one 256-thread workgroup and no multiple of 64 -- with ACTNUM holes, two saturation regions with
DIFFERENT tables, per-cell end points and a PCW / PCG array, for the default and the Stone II three-phase model, and its oil-water
counterpart from tests/twophase.py; random imposed saturations and target capillary pressures for the setter."""
import numpy as np

from opmgpu import capi, decks

import twophase

DT = 2 * decks.DAY


def three_phase_tables(stone2=False):
    """the satfuncStandard tables twice; the second region's SWOF is squeezed in Sw and carries 0.6 of the capillary pressure"""
    extra = {"threephase_model": capi.KRO_STONE2} if stone2 else {}
    t = decks.satfunc_standard_tables(regions=2, **extra)
    a, b = t.swof_ptr[1], t.swof_ptr[2]
    t.swof_sw[a:b] = 0.12 + (t.swof_sw[a:b] - 0.1) * 0.95
    t.swof_pcow[a:b] *= 0.6
    return t


def grid(arrays=True, holes=True, seed=31):
    """arrays = False: the same cells and regions without end points and vertical maxima (a context created without any scaling);
    "eps": the end points only (what opmgpu.partition.LocalDomain carries to a rank)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    act = rng.random(7 * 5 * 9) > 0.2 if holes else None
    base = decks.cartesian_grid(7, 5, 9, lognormal_sigma=0.5, seed=seed, actnum=act)
    n = base.nc
    satnum = rng.integers(0, 2, n).astype(np.int32)
    eps = decks.random_endpoints(base, seed=seed + 1)
    eps["SWL"] = eps["SWL"] + 0.03 * satnum                    # (the second region's table starts at 0.12)
    eps["SWCR"] = np.maximum(eps["SWCR"], eps["SWL"])
    eps_v = {"PCW": rng.uniform(0.5, 2.0, n) * decks.BAR, "PCG": rng.uniform(1.0, 3.0, n) * decks.BAR}
    g = decks.GridData(n, base.conn_cells, base.trans, base.pv, base.z, gravity=base.gravity, satnum=satnum, dims=base.dims,
                       eps=eps if arrays else None, eps_v=eps_v if arrays is True else None)
    g.active_index = base.active_index
    return g


def with_pcw(g, pcw):
    """a copy of g whose PCW array is pcw (the other arrays as they are)"""
    ev = dict(g.eps_v or {})
    ev["PCW"] = np.array(pcw)
    eps = None if g.eps is None else {k: g.eps[i] for i, k in enumerate(g.EPS_NAMES)}
    return decks.GridData(g.nc, g.conn_cells, g.trans, g.pv, g.z, gravity=g.gravity, thpres=g.thpres, pvtnum=g.pvtnum, satnum=g.satnum,
                          dims=g.dims, eps=eps, scalecrs=g.scalecrs, eps_v=ev)


def case(kind):
    """kind: 'arrays' (default model, every array), 'plain' / 'stone2' / 'ow' (no scaling array at creation) -> grid, tables, state"""
    if kind == "ow":
        g, t = twophase.grid(7, 5, 9), twophase.tables(2)
        return g, t, twophase.state(g, seed=5)
    if kind == "ow_arrays":
        g, t = twophase.grid(7, 5, 9, endpoints=True, vertical=True), twophase.tables(2)
        return g, t, twophase.state(g, seed=5)
    g, t = grid(arrays=kind == "arrays"), three_phase_tables(stone2=kind == "stone2")
    return g, t, decks.random_state(g, t, seed=9)


def imposed(g, t, seed=17):
    """an imposed water saturation and a target pcow per cell: saturations over [0, 1] with some cells at exactly 0 (clamped to Swl) --
    for a table whose pcow ends at zero (the oil-water tables) only up to 0.8: at Swu such a curve is a rounding residue of the
    horizontal map, and the rule's test pc_at > 0 has no tolerance --, targets between -0.3 and 2 bar with some
    exact zeros"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = g.nc
    top = 0.8 if t.swof_pcow[t.swof_ptr[1:] - 1].min() == 0.0 else 1.0
    sw = top * rng.random(n)
    sw[rng.random(n) < 0.1] = 0.0
    pcow = rng.uniform(-0.3, 2.0, n) * decks.BAR
    pcow[rng.random(n) < 0.05] = 0.0
    return sw, pcow


def wells(g):
    """a well pattern for the re-plan (host wells: clique fill in the matrix, another internal numbering)"""
    n = g.nc
    return np.array([0, 3, 5], np.int32), np.array([7, n // 3, n // 2, n - 40, n - 9], np.int32)
