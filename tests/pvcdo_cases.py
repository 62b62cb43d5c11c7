"""The cases of the PVCDO tests: their PVCDO rows, their tables in the three forms (default three-phase law, Stone II, oil-water), their
states, and their dense-PVDO TWINS with the bounds of the twins' error.

The twin of a case is the same deck with the oil given as a PVDO table that samples the rule (tests/pvcdo_reference.py) every H = 0.25 bar
from 1 to 801 bar: something the unchanged CPU oracle, and the device's tabulated path, can evaluate.  An oil-water case's twin also takes
the dummy gas of tests/twophase.py.  The tables are piecewise linear in 1 / B and 1 / (B mu), the rule is quadratic in p with second
derivative c^2 / (B_ref ...), so with c = max(C_o, |C_o - C_v|) over the case's regions the twin differs from the rule by at most
    values  (H c)^2 / 8                                   of the polynomial 1 + Y (1 + Y / 2) (linear interpolation of a quadratic over a
                                                          segment of width H); see value_bound_relative for the relative figure,
    slopes  (H c / 2) / (1 - c max |p - p_ref|)            relative (a chord's slope against the tangent's, over the smallest slope).
Nothing here is measured on the code under test."""
import numpy as np

from opmgpu import capi, decks

import pvcdo_reference as ref
import twophase as tp

H = 0.25                                        # bar: spacing of the twin's PVDO nodes
P_LO, P_HI = 50.0, 600.0                        # bar: every pressure of every state lies inside
# (p_ref [bar], B_ref, C_o [1/bar], mu_ref [cP], C_v [1/bar]) of the two PVT regions; C_o <= 1.5e-4 / bar, C_v <= 6e-4 / bar
ROWS = [(230.0, 1.045, 1.2e-4, 1.20, 5.0e-4), (280.0, 1.090, 1.5e-4, 2.30, 6.0e-4)]
FORMS = ("default", "stone2", "ow")
PVTW = [[200.0, 1.02, 4.0e-5, 0.50, 1.0e-4], [250.0, 1.01, 4.5e-5, 0.45, 0.0]]
DENSITY_WO = [[1030.0, 820.0], [1010.0, 870.0]]
ROCK = (200.0, 5.0e-5)
SWOF3 = [(0.1, 0.0, 1.0, 0.9), (0.2, 0.0, 0.8, 0.8), (0.3, 0.1, 0.6, 0.7), (0.4, 0.2, 0.4, 0.6), (0.7, 0.5, 0.1, 0.3), (0.8, 0.6, 0.0, 0.2),
         (0.9, 0.7, 0.0, 0.1)]
SGOF3 = [(0.0, 0.0, 1.0, 0.2), (0.1, 0.0, 0.7, 0.4), (0.2, 0.1, 0.6, 0.6), (0.8, 0.7, 0.0, 2.0), (0.9, 1.0, 0.0, 2.1)]


def rows_si(regions=2):
    return ref.si(ROWS[:regions])


def c_max(regions=2):
    """c = max(C_o, |C_o - C_v|) over the regions [1 / bar]"""
    return max(max(r[2], abs(r[2] - r[4])) for r in ROWS[:regions])


def value_bound(regions=2):
    return (H * c_max(regions)) ** 2 / 8.0


def _reach(regions=2):
    """max |p - p_ref| over the regions and the pressure range [bar]"""
    return max(max(abs(P_LO - r[0]), abs(P_HI - r[0])) for r in ROWS[:regions])


def value_bound_relative(regions=2):
    """(H c)^2 / 8 is the ABSOLUTE error of the interpolated polynomial 1 + Y (1 + Y / 2); relative to the polynomial's value, which is
    below 1 on the side of p_ref where Y < 0 but never below 1 - c max |p - p_ref|, it is this.  What test_pvcdo_reference.py holds the twin
    to; the tolerances of the GPU tests are 10 x value_bound(), which covers the factor (1.2 here)."""
    return value_bound(regions) / (1.0 - c_max(regions) * _reach(regions))


def slope_bound(regions=2):
    c = c_max(regions)
    return (H * c / 2.0) / (1.0 - c * _reach(regions))


def tol_value(regions=2):
    """what the tests ADD to the tolerance an existing test uses for a tabulated oil, where VALUES are compared"""
    return 10.0 * value_bound(regions)


def tol_slope(regions=2):
    """... and where SLOPES enter (Jacobian blocks, what follows from a linear solve)"""
    return 2.0 * slope_bound(regions)


def dense_pvdo(row):
    """PVDO rows (p [bar], B_o, mu_o [cP]) sampling the rule of `row` (deck units) every H from 1 to 801 bar"""
    o = ref.si([row])[0]
    p = 1.0 + H * np.arange(int(round(800.0 / H)) + 1)
    ib, _ = ref.inv_b(o, p * ref.BAR)
    mu, _ = ref.viscosity(o, p * ref.BAR)
    return list(zip(p.tolist(), (1.0 / ib).tolist(), (mu / ref.CP).tolist()))


def _dead(rows):
    return [(0.0, [r]) for r in rows]


_CACHE = {}


def tables(form, regions=2):
    """(the tables with the analytic oil, their dense twin) of a form; built once and shared"""
    key = (form, regions)
    if key not in _CACHE:
        dense = [_dead(dense_pvdo(r)) for r in ROWS[:regions]]
        rows = [list(r) for r in ROWS[:regions]]
        if form == "ow":
            swof = tp.SWOF[:regions]
            sgof = [[(0.0, 0.0, t[0][2], 0.0), (1.0 - t[0][0], 0.0, 0.0, 0.0)] for t in swof]         # the twin's dummy gas (tests/twophase.py)
            pvdg, rho_g = tp.GASES[0]
            own = decks.FluidTables(density_wog=DENSITY_WO[:regions], pvtw=PVTW[:regions], pvto=None, pvtg=None, swof=swof, sgof=None, rock=ROCK,
                                    phases="wo", pvcdo=rows)
            twin = decks.FluidTables(density_wog=[d + [rho_g] for d in DENSITY_WO[:regions]], pvtw=PVTW[:regions], pvto=dense,
                                     pvtg=[[(p, [(0.0, B, mu)]) for p, B, mu in pvdg]] * regions, swof=swof, sgof=sgof, rock=ROCK,
                                     disgas=False, vapoil=False)
        else:
            model = capi.KRO_STONE2 if form == "stone2" else capi.KRO_DEFAULT
            gas = [[(p, [(0.0, B, mu)]) for p, B, mu in tp.GASES[r][0]] for r in range(regions)]
            common = dict(density_wog=[DENSITY_WO[r] + [tp.GASES[r][1]] for r in range(regions)], pvtw=PVTW[:regions], pvtg=gas,
                          swof=[SWOF3] * regions, sgof=[SGOF3] * regions, rock=ROCK, disgas=False, vapoil=False, threephase_model=model)
            own = decks.FluidTables(pvto=None, pvcdo=rows, **common)
            twin = decks.FluidTables(pvto=dense, **common)
        _CACHE[key] = (own, twin)
    return _CACHE[key]


def grid(pvt_regions=2, seed=3):
    """5 x 7 x 9 cells (315: the last wave is partial) with random SATNUM and PVTNUM over two regions"""
    return tp.grid(5, 7, 9, seed=seed, pvt_regions=pvt_regions)


def state(g, form, seed=11):
    """a random state with every pressure inside [P_LO, P_HI] bar and, in each PVT region, pressures on both sides of its p_ref"""
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    n = g.nc
    st = tp.state(g, seed=seed)                 # Sw >= Swco + 1e-3 (the oil-water twin's range of validity), Sg = rs = rv = 0
    p = (P_LO + 5.0 + (P_HI - P_LO - 10.0) * rng.random(n)) * decks.BAR
    if form != "ow":
        sw = 0.12 + 0.5 * rng.random(n)
        sg = 0.02 + 0.3 * rng.random(n)
        sat = np.stack([sw, 1.0 - sw - sg, sg], 1)
        st = decks.State(p, sat, np.zeros(n), np.zeros(n), np.full(n, capi.HC_GAS_AND_OIL, np.int8))
    else:
        st = decks.State(p, st.sat, st.rs, st.rv, st.hc)
    return _checked(g, st)


def _checked(g, st):
    for r, row in enumerate(ROWS):
        k = g.pvtnum == r
        if k.any():
            assert (st.p[k] < row[0] * decks.BAR).any() and (st.p[k] > row[0] * decks.BAR).any()
    assert st.p.min() >= P_LO * decks.BAR and st.p.max() <= P_HI * decks.BAR
    return st


def smooth_state(g, form, seed=11):
    """the state of the Newton lockstep: state()'s saturations with a pressure field that varies smoothly around the two reference pressures
    (random pressures over 550 bar between neighbours are no reservoir state: the first Newton update of such a field is chopped)"""
    st = state(g, form, seed)
    nx, ny, nz = g.dims
    i, j, k = np.unravel_index(np.arange(g.nc), (nz, ny, nx))[::-1]
    p = (200.0 + 120.0 * i / (nx - 1) + 10.0 * j / (ny - 1)) * decks.BAR + g.z * 0.0
    return _checked(g, decks.State(p + 800.0 * 9.81 * (g.z - g.z.min()), st.sat, st.rs, st.rv, st.hc))
