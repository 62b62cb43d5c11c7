"""Oil-water decks (no gas phase) and their three-phase TWINS, the yardstick of the two-phase tests.

The twin of a two-phase deck is a three-phase deck the unchanged CPU oracle can evaluate: the same water / oil tables plus a dummy gas --
SGOF [(0, 0, krocw, 0), (1 - Swco, 0, 0, 0)] per region (krg = 0, pcgo = 0, krog(0) = krow(Swco)), any smooth PVDG, any gas density,
DISGAS = VAPOIL off -- and a state with Sg = 0, hc = GAS_AND_OIL.  With krg = 0 and Sg = 0 the twin's gas equation is empty and its
water / oil equations do not see the gas tables, as long as Sw >= Swco + 1e-3 (closer to Swco the default three-phase law blends krow
with krog: test_twophase_twin.py pins all of this on the oracle itself).  Restricted to water and oil, the oracle on the twin is the
expected answer of the two-phase code.
"""
import numpy as np

from opmgpu import capi, decks

# two saturation regions with different connate water, critical saturations, maxima and capillary pressure [bar]
SWOF = [
    [(0.1, 0.0, 1.0, 0.9), (0.2, 0.0, 0.8, 0.8), (0.3, 0.1, 0.6, 0.7), (0.4, 0.2, 0.4, 0.6), (0.7, 0.5, 0.1, 0.3), (0.8, 0.6, 0.0, 0.2),
     (0.9, 0.7, 0.0, 0.1)],
    [(0.15, 0.0, 0.9, 0.5), (0.3, 0.05, 0.55, 0.3), (0.5, 0.2, 0.25, 0.15), (0.75, 0.5, 0.0, 0.05), (1.0, 1.0, 0.0, 0.0)],
]
# PVDO rows (p [bar], Bo, mu [cP]) of two PVT regions, PVTW, surface densities (water, oil)
PVDO = [
    [(1.0, 1.062, 1.00), (100.0, 1.045, 1.08), (200.0, 1.030, 1.17), (400.0, 1.004, 1.37), (600.0, 0.982, 1.60)],
    [(1.0, 1.120, 2.00), (150.0, 1.090, 2.20), (300.0, 1.065, 2.45), (600.0, 1.030, 3.00)],
]
PVTW = [[200.0, 1.02, 4.0e-5, 0.50, 1.0e-4], [250.0, 1.01, 4.5e-5, 0.45, 0.0]]
DENSITY_WO = [[1030.0, 820.0], [1010.0, 870.0]]
ROCK = (200.0, 5.0e-5)
# dummy gases of the twin: (PVDG rows (p, Bg, mu), surface density).  Completely different on purpose.
GASES = [
    ([(1.0, 1.0, 0.012), (100.0, 0.011, 0.016), (400.0, 0.0031, 0.028), (800.0, 0.0019, 0.040)], 0.9),
    ([(1.0, 0.7, 0.100), (300.0, 0.020, 0.300), (900.0, 0.0100, 0.900)], 55.0),
]


def _dead_oil(rows):
    return [(0.0, [r]) for r in rows]


def tables(regions=2, pc_scale=1.0):
    """the two-phase tables: `regions` saturation and PVT regions (1 or 2)"""
    swof = [[(a, b, c, d * pc_scale) for a, b, c, d in t] for t in SWOF[:regions]]
    return decks.FluidTables(density_wog=DENSITY_WO[:regions], pvtw=PVTW[:regions], pvto=[_dead_oil(r) for r in PVDO[:regions]], pvtg=None,
                             swof=swof, sgof=None, rock=ROCK, phases="wo")


def twin_tables(regions=2, pc_scale=1.0, gas=0):
    """the three-phase twin of tables(regions, pc_scale) with dummy gas number `gas`"""
    swof = [[(a, b, c, d * pc_scale) for a, b, c, d in t] for t in SWOF[:regions]]
    sgof = [[(0.0, 0.0, t[0][2], 0.0), (1.0 - t[0][0], 0.0, 0.0, 0.0)] for t in swof]
    pvdg, rho_g = GASES[gas]
    return decks.FluidTables(density_wog=[d + [rho_g] for d in DENSITY_WO[:regions]], pvtw=PVTW[:regions],
                             pvto=[_dead_oil(r) for r in PVDO[:regions]], pvtg=[[(p, [(0.0, B, mu)]) for p, B, mu in pvdg]] * regions,
                             swof=swof, sgof=sgof, rock=ROCK, disgas=False, vapoil=False)


def grid(nx, ny, nz, regions=2, seed=3, endpoints=False, vertical=False, scalecrs=False, thpres=False, pvt_regions=None):
    """Cartesian grid with lognormal permeability, random SATNUM / PVTNUM and, on request, per-cell end points (+ KRW / KRO / PCW
    maxima, three-point scaling) and threshold pressures.  The same object serves the two-phase model and the oracle on the twin: its gas
    end points are the twin's (SGL = SGCR = 0, SGU = 1 - SWL, SOGCR = SOWCR), which the two-phase code does not read.  pvt_regions = 1:
    every cell in the first PVT region (the host well model of the oracle side takes ONE set of surface densities)."""
    g = decks.cartesian_grid(nx, ny, nz, lognormal_sigma=0.8, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 100))
    n = g.nc
    satnum = rng.integers(0, regions, n).astype(np.int32)
    pvtnum = rng.integers(0, regions if pvt_regions is None else pvt_regions, n).astype(np.int32)
    th = 0.3 * decks.BAR * rng.random(g.nconn) if thpres else None
    eps, eps_v = None, None
    if endpoints:
        swco = np.array([SWOF[r][0][0] for r in satnum])
        swl = swco + 0.04 * (rng.random(n) - 0.5)
        swcr = swl + 0.08 + 0.04 * rng.random(n)
        sowcr = 0.15 + 0.1 * rng.random(n)
        swu = 0.92 + 0.06 * rng.random(n)
        eps = {"SWL": swl, "SWCR": swcr, "SWU": swu, "SOWCR": sowcr, "SGL": np.zeros(n), "SGCR": np.zeros(n), "SGU": 1.0 - swl, "SOGCR": sowcr}
    if vertical:
        eps_v = {"KRW": 0.6 + 0.3 * rng.random(n), "KRO": 0.7 + 0.3 * rng.random(n), "PCW": (0.4 + 0.8 * rng.random(n)) * decks.BAR}
    return decks.GridData(g.nc, g.conn_cells, g.trans, g.pv, g.z, gravity=g.gravity, thpres=th, pvtnum=pvtnum, satnum=satnum, dims=g.dims,
                          eps=eps, scalecrs=scalecrs, eps_v=eps_v)


def connate(g):
    """connate water saturation of every cell: its scaled SWL, else the first Sw node of its region's SWOF"""
    if g.eps is not None:
        return np.asarray(g.eps[0])
    sn = np.zeros(g.nc, int) if g.satnum is None else g.satnum
    return np.array([SWOF[r][0][0] for r in sn])


def state(g, seed=11, margin=1e-3):
    """random pressures and water saturations with Sw >= Swco + margin (the twin's range of validity), Sg = rs = rv = 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = g.nc
    p = (150.0 + 200.0 * rng.random(n)) * decks.BAR
    lo = connate(g) + margin
    sw = lo + (0.97 - lo) * rng.random(n)
    k = rng.random(n) < 0.1                      # some cells on table nodes
    nodes = np.array([0.2, 0.3, 0.4, 0.5, 0.7, 0.75, 0.8, 0.9])
    sw[k] = np.maximum(rng.choice(nodes, k.sum()), lo[k])
    sat = np.stack([sw, 1.0 - sw, np.zeros(n)], 1)
    return decks.State(p, sat, np.zeros(n), np.zeros(n), np.full(n, capi.HC_GAS_AND_OIL, np.int8))


# ------------------------------------------------------------------------------------------------------------------------------------------
# the golden oil-water deck and its three-phase twin deck
# ------------------------------------------------------------------------------------------------------------------------------------------
import os  # noqa: E402

DECK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decks", "OILWATER_SMALL.DATA")


def deck_text():
    return open(DECK).read()


def write_deck(path, text):
    with open(str(path), "w") as f:
        f.write(text)
    return str(path)


def _per_cell(values):
    return " ".join("%.17g" % v for v in values)


def twin_deck_text(gas=0):
    """the three-phase twin of the golden deck: GAS in RUNSPEC, the dummy SGOF and PVDG, a gas density, and the twin's gas end points
    (SGL = SGCR = 0, SGU = 1 - SWL, SOGCR = SOWCR) per cell"""
    from opmgpu import deck as deckmod
    d = deckmod.read_deck(DECK)
    t = d.tables()
    pvdg, rho_g = GASES[gas]
    sgof = ""
    for r in range(t.n_sat):
        a = t.swof_ptr[r]
        sgof += " 0.0 0.0 %.17g 0.0\n %.17g 0.0 0.0 0.0\n/\n" % (t.swof_krow[a], 1.0 - t.swof_sw[a])
    nx, ny, nz = d.dims
    n = nx * ny * nz
    swl, sowcr = d.array("SWL", n), d.array("SOWCR", n)
    ends = "SGL\n %d*0 /\nSGCR\n %d*0 /\nSGU\n %s /\nSOGCR\n %s /\n" % (n, n, _per_cell(1.0 - swl), _per_cell(sowcr))
    text = deck_text()
    text = text.replace("\nWATER\n", "\nWATER\nGAS\n", 1)
    text = text.replace("\nDENSITY\n 820 1030 /\n", "\nDENSITY\n 820 1030 %.17g /\n" % rho_g, 1)
    text = text.replace("\nREGIONS\n", "\nSGOF\n" + sgof + "PVDG\n" + "\n".join(" %.17g %.17g %.17g" % row for row in pvdg) + " /\n" + ends + "REGIONS\n", 1)
    assert "GAS" in text and "SGOF" in text and "PVDG" in text and " %.17g /" % rho_g in text
    return text
