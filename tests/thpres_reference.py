"""numpy restatement of the reference's threshold-pressure set-up, the yardstick of the THPRES tests:

    compute_max_dp        computeMaxDp            opm/simulators/thresholdPressures.hpp:46-298
    threshold_pressures   thresholdPressures      ibid. :320-369   (grid faces)
                          thresholdPressuresNNC   ibid. :383-417   (NNCs)

Written from those lines.  What it takes from the unchanged CPU oracle (oracle.cell_props / oracle.pvt) are the table evaluations only:
p_w, p_g, b_w(p_w), RsSat(p_o), RvSat(p_g) and the saturated / undersaturated b_o, b_g.  computeMaxDp chooses the PVT branch per phase
by Rs >= RsSat and Rv >= RvSat, not by the hydrocarbon state, so the oracle is evaluated with the hc that selects the wanted branch:

    hc = GAS_AND_OIL  sg = the state's Sg -> p_w, p_g; rs = RsSat(p_o), rv = RvSat(p_g); the SATURATED b_o(p_o) and b_g(p_g); b_w(p_w)
    hc = OIL_ONLY     the UNDERSATURATED b_o(p_o, Rs) at the state's Rs
    the UNDERSATURATED b_g(p_g, Rv): oracle.pvt at the p_g of the first evaluation -- cell_props with hc = GAS_ONLY takes Sg = 1 - Sw, so
                      its p_g is the state's only where So = 0

Everything else is done here: the densities with the state's Rs / Rv, satRange (SaturationPropsFromDeck.cpp:212-250), the per-face rule
and the maxima per pair of regions.  No VAPPARS (the oracle's rs / rv would carry its factor; computeMaxDp's RsSat / RvSat do not).

phases = "wo": a deck without a gas phase.  The oracle is then evaluated on the deck's three-phase TWIN (tests/twophase.py); the loop runs
over water and oil and satRange's oil minimum is 1 - SWU, as the reference's two-phase branch has it (the twin's SGU is no end point of
the deck).
"""
import numpy as np

from opmgpu import capi
from opmgpu.decks import State

P_W, P_G, B_W, B_O, B_G, RS, RV = 0, 2, 3, 4, 5, 18, 19       # slots of oracle.cell_props


def sat_range_min(grid, tables, phases="wog"):
    """smin of satRange, [nc][3] (water, oil, gas): the cell's scaled SWL / SGL, else the first node of its region's table; oil
    max(0, 1 - SWU - SGU), with two phases max(0, 1 - SWU)"""
    sn = np.zeros(grid.nc, int) if grid.satnum is None else np.asarray(grid.satnum, int)
    t = tables

    def point(k, x, ptr, last):
        if grid.eps is not None:
            return np.asarray(grid.eps[k])
        return x[ptr[sn + 1] - 1] if last else x[ptr[sn]]
    swl, swu = point(0, t.swof_sw, t.swof_ptr, False), point(2, t.swof_sw, t.swof_ptr, True)
    smin = np.zeros((grid.nc, 3))
    smin[:, 0] = swl
    so = 1.0 - swu
    if phases == "wog":
        smin[:, 2] = point(4, t.sgof_sg, t.sgof_ptr, False)
        so = so - point(6, t.sgof_sg, t.sgof_ptr, True)
    smin[:, 1] = np.maximum(0.0, so)
    return smin


def phase_quantities(oracle, grid, tables, st, phases="wog"):
    """(pressure, density, saturation) of the phases, each [nc][3] (water, oil, gas), by the rules of thresholdPressures.hpp:109-248"""
    assert tables.vap1 == 0.0 and tables.vap2 == 0.0, "no VAPPARS here"
    n = grid.nc
    pvtnum = np.zeros(n, np.int32) if grid.pvtnum is None else grid.pvtnum
    rhos = tables.surface_density[np.asarray(pvtnum, int)]
    A = oracle.cell_props(grid, tables, State(st.p, st.sat, st.rs, st.rv, np.full(n, capi.HC_GAS_AND_OIL, np.int8)))[:, :, 0]
    B = oracle.cell_props(grid, tables, State(st.p, st.sat, st.rs, st.rv, np.full(n, capi.HC_OIL_ONLY, np.int8)))[:, :, 0]
    p = np.stack([A[:, P_W], st.p, A[:, P_G]], 1)
    rs_sat = A[:, RS] if tables.has_disgas else np.zeros(n)
    rv_sat = A[:, RV] if tables.has_vapoil else np.zeros(n)
    b_o = np.where(st.rs >= rs_sat, A[:, B_O], B[:, B_O])
    b_g_under = oracle.pvt(tables, "bGas", p[:, 2], r=st.rv, saturated=np.zeros(n, np.int8), pvtnum=capi.i32(pvtnum))[:, 0]
    b_g = np.where(st.rv >= rv_sat, A[:, B_G], b_g_under)
    rho = np.zeros((n, 3))
    rho[:, 0] = rhos[:, 0] * A[:, B_W]
    rho[:, 1] = rhos[:, 1] * b_o + rhos[:, 2] * st.rs * b_o
    rho[:, 2] = rhos[:, 2] * b_g + rhos[:, 1] * st.rv * b_g
    s = np.array(st.sat, float)
    if phases == "wo":
        p[:, 2], rho[:, 2], s[:, 2] = st.p, 0.0, 0.0
        rho[:, 1] = rhos[:, 1] * b_o
    return p, rho, s


def face_potentials(grid, p, rho, n_face_conn):
    """p1, p2 of every face connection and phase, [n_face_conn][3] each (thresholdPressures.hpp:279-292)"""
    c = grid.conn_cells[:n_face_conn]
    c1, c2 = c[:, 0], c[:, 1]
    rho_avg = (rho[c1] + rho[c2]) / 2
    dz = grid.z[c1] - grid.z[c2]
    return p[c1], p[c2] + rho_avg * grid.gravity * dz[:, None]


def compute_max_dp(oracle, grid, tables, st, eqlnum, nregions, n_face_conn, phases="wog", details=False):
    """-> (max_dp [nregions][nregions], dp_conn [nconn]).  max_dp is symmetric, -1.0 where no face connection joins the pair (the
    reference's "pair absent from the map"), 0.0 for a present pair whose phases never count; dp_conn is 0 on connections within one
    region, where no phase counts and on the NNCs (f >= n_face_conn: the reference scans the grid's faces only).
    details=True adds a dict with the face potentials and the saturations the conditioning check of the tests needs."""
    eq = np.asarray(eqlnum, int)
    p, rho, s = phase_quantities(oracle, grid, tables, st, phases)
    smin = sat_range_min(grid, tables, phases)
    p1, p2 = face_potentials(grid, p, rho, n_face_conn)
    c = grid.conn_cells[:n_face_conn]
    c1, c2 = c[:, 0], c[:, 1]
    nph = 2 if phases == "wo" else 3
    counts = ((p1 > p2) & (s[c1] > smin[c1])) | ((p2 > p1) & (s[c2] > smin[c2]))
    counts[:, nph:] = False
    barrier = eq[c1] != eq[c2]
    dp_face = np.where(counts, np.abs(p1 - p2), 0.0).max(axis=1)
    dp_face = np.where(barrier, dp_face, 0.0)
    dp_conn = np.zeros(grid.nconn)
    dp_conn[:n_face_conn] = dp_face
    max_dp = np.full((nregions, nregions), -1.0)
    for f in np.flatnonzero(barrier):
        a, b = eq[c1[f]] - 1, eq[c2[f]] - 1
        max_dp[a, b] = max_dp[b, a] = max(max_dp[a, b], 0.0, dp_face[f])
    if details:
        return max_dp, dp_conn, dict(p1=p1, p2=p2, barrier=barrier, s=s, smin=smin, nph=nph)
    return max_dp, dp_conn


def well_conditioned(details, dp_tie=1e-3, s_tie=1e-9):
    """The strict tests of the per-face rule must not hinge on rounding: no barrier face with 0 < |p1 - p2| < dp_tie [Pa] in an active
    phase, and no saturation within s_tie of its residual value without being bitwise equal to it.  -> list of complaints (empty: fine)"""
    d, bad = details, []
    gap = np.abs(d["p1"] - d["p2"])[d["barrier"]][:, :d["nph"]]
    if ((gap > 0.0) & (gap < dp_tie)).any():
        bad.append("a barrier face with 0 < |p1 - p2| < %g Pa" % dp_tie)
    ds = np.abs(d["s"] - d["smin"])[:, :d["nph"]]
    if ((ds > 0.0) & (ds < s_tie)).any():
        bad.append("a saturation within %g of its residual value, but not equal to it" % s_tie)
    return bad


def threshold_pressures(grid, eqlnum, barriers, max_dp, n_face_conn):
    """thresholdPressures + thresholdPressuresNNC: [nconn].  barriers = {(r1, r2) with r1 < r2: value or None (defaulted)}; max_dp the
    table of compute_max_dp.  A face of a defaulted barrier whose pair is absent takes 0; an NNC there raises KeyError like the
    reference's maxDp.at() (with the pair ordered, where the reference looks it up as given)."""
    eq = np.asarray(eqlnum, int)
    out = np.zeros(grid.nconn)
    for f in range(grid.nconn):
        e1, e2 = eq[grid.conn_cells[f, 0]], eq[grid.conn_cells[f, 1]]
        key = (min(e1, e2), max(e1, e2))
        if key not in barriers:
            continue
        if barriers[key] is not None:
            out[f] = barriers[key]
            continue
        present = max_dp[key[0] - 1, key[1] - 1] >= 0.0
        if f < n_face_conn:
            out[f] = max_dp[key[0] - 1, key[1] - 1] if present else 0.0
        else:
            if not present:
                raise KeyError(key)
            out[f] = max_dp[key[0] - 1, key[1] - 1]
    return out
