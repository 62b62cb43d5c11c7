"""numpy restatement of the PVCDO rule (include/opmgpu.h at opmgpu_set_pvcdo), the yardstick of the PVCDO tests.  Written from the
formulas, not from the device code.  Per PVT region one row (p_ref, B_ref, C_o, mu_ref, C_v), SI:

    X = C_o (p - p_ref)             1 / B_o        = (1 + X (1 + X / 2)) / B_ref
    Y = (C_o - C_v) (p - p_ref)     1 / (B_o mu_o) = (1 + Y (1 + Y / 2)) / (B_ref mu_ref)

Every function takes a row (or an [n][5] array of rows, one per pressure) and pressures, real or complex (the complex-step check of the
derivatives), and returns (value, d value / d p)."""
import numpy as np

BAR, CP = 1.0e5, 1.0e-3


def si(rows):
    """PVCDO rows in deck units (bar, -, 1/bar, cP, 1/bar) -> SI"""
    o = np.array(rows, float).reshape(-1, 5)
    o[:, 0] *= BAR; o[:, 2] /= BAR; o[:, 3] *= CP; o[:, 4] /= BAR
    return o


def _cols(row):
    r = np.asarray(row, float)
    return r[..., 0], r[..., 1], r[..., 2], r[..., 3], r[..., 4]


def inv_b(row, p):
    pref, bref, co, _, _ = _cols(row)
    x = co * (p - pref)
    return (1.0 + x * (1.0 + x / 2.0)) / bref, co * (1.0 + x) / bref


def inv_bmu(row, p):
    pref, bref, co, muref, cv = _cols(row)
    c = co - cv
    y = c * (p - pref)
    return (1.0 + y * (1.0 + y / 2.0)) / (bref * muref), c * (1.0 + y) / (bref * muref)


def viscosity(row, p):
    """mu_o = (1 / B_o) / (1 / (B_o mu_o)) and its derivative (quotient rule)"""
    b, db = inv_b(row, p)
    bm, dbm = inv_bmu(row, p)
    mu = b / bm
    return mu, (db - mu * dbm) / bm


def rows_of(rows, pvtnum):
    """the row of every cell: rows [n_pvt][5], pvtnum [n] (0-based)"""
    return np.asarray(rows, float).reshape(-1, 5)[np.asarray(pvtnum, int)]
