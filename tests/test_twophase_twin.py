"""The yardstick of the oil-water tests, pinned on the CPU oracle itself (tests/twophase.py): the three-phase twin of a two-phase deck has
an empty gas equation, and its water / oil equations do not depend on the dummy gas for Sw >= Swco + 1e-3.  Two twins whose gas tables
differ completely must therefore agree BIT FOR BIT in everything that concerns water and oil.  This guards the yardstick, not the feature."""
import numpy as np
import pytest

import twophase as tp


@pytest.mark.parametrize("endpoints", [False, True])
def test_twin_water_oil_part_is_independent_of_the_dummy_gas(oracle, endpoints):
    g = tp.grid(5, 4, 3, endpoints=endpoints, vertical=endpoints)
    st = tp.state(g)
    rowptr, col = oracle.pattern(g)
    dt = 5 * 86400.0
    out = []
    for gas in (0, 1):
        t = tp.twin_tables(gas=gas)
        r, val, acc, binv = oracle.assemble(g, t, dt, st, rowptr, col, scale=(1.1169, 1.0031, 0.0031))
        out.append((r, val.reshape(-1, 3, 3), oracle.cell_props(g, t, st)))
    nc = g.nc
    rows = np.repeat(np.arange(nc), np.diff(rowptr))
    for r, val, props in out:
        assert np.all(r[2 * nc:] == 0.0)                                    # empty gas residual
        assert np.all(val[:, 2, :2] == 0.0)                                 # the gas rows: no p / Sw entries ...
        assert np.all(val[rows != col][:, 2, :] == 0.0)                     # ... and no off-diagonal ones
        nm = oracle.PROP_NAMES
        assert np.all(props[:, nm.index("kr_g"), 0] == 0.0) and np.all(props[:, nm.index("mob_g"), 0] == 0.0)
    (r0, v0, p0), (r1, v1, p1) = out
    assert np.array_equal(r0[:2 * nc], r1[:2 * nc])
    assert np.array_equal(v0[:, :2, :2], v1[:, :2, :2])
    for name in ("p_w", "b_w", "b_o", "mu_w", "mu_o", "kr_w", "kr_o", "rho_w", "rho_o", "mob_w", "mob_o", "accum_w", "accum_o"):
        k = oracle.PROP_NAMES.index(name)
        assert np.array_equal(p0[:, k, :3], p1[:, k, :3]), name


def test_twin_kro_is_the_krow_column_away_from_connate_water(oracle):
    """kro of the twin = krow(Sw) of the SWOF table (what the two-phase law states), to rounding"""
    g = tp.grid(5, 4, 3)
    st = tp.state(g)
    kro = oracle.cell_props(g, tp.twin_tables(), st)[:, oracle.PROP_NAMES.index("kr_o"), 0]
    ref = np.empty(g.nc)
    for c in range(g.nc):
        t = np.array(tp.SWOF[g.satnum[c]])
        ref[c] = np.interp(st.sat[c, 0], t[:, 0], t[:, 2])
    assert np.allclose(kro, ref, rtol=1e-11, atol=1e-13)
