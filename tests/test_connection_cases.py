"""The connection edge cases (connection_edge_cases.py) on the CPU: the condition on the inputs for every (connection, phase), the census of
the fixture, and the controls that show that every tie and threshold case discriminates.  No GPU: the oracle's cell values and assembly."""
import numpy as np
import pytest

import connection_edge_cases as K
from opmgpu import capi, decks

DT = 3 * decks.DAY
SEEDS = (1, 2)            # the two states the device tests assemble
ORDERINGS = {"natural": capi.ORDER_NATURAL, "multicolour": capi.ORDER_MULTICOLOR}


def _deck(kind, variant):
    g = K.grid(variant)
    return g, (K.tables() if kind == "wog" else K.twin_wo())


@pytest.mark.parametrize("variant", K.VARIANTS)
@pytest.mark.parametrize("kind", ["wog", "wo"])
def test_every_connection_and_phase_is_exact_or_far(oracle, kind, variant):
    """the condition of the fixture's docstring, none left out; and what 'exact' promises: phase pressures equal bit for bit at a tie"""
    g, tab = _deck(kind, variant)
    nph = 3 if kind == "wog" else 2
    for seed in SEEDS:
        st = K.state(seed, kind)
        cv = K.connection_values(g, oracle.cell_props(g, tab, st))
        exact = K.exact_by_construction(g, st, nph)
        far = np.abs(cv["dh0"]) >= K.FAR * cv["psum"]
        if g.thpres is not None:
            far &= np.abs(np.abs(cv["dh0"]) - g.thpres[:, None]) >= K.FAR * cv["psum"]
        ok = (exact | far)[:, :nph]
        bad = np.argwhere(~ok)
        assert bad.size == 0, [(int(f), "wog"[a], K.fixture().case[f], cv["dh0"][f, a], cv["psum"][f, a]) for f, a in bad[:10]]
        # exact means exact: with g dz == 0 the oracle's head difference IS the subtraction of the two state pressures where p_a = p,
        # and 0 where the capillary pressure comes from equal inputs
        c1, c2 = g.conn_cells[:, 0], g.conn_cells[:, 1]
        dp = (st.p[c1] - st.p[c2])[:, None]
        assert np.array_equal(cv["dh0"][exact], np.broadcast_to(dp, exact.shape)[exact])
        worst = (cv["psum"] / np.maximum(np.abs(cv["dh0"]), 1e-300))[:, :nph][~exact[:, :nph] & ok]
        print("%s %s state %d: %d exact and %d far (connection, phase) pairs; largest (|p1| + |p2|) / |dh| of a far one %.1f" %
              (kind, variant, seed, exact[:, :nph].sum(), (~exact[:, :nph]).sum(), worst.max()))
        for name in K.TIES:
            f = K.cases(name)
            phases = [1] if name == "oil tie" else list(range(nph))
            assert np.all(cv["dh0"][f][:, phases] == 0.0) and np.all(cv["up"][f][:, phases] == 0), name
        if variant != "nothp":
            f = np.concatenate([K.cases(n) for n in K.AT_THP])
            assert np.all(np.abs(cv["dh0"][f, 1]) == g.thpres[f]) and np.all(cv["dh"][f, 1] == 0.0) and np.all(cv["open"][f, 1])
            assert set(np.sign(cv["dh0"][f, 1])) == {-1.0, 1.0}
            f = K.cases("one float below")
            assert not cv["open"][f, 1].any() and set(np.sign(cv["dh0"][f, 1])) == {-1.0, 1.0}
            assert np.all(np.nextafter(g.thpres[f], 0.0) == np.abs(cv["dh0"][f, 1]))
            f = K.cases("one float above")
            assert cv["open"][f, 1].all() and np.all(cv["dh"][f, 1] != 0.0) and set(cv["up"][f, 1]) == {0, 1}


def test_census(oracle):
    """every row of the issue's table is present, ascending and descending in caller numbering, inside one 256-row chunk and across two
    in both orderings; the U ratios at the ties; the hub's slice; the kinds of diagonal position among the named cells"""
    F = K.fixture()
    g, tab = _deck("wog", "base")
    rowptr, col = oracle.pattern(g)
    c1, c2 = F.conn[:, 0], F.conn[:, 1]
    assert 500 <= g.nc <= 700 and -(-g.nc // K.CHUNK) == 3 and g.nc % K.CHUNK != 0 and g.nc % 64 != 0
    asc = c1 < c2
    pos = {o: K.plan_position(rowptr, col, code) for o, code in ORDERINGS.items()}
    same = {o: pos[o][c1] // K.CHUNK == pos[o][c2] // K.CHUNK for o in pos}
    print("census: %d cells, %d connections, rows of 1 to %d entries and the hub's %d" % (g.nc, g.nconn, np.delete(F.deg, F.hub).max() + 1, F.deg[F.hub] + 1))
    print("%-22s %5s %4s %5s | same / other chunk: %s" % ("case", "count", "asc", "desc", ", ".join(pos)))
    for name in K.PAIR_CASES + ("hub", "thp == 0", "closed", "ordinary"):
        f = K.cases(name)
        rel = ["%d / %d" % (same[o][f].sum(), (~same[o][f]).sum()) for o in pos]
        print("%-22s %5d %4d %5d | %s" % (name, f.size, asc[f].sum(), (~asc[f]).sum(), ", ".join(rel)))
        assert f.size > 0 and asc[f].any() and (~asc[f]).any(), name
        for o in pos:
            assert same[o][f].any() and (~same[o][f]).any(), (name, o)
    print("leaves %s, isolated %s, cells whose one connection is a case's own %s" % (F.leaves, F.isolated, F.alone))
    assert len(F.leaves) >= 1 and len(F.isolated) >= 1
    # thp == 0 on the deck with thpres: some of them exact ties
    zero = g.thpres == 0.0
    ties = np.concatenate([K.cases(n) for n in K.TIES])
    assert zero[ties].all() and (zero.sum() > ties.size) and (g.thpres > 0).any()
    print("thp == 0 on %d connections of the deck with thpres, %d of them exact ties" % (zero.sum(), ties.size))
    # the hub: at least 40 connections to cells of all chunks, its slice's other rows short
    hub_nbrs = np.where(c1 == F.hub, c2, c1)[K.cases("hub")]
    assert hub_nbrs.size >= 40
    for o in pos:
        assert set(pos[o][hub_nbrs] // K.CHUNK) == {0, 1, 2}, o
        mates = np.flatnonzero(pos[o] // K.SLICE == pos[o][F.hub] // K.SLICE)
        lens = F.deg[mates[mates != F.hub]] + 1
        print("hub (cell %d, %d entries) in slice %d of the %s order; the other rows of the slice have %d to %d entries" %
              (F.hub, F.deg[F.hub] + 1, pos[o][F.hub] // K.SLICE, o, lens.min(), lens.max()))
        assert lens.min() >= 1 and lens.max() <= 7
    # the diagonal first, last and in the middle among the cells of the named cases (and alone in its row)
    named = np.unique(np.concatenate([F.conn[K.cases(n)].ravel() for n in K.PAIR_CASES] + [np.array(F.leaves + [F.hub])]))
    for o in pos:
        kinds = K.diagonal_kind(F.conn, pos[o])
        print("diagonal position among the %d named cells, %s order: %s" % (named.size, o, {k: int((kinds[named] == k).sum()) for k in ("first", "middle", "last")}))
        assert {"first", "middle", "last"} <= set(kinds[named]) and set(kinds[np.array(F.isolated)]) == {"only"}
    # the ties' U ratios (and rs, rv): a wrong winner is a factor of two away
    for seed in SEEDS:
        cv = K.connection_values(g, oracle.cell_props(g, tab, K.state(seed)))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.maximum(cv["U"][:, :, 0] / cv["U"][:, :, 1], cv["U"][:, :, 1] / cv["U"][:, :, 0])
        for name, phases in (("oil tie", [1]), ("three-phase tie", [0, 1, 2]), ("water tie by region", [0])):
            f = K.cases(name)
            print("state %d, %s: smallest U ratio per phase %s" % (seed, name, ["%s %.2f" % ("wog"[a], ratio[f, a].min()) for a in phases]))
            assert np.all(ratio[f][:, phases] >= 2.0), name
        f = K.cases("oil tie")
        assert np.all(cv["rs"][f, 0] != cv["rs"][f, 1])
        f = K.cases("three-phase tie")
        assert np.all(cv["rs"][f, 0] != cv["rs"][f, 1]) and np.all(cv["rv"][f, 0] != cv["rv"][f, 1])


@pytest.mark.parametrize("kind", ["wog", "wo"])
def test_controls_discriminate(oracle, kind):
    """every tie and |dh| == thp connection listed the other way round (the tie then goes to the other cell), every 'one float below'
    with thp one float lower: the per-connection distance between the oracle's result and its control is at least 100 times the
    tolerance the device is held to -- in double AND in float"""
    F = K.fixture()
    g, tab = _deck(kind, "base")
    rowptr, col = oracle.pattern(g)
    scale = tuple(capi.default_params().matbalscale)
    smallest = (np.inf, None)
    for seed in SEEDS:
        st = K.state(seed, kind)
        base = K.connection_blocks(rowptr, col, F.conn, oracle.assemble(g, tab, DT, st, rowptr, col, scale=scale)[1])
        todo = [(f, K.reversed_connection(g, f)) for n in K.TIES + K.AT_THP for f in K.cases(n)]
        todo += [(f, K.with_threshold(g, f, np.nextafter(g.thpres[f], 0.0))) for f in K.cases("one float below")]
        for f, g2 in todo:
            rp2, col2 = oracle.pattern(g2)
            assert np.array_equal(rp2, rowptr) and np.array_equal(col2, col)
            ctl = K.connection_blocks(rowptr, col, F.conn, oracle.assemble(g2, tab, DT, st, rowptr, col, scale=scale)[1])
            err, norm = K.connection_error(ctl, base, both=True)
            rel = K.relative(err, norm)
            others = np.delete(np.arange(g.nconn), f)
            assert np.array_equal(ctl[others], base[others])            # nothing else moved
            d = rel[f].max()
            if d < smallest[0]:
                smallest = (d, (seed, int(f), F.case[f], K.SLOTS[int(rel[f].argmax())]))
            assert d >= 100 * K.RTOL_JAC_F32 > 100 * K.RTOL_JAC, (seed, f, F.case[f], d)
    print("%s: smallest control distance %.3e at (state, connection, case, slot) %s" % ((kind,) + smallest))


@pytest.mark.parametrize("bad", [-1e-13, float("nan"), float("inf"), float("-inf")], ids=["negative", "nan", "inf", "-inf"])
def test_bad_transmissibility_is_refused_at_creation(bad):
    """opmgpu_grid.trans must be finite and >= 0: the SELL planes carry the row's side of a connection in the sign of T and mark well
    fill with NaN, so a negative T was assembled as |T| and a NaN one as a closed connection.  Refused with OPMGPU_EINVAL before any
    device call (so also on a machine without a GPU, and for the local grid of a decomposed context); the message names the connection."""
    import ctypes as C
    lib = capi.load()
    g = K.grid()
    f = int(K.cases("ordinary")[3])
    trans = np.array(g.trans)
    trans[f] = bad
    g2 = decks.GridData(g.nc, g.conn_cells, trans, g.pv, g.z, thpres=g.thpres, pvtnum=g.pvtnum, satnum=g.satnum)
    ctx = C.c_void_p()
    st = lib.opmgpu_create(C.byref(ctx), 0, C.byref(g2.struct()), C.byref(K.tables().struct()), None)
    why = lib.opmgpu_last_error(None).decode()
    assert st == capi.EINVAL and not ctx, (st, why)
    assert "connection %d " % f in why and "(cells %d, %d)" % tuple(g.conn_cells[f]) in why and "negative or not finite" in why


def test_zero_transmissibility_stays_legal():
    """T == 0 (and -0.0) passes the check: without a device the call goes on to OPMGPU_ENODEVICE, with one it succeeds"""
    import ctypes as C
    lib = capi.load()
    g = K.grid()
    trans = np.array(g.trans)
    trans[K.cases("T == 0")[0]] = -0.0
    assert (g.trans == 0.0).sum() == K.PER_CASE
    g2 = decks.GridData(g.nc, g.conn_cells, trans, g.pv, g.z, thpres=g.thpres, pvtnum=g.pvtnum, satnum=g.satnum)
    ctx = C.c_void_p()
    st = lib.opmgpu_create(C.byref(ctx), 0, C.byref(g2.struct()), C.byref(K.tables().struct()), None)
    assert st == (capi.OK if lib.opmgpu_device_count() > 0 else capi.ENODEVICE), (st, lib.opmgpu_last_error(None))
    if ctx:
        lib.opmgpu_destroy(ctx)
