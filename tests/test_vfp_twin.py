"""The device's VFP evaluators (csrc/vfp.hpp: vfp_find, vfp_interp5, vfp_vars, vfp_bhp, vfp_thp), compiled by plain g++ into the host twin
tests/support/vfp_host.cpp, against the restatement opmgpu/vfp.py -- axis by axis, for every FLO / WFR / GFR definition, producer and injector
signs, one-point axes, two- and one-point THP axes, and a table whose bhp(thp) is not sorted.  No GPU needed; tests/test_gpu_vfp.py runs the
same tables, points and bounds through the device.  Tables, points and the derivation of the bounds: tests/vfp_cases.py.

Worst errors measured over the eight tables, in units of the derived bounds (each test prints its own): value 0.080, partial derivatives 0.019,
gradient in q 0.012, THP inversion 0.030; every decision of the THP inversion lies at least 1.2e9 bounds away from every point.
Swapping two strides of vfp_interp5, dropping the d[2] * dgfr term and flipping the injector's flo sign in csrc/vfp.hpp each fail
test_twin_matches_host_restatement here (tried on the twin; errors of 1e13 bounds).
"""
import subprocess

import numpy as np
import pytest

import vfp_cases as vc

NAMES = list(vc.tables())


def _worst(err, bound):
    """largest error in units of its bound; a zero bound demands a zero error"""
    err, bound = np.abs(np.asarray(err, float)), np.asarray(bound, float)
    assert np.all(np.isfinite(err))
    assert np.all(err[bound == 0.0] == 0.0)
    nz = bound > 0.0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_points_cover_what_they_claim(name):
    """every multi-point axis is met below its first node, exactly on its first and last node (the latter is the v >= ax[n-1] boundary), inside, and
    above the last node; zero rates and both zero-denominator forms occur; producer rates are negative, injector rates positive"""
    t, pts, h = vc.tables()[name], vc.points(name), vc.host_values(name)
    values = [pts["thp"], h.vars[:, 1], h.vars[:, 2], pts["alq"], h.vars[:, 0]]
    for k, (ax, v) in enumerate(zip(vc._axes5(t), values)):
        if ax.size == 1:
            continue
        lowest_possible = ax[0] <= 0.0 and k in (1, 2, 4)         # nothing lies below a first node of zero on an axis of non-negative values
        assert lowest_possible or np.any(v < ax[0]), k
        assert np.any(v == ax[0]) and np.any(v == ax[-1]) and np.any(v > ax[-1]) and np.any((v > ax[0]) & (v < ax[-1])), k
        on = pts["on_node"] == k
        assert on.sum() == ax.size and np.all(np.isin(v[on], ax)), k      # built to sit on a node, and does, to the bit
    q = pts["q"]
    signed = q[pts["kind"] != "zero"]         # (the zero block has one point of opposite aqua and liquid rates, for a zero sum)
    assert np.all(signed >= 0.0) if t.is_injector else np.all(signed <= 0.0)
    assert np.any(np.all(q == 0.0, axis=1))
    if not t.is_injector:
        z = q[pts["kind"] == "zero"]
        assert np.any((z[:, 0] != 0.0) & (z[:, 1] == 0.0)) and np.any((z[:, 0] == 0.0) & (z[:, 1] != 0.0)) and np.any((z[:, 2] == 0.0) & (z[:, 1] != 0.0))
        assert np.any(z[:, 0] + z[:, 1] == 0.0)
    assert (pts["kind"] == "random").sum() >= 300
    if name == "dip":
        assert h.unsorted.all()              # the unsorted branch of find_thp, at every point
    else:
        assert not h.unsorted[pts["kind"] == "random"].all()


@pytest.mark.parametrize("name", NAMES)
def test_twin_matches_host_restatement(name):
    tabs = list(vc.tables().values())
    index = NAMES.index(name)                   # every table but the first sits behind others in the packed blob
    t, pts, h = tabs[index], vc.points(name), vc.host_values(name)
    bhp, dq, thp = vc.twin_evaluate(tabs, index, pts["q"], pts["thp"], pts["alq"], pts["bhp_in"])
    var, val, par = vc.twin_partials(tabs, index, pts["q"], pts["thp"], pts["alq"])
    sgn = 1.0 if t.is_injector else -1.0
    assert np.array_equal(var[:, 0] * sgn, h.vars[:, 0])                          # flo, wfr, gfr: the same IEEE operations, the same bits
    assert t.is_injector or np.array_equal(var[:, 1:], h.vars[:, 1:])             # (an injector table has no ratio axes to look them up on)
    assert np.array_equal(val, bhp)
    worst = {"value": _worst(bhp - h.bhp, h.bhp_bound), "partials": _worst(par - h.partials, h.partials_bound),
             "gradient": _worst(dq - h.dq, h.dq_bound), "thp": _worst(thp - h.thp, h.thp_bound)}
    print("%s: worst error / bound %s; decisions of the THP inversion at >= %.3g bounds" % (name, worst, h.knot_margin))
    assert worst["value"] <= 1.0 and worst["partials"] <= 1.0 and worst["gradient"] <= 1.0 and worst["thp"] <= 1.0, worst
    # the table is felt along every axis it has, and through every rate the chain rule reaches
    for k, ax in enumerate(vc._axes5(t)):
        assert (np.abs(h.partials[:, k]).max() > 0.0) == (ax.size > 1), k
    if not t.is_injector and t.wfr.size > 1 and t.gfr.size > 1:
        assert np.all(np.abs(h.dq[pts["kind"] == "random"]).max(axis=0) > 0.0)
    if t.thp.size == 1:
        assert np.all(thp == t.thp[0])


def test_a_table_behind_others_gives_what_it_gives_alone():
    """the blob offsets of a table that is not the first: bit for bit the single-table result"""
    tabs = list(vc.tables().values())
    for index in (0, 3, len(tabs) - 1):
        pts = vc.points(NAMES[index])
        a = vc.twin_evaluate(tabs, index, pts["q"], pts["thp"], pts["alq"], pts["bhp_in"])
        b = vc.twin_evaluate([tabs[index]], 0, pts["q"], pts["thp"], pts["alq"], pts["bhp_in"])
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", NAMES)
def test_non_finite_arguments_terminate_and_come_back_as_nan(name):
    """a NaN flo, thp, alq or bhp -- what a diverged update hands the tables -- must end inside the table and come back as NaN wherever the
    argument is looked up on an axis of more than one point; the host restatement raises there, a kernel cannot"""
    tabs = list(vc.tables().values())
    index = NAMES.index(name)
    t, pts = tabs[index], vc.points(name)
    i = int(np.flatnonzero(pts["kind"] == "random")[0])
    base = np.concatenate([pts["q"][i], [pts["thp"][i], pts["alq"][i], pts["bhp_in"][i]]])
    flo_rates = {0: [1], 1: [0, 1], 2: [2]}[t.flo_type]
    multi_alq = (not t.is_injector) and t.alq.size > 1
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            p = base.copy()
            p[k] = bad
            bhp, dq, thp = vc.twin_evaluate(tabs, index, p[None, :3], p[3:4], p[4:5], p[5:6])          # returns at all
            if not np.isnan(bad):
                continue
            if k in flo_rates or (k == 4 and multi_alq):
                assert np.isnan(bhp[0]) and (t.thp.size == 1 or np.isnan(thp[0])), (k, bhp, thp)
            if k == 3 and t.thp.size > 1:
                assert np.isnan(bhp[0])
            if k == 5 and t.thp.size > 1:
                assert np.isnan(thp[0])
            if k == 5:
                assert np.isfinite(bhp[0]) and np.all(np.isfinite(dq))          # bhp_in feeds the inversion alone


def test_unknown_table_is_refused():
    tabs = list(vc.tables().values())
    z = np.zeros(1)
    for index in (-1, len(tabs)):
        st = vc.twin().vfp_host_evaluate(len(tabs), vc.ctypes_tables(tabs), index, 1, *[vc.capi.dptr(a) for a in (np.zeros(3), z, z, z, z, np.zeros(3), z)])
        assert st != 0


def test_edge_list_runs_clean_under_the_sanitizers():
    """vfp_host_check: the fixed edge list, non-finite arguments included, on the same header built with -fsanitize=address,undefined
    (a stand-alone program; nothing sanitized is loaded into this interpreter)"""
    r = subprocess.run(["timeout", "-k", "5", "120", vc.CHECK_PATH], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failed checks" in r.stdout


@pytest.mark.parametrize("name", ["prod_thp5", "inj_thp", "bhp_to_thp"])
def test_lockstep_cases_test_what_they_claim_on_the_host(oracle, name):
    """the decks tests/test_gpu_vfp.py runs in lockstep against the device, on the host model alone: they converge, the producer's wfr and gfr lie
    strictly inside their axes with aqua and vapour entries in d bhp / d q, the injector's flo inside its axis, and the THP limit found on the
    host is broken after the first update"""
    kw = dict(thp_limit_bar=vc.host_thp_limit(oracle)) if name == "bhp_to_thp" else {}
    case = vc.lockstep_case(name, **kw)
    ws, conv, history = vc.host_run(oracle, case)
    assert conv and len(history) <= 12
    vc.assert_case_claims(name, case, ws, history)
