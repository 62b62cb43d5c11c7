"""Tables, points, host values and derived error bounds shared by tests/test_vfp_twin.py (the host build of csrc/vfp.hpp) and
tests/test_gpu_vfp.py (the same evaluators on the device).  The reference of both is the restatement opmgpu/vfp.py, which tests/test_vfp.py
pins to the reference's known answers.

Bounds (float64, eps = 2^-52).  The evaluator forms the value as a sum over the 32 corners c of the table cell, sum_c w_c v_c with w_c a product
of five interpolation factors, and each partial derivative as sum_c pw_c v_c; opmgpu/vfp.py nests the same interpolation axis by axis.  Both
are sums of the same 32 terms with at most five products each, so they differ by at most a small multiple of eps * sum_c |w_c v_c|:
    value                |dev - host| <= 64 eps * sum_c |w_c v_c|
    partial derivative k                 64 eps * sum_c |pw_c v_c|
    gradient in q_j                      the chain rule's sum of the partials' bounds, each times |d var_k / d q_j|
    thp of a bhp                         (the value bounds at the two ends of the interval taken) / |d bhp / d thp| of it + 64 eps |thp|
64 covers the 32-term sum and the five products per term.  The interval of an axis is chosen from flo / wfr / gfr, which both sides compute by
the same single IEEE operations, so it never differs; the interval of the THP inversion is chosen by comparing bhp values that do differ, so
every point keeps a distance from each such decision that exceeds the bound (asserted in evaluate(), no point is left out).
"""
import ctypes as C
import functools
import os

import numpy as np

from opmgpu import capi, vfp

EPS = 2.0 ** -52
K = 64.0
BAR = 1e5

TWIN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "support", "_build", "libvfphost.so")
CHECK_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "support", "_build", "vfp_host_check")


# ---- tables --------------------------------------------------------------------------------------------------------------------------
def _axes(nthp, nwfr, ngfr, nalq, nflo, wfr_type, gfr_type):
    """unequally spaced axes; the ratios' nodes are dyadic so that rates can be built that sit on them exactly"""
    flo = 0.0009765625 * np.array([1, 3, 8, 14, 24, 40][:nflo], float)                                  # m3/s (2^-10 multiples)
    thp = BAR * np.array([10.0, 22.0, 50.0, 70.0, 115.0][:nthp])
    wfr = {vfp.WFR_WOR: [0.0, 0.25, 1.0, 3.0], vfp.WFR_WCT: [0.0, 0.125, 0.5, 0.75], vfp.WFR_WGR: [0.0, 0.0009765625, 0.00390625, 0.0078125]}[wfr_type][:nwfr]
    gfr = {vfp.GFR_GOR: [32.0, 128.0, 320.0, 1024.0], vfp.GFR_GLR: [16.0, 64.0, 256.0, 640.0], vfp.GFR_OGR: [0.0009765625, 0.00390625, 0.0078125, 0.03125]}[gfr_type][:ngfr]
    alq = np.array([0.0, 64.0, 256.0, 448.0][:nalq])
    one = lambda a, n: np.array([0.0]) if n == 1 else np.asarray(a, float)      # noqa: E731
    return flo, thp, one(wfr, nwfr), one(gfr, ngfr), one(alq, nalq)


def _data(flo, thp, wfr, gfr, alq, profile=None):
    """bhp [Pa] non-linear in every variable and not separable; increasing in thp unless `profile` gives the THP term per node"""
    t = (thp / BAR) if profile is None else np.asarray(profile, float)
    T, Wf, G, A, F = np.meshgrid(t, wfr / max(wfr[-1], 1e-300), gfr / max(gfr[-1], 1e-300), alq / max(alq[-1], 1e-300), flo / flo[-1], indexing="ij")
    return BAR * (60.0 + 1.1 * T + 0.002 * T * T * (1.0 + 0.3 * Wf) + 45.0 * F ** 1.5 * (1.0 + 0.8 * Wf) + 22.0 * Wf ** 2 * (1.0 - 0.4 * G)
                  - 30.0 * np.sqrt(G + 0.01) * (1.0 - 0.5 * F) - 9.0 * A * A * (1.0 + 0.5 * Wf) - 4.0 * A * G + 2.0 * np.sin(3.0 * Wf + 2.0 * G + A))


def _prod(table_id, types, shape, profile=None):
    nthp, nwfr, ngfr, nalq, nflo = shape
    ax = _axes(nthp, nwfr, ngfr, nalq, nflo, types[1], types[2])
    return vfp.VFPProdTable(table_id, 2500.0, types[0], types[1], types[2], *ax, _data(*ax, profile=profile))


def _inj(table_id, flo_type, nthp, nflo):
    flo, thp, wfr, gfr, alq = _axes(nthp, 1, 1, 1, nflo, 0, 0)
    d = _data(flo, thp, wfr, gfr, alq).reshape(nthp, nflo)
    return vfp.VFPInjTable(table_id, 2500.0, flo_type, flo, thp, d - 0.5 * (d - d[:, :1]))          # an injector's bhp still rises with its rate


@functools.lru_cache(maxsize=None)
def tables():
    """name -> table; the order is the order they are set in on the device, so all but the first sit at non-zero blob offsets"""
    LIQ = (vfp.FLO_LIQ, vfp.WFR_WCT, vfp.GFR_GLR)
    return {
        "prod5_liq": _prod(11, LIQ, (4, 4, 4, 3, 5)),
        "prod5_oil": _prod(12, (vfp.FLO_OIL, vfp.WFR_WOR, vfp.GFR_GOR), (3, 2, 4, 2, 6)),
        "prod5_gas": _prod(13, (vfp.FLO_GAS, vfp.WFR_WGR, vfp.GFR_OGR), (5, 3, 2, 4, 3)),
        "inj": _inj(11, vfp.FLO_LIQ, 4, 5),                                                 # same id as a producer table: the kinds are kept apart
        "one_point": _prod(15, (vfp.FLO_OIL, vfp.WFR_WOR, vfp.GFR_GOR), (3, 1, 1, 1, 4)),
        "thp2": _prod(16, LIQ, (2, 3, 2, 2, 3)),
        "thp1": _prod(17, LIQ, (1, 2, 3, 2, 3)),
        # the THP term of the data dips at the third node (below the second, above the first): bhp(thp) is not sorted anywhere in the table
        "dip": _prod(18, LIQ, (5, 3, 3, 2, 4), profile=[10.0, 40.0, 25.0, 70.0, 115.0]),
    }


def ctypes_tables(tabs):
    """array of opmgpu_vfp_table for the host twin (the device path builds its own in DeviceWellModel); keeps its arrays alive"""
    arr = (capi.VfpTable * len(tabs))()
    keep = []
    for k, t in enumerate(tabs):
        v = arr[k]
        v.id, v.is_injector, v.flo_type, v.datum_depth = t.id, int(t.is_injector), t.flo_type, t.datum_depth
        axes = [capi.f64(t.flo), capi.f64(t.thp)] + ([] if t.is_injector else [capi.f64(t.wfr), capi.f64(t.gfr), capi.f64(t.alq)])
        data = capi.f64(t.data).ravel()
        keep += axes + [data]
        v.nflo, v.nthp, v.flo, v.thp, v.data = axes[0].size, axes[1].size, capi.dptr(axes[0]), capi.dptr(axes[1]), capi.dptr(data)
        if not t.is_injector:
            v.wfr_type, v.gfr_type = t.wfr_type, t.gfr_type
            v.nwfr, v.ngfr, v.nalq = axes[2].size, axes[3].size, axes[4].size
            v.wfr, v.gfr, v.alq = capi.dptr(axes[2]), capi.dptr(axes[3]), capi.dptr(axes[4])
    arr._keep = keep
    return arr


# ---- the host twin --------------------------------------------------------------------------------------------------------------------
_twin = None


def twin():
    global _twin
    if _twin is None:
        if not os.path.exists(TWIN_PATH):
            raise RuntimeError("%s not found -- build it with `make -C tests/support` (build() does)" % TWIN_PATH)
        lib = C.CDLL(TWIN_PATH)
        dp = C.POINTER(C.c_double)
        lib.vfp_host_evaluate.restype = C.c_int
        lib.vfp_host_evaluate.argtypes = [C.c_int, C.POINTER(capi.VfpTable), C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp]
        lib.vfp_host_partials.restype = C.c_int
        lib.vfp_host_partials.argtypes = [C.c_int, C.POINTER(capi.VfpTable), C.c_int, C.c_int, dp, dp, dp, dp, dp, dp]
        _twin = lib
    return _twin


def twin_evaluate(tabs, index, q, thp, alq, bhp_in):
    q, thp, alq, bhp_in = (capi.f64(a) for a in (q, thp, alq, bhp_in))
    n = thp.size
    bhp, dq, tout = np.full(n, -1.0), np.full((n, 3), -1.0), np.full(n, -1.0)
    st = twin().vfp_host_evaluate(len(tabs), ctypes_tables(tabs), index, n, capi.dptr(q), capi.dptr(thp), capi.dptr(alq), capi.dptr(bhp_in),
                                  capi.dptr(bhp), capi.dptr(dq), capi.dptr(tout))
    assert st == 0, st
    return bhp, dq, tout


def twin_partials(tabs, index, q, thp, alq):
    q, thp, alq = (capi.f64(a) for a in (q, thp, alq))
    n = thp.size
    var, val, par = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 5))
    st = twin().vfp_host_partials(len(tabs), ctypes_tables(tabs), index, n, capi.dptr(q), capi.dptr(thp), capi.dptr(alq), capi.dptr(var), capi.dptr(val), capi.dptr(par))
    assert st == 0, st
    return var, val, par


# ---- host evaluation with its bounds --------------------------------------------------------------------------------------------------
def table_vars(t, q):
    """flo (on the table's own, positive axis), wfr, gfr of the rates q = (aqua, liquid, vapour)"""
    sgn = 1.0 if t.is_injector else -1.0
    flo = sgn * vfp.get_flo(q[0], q[1], q[2], t.flo_type)
    if t.is_injector:
        return flo, 0.0, 0.0
    return flo, vfp.get_wfr(q[0], q[1], q[2], t.wfr_type), vfp.get_gfr(q[0], q[1], q[2], t.gfr_type)


def _axes5(t):
    one = np.array([0.0])
    return [t.thp, one, one, one, t.flo] if t.is_injector else [t.thp, t.wfr, t.gfr, t.alq, t.flo]


def corner_sums(t, q, thp, alq):
    """sum_c |w_c v_c| and, per axis k, sum_c |pw_c v_c| over the 32 corners of the cell the point lies in (the bounds' scale)"""
    flo, wfr, gfr = table_vars(t, q)
    it = [vfp.find_interp_data(v, ax) for v, ax in zip((thp, wfr, gfr, alq, flo), _axes5(t))]
    cube = np.asarray(t.data, float).reshape([a.size for a in _axes5(t)])[np.ix_(*[(i[0], i[1]) for i in it])]
    w = [np.array([1.0 - i[3], i[3]]) for i in it]
    outer = lambda vs: functools.reduce(np.multiply.outer, vs)      # noqa: E731
    s0 = float(np.abs(outer(w) * cube).sum())
    sk = [float(np.abs(outer([np.array([-it[k][2], it[k][2]]) if j == k else w[j] for j in range(5)]) * cube).sum()) for k in range(5)]
    return s0, np.array(sk)


def host_lookup(t, q, thp, alq, swap_ratios=False, flip_flo=False):
    """value and the five partials (thp, wfr, gfr, alq, flo) by opmgpu/vfp.py; the two switches make the WRONG evaluations the sensitivity
    controls need: wfr and gfr looked up on each other's axis, and flo looked up with the opposite sign"""
    flo, wfr, gfr = table_vars(t, q)
    if swap_ratios:
        wfr, gfr = gfr, wfr
    if flip_flo:
        flo = -flo
    it = [vfp.find_interp_data(v, ax) for v, ax in zip((thp, wfr, gfr, alq, flo), _axes5(t))]
    cube = np.asarray(t.data, float).reshape([a.size for a in _axes5(t)])[np.ix_(*[(i[0], i[1]) for i in it])]
    v, d = vfp._interpolate(cube, it)
    return v, np.array(d)


def var_gradients(t, q):
    """d (wfr, gfr, flo-as-in-the-rates) / d q, rows of 3"""
    if t.is_injector:
        return np.zeros(3), np.zeros(3), vfp.d_flo(t.flo_type)
    return vfp.d_wfr(q[0], q[1], q[2], t.wfr_type), vfp.d_gfr(q[0], q[1], q[2], t.gfr_type), vfp.d_flo(t.flo_type)


class HostValues:
    """what opmgpu/vfp.py gives at the points of a case, with the bound of every number"""


def evaluate(t, pts):
    """pts: dict q [n,3], thp, alq, bhp_in -> HostValues (arrays over the points).  Asserts every point's distance to the decisions of the
    THP inversion."""
    q, thp, alq, bhp_in = pts["q"], pts["thp"], pts["alq"], pts["bhp_in"]
    n = thp.size
    h = HostValues()
    h.bhp, h.bhp_bound, h.partials, h.partials_bound = np.zeros(n), np.zeros(n), np.zeros((n, 5)), np.zeros((n, 5))
    h.dq, h.dq_bound, h.thp, h.thp_bound, h.vars = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n), np.zeros((n, 3))
    h.unsorted = np.zeros(n, bool)
    h.knot_margin = np.inf              # smallest distance to a decision of the THP inversion, in units of the bound there
    for i in range(n):
        a, l, v = q[i]
        s0, sk = corner_sums(t, q[i], thp[i], alq[i])
        h.vars[i] = table_vars(t, q[i])
        h.bhp[i], h.partials[i] = host_lookup(t, q[i], thp[i], alq[i])
        h.bhp_bound[i], h.partials_bound[i] = K * EPS * s0, K * EPS * sk
        val, dq = t.bhp_dq(a, l, v, thp[i], alq[i])
        assert val == h.bhp[i]
        dw, dg, df = var_gradients(t, q[i])
        h.dq[i] = dq
        h.dq_bound[i] = h.partials_bound[i, 1] * np.abs(dw) + h.partials_bound[i, 2] * np.abs(dg) + h.partials_bound[i, 4] * np.abs(df)
        nthp = t.thp.size
        if nthp == 1:
            h.thp[i], h.thp_bound[i] = t.thp[0], 0.0          # the device's convention; the host restatement has no answer for one node
            continue
        b = np.array([host_lookup(t, q[i], tn, alq[i])[0] for tn in t.thp])
        bb = np.array([K * EPS * corner_sums(t, q[i], tn, alq[i])[0] for tn in t.thp])
        h.unsorted[i] = bool(np.any(b[:-1] > b[1:]))
        h.thp[i] = t.thp_of(a, l, v, bhp_in[i], alq[i])
        # decisions: bhp against every node's value, and the order of neighbouring nodes
        h.knot_margin = min(h.knot_margin, float((np.abs(bhp_in[i] - b) / bb).min()), float((np.abs(np.diff(b)) / (bb[:-1] + bb[1:])).min()))
        j = _interval_taken(b, bhp_in[i])
        slope = abs((b[j + 1] - b[j]) / (t.thp[j + 1] - t.thp[j]))
        h.thp_bound[i] = (bb[j] + bb[j + 1]) / slope + K * EPS * abs(h.thp[i])
    assert h.knot_margin > 4.0, h.knot_margin
    return h


def _interval_taken(b, bhp):
    """the interval vfp.find_thp interpolates on"""
    n = b.size
    is_sorted = bool(np.all(b[:-1] <= b[1:]))
    if is_sorted and bhp <= b[0]:
        return 0
    if is_sorted and bhp > b[-1]:
        return n - 2
    for i in range(n - 1):
        if b[i] < bhp <= b[i + 1]:
            return i
    return 0 if bhp <= b[0] else n - 2


# ---- points ---------------------------------------------------------------------------------------------------------------------------
def rates_for(t, flo, wfr, gfr):
    """rates (aqua, liquid, vapour), signed like the well's, whose table variables are flo (positive axis value), wfr, gfr"""
    sgn = 1.0 if t.is_injector else -1.0
    if t.is_injector:
        return {vfp.FLO_OIL: (0.0, sgn * flo, 0.0), vfp.FLO_LIQ: (sgn * flo, 0.0, 0.0), vfp.FLO_GAS: (0.0, 0.0, sgn * flo)}[t.flo_type]
    key = (t.flo_type, t.wfr_type, t.gfr_type)
    f = sgn * flo
    if key == (vfp.FLO_OIL, vfp.WFR_WOR, vfp.GFR_GOR):
        return wfr * f, f, gfr * f
    if key == (vfp.FLO_LIQ, vfp.WFR_WCT, vfp.GFR_GLR):
        return wfr * f, f - wfr * f, gfr * f
    if key == (vfp.FLO_GAS, vfp.WFR_WGR, vfp.GFR_OGR):
        return wfr * f, gfr * f, f
    raise ValueError(key)


def _positions(ax, rng, n_random):
    """below the first node, every node (the last is the v >= ax[n-1] boundary), between nodes, above the last; then random over 1.6 spans"""
    if ax.size == 1:
        return np.concatenate([[ax[0]], ax[0] + rng.uniform(-1.0, 1.0, n_random)])
    span = ax[-1] - ax[0]
    fixed = np.concatenate([[ax[0] - 0.25 * span], ax, 0.5 * (ax[:-1] + ax[1:]), [ax[-1] + 0.25 * span]])
    return np.concatenate([fixed, rng.uniform(ax[0] - 0.3 * span, ax[-1] + 0.3 * span, n_random)])


@functools.lru_cache(maxsize=None)
def points(name, n_random=300):
    """dict of arrays for table `name`: a block that walks every axis through its fixed positions (the others at an inner value), zero rates and
    zero denominators, then n_random points over and around the whole table.  `on_node[k]` marks the points built to sit exactly on a node of
    axis k (thp, wfr, gfr, alq, flo); `kind` names each point's block."""
    t = tables()[name]
    rng = np.random.default_rng(20240611 + t.id)
    ax = _axes5(t)
    # the inner value of the axes not walked: thp and alq are arguments and take any value; wfr, gfr and flo are made of the rates, and only
    # values of a few bits (as the nodes have) keep the products and sums of rates_for() exact, which "exactly on a node" needs
    mid = [a[0] if a.size == 1 else 0.5 * (a[0] + a[1]) * (1.03 if k in (0, 3) else 1.0) for k, a in enumerate(ax)]
    rows, kind, node = [], [], []
    for k in range(5):                                          # axis by axis
        if ax[k].size == 1 and k != 3:
            continue
        for p in _positions(ax[k], rng, 0):
            v = list(mid)
            v[k] = p
            if k in (1, 2) and p < 0.0:                         # a ratio of rates of one sign is not negative: below a first node of 0 there is nothing
                continue
            if k == 4 and p <= 0.0:
                continue
            rows.append(v); kind.append("axis%d" % k); node.append(k if p in ax[k] else -1)
    ext = [_positions(a, rng, n_random) for a in ax]
    for i in range(n_random):                                   # everything at once
        v = [e[-1 - i] for e in ext]
        v[1], v[2], v[4] = abs(v[1]), abs(v[2]), max(abs(v[4]), 1e-5)
        rows.append(v); kind.append("random"); node.append(-1)
    q = [rates_for(t, v[4], v[1], v[2]) for v in rows]
    thp, alq = [v[0] for v in rows], [v[3] for v in rows]
    # zero rates and zero denominators: all rates zero (0/0 in both ratios); single phases (x/0 and 0/x)
    sgn = 1.0 if t.is_injector else -1.0
    f = sgn * float(0.5 * (t.flo[0] + t.flo[1]))
    for z in [(0.0, 0.0, 0.0), (f, 0.0, 0.0), (0.0, f, 0.0), (0.0, 0.0, 200.0 * f), (f, 0.0, 200.0 * f), (0.0, f, 200.0 * f), (0.3 * f, 0.7 * f, 0.0), (f, -f, 100.0 * f)]:
        q.append(z); thp.append(mid[0] * 1.01); alq.append(mid[3]); kind.append("zero"); node.append(-1)
    q, thp, alq = np.array(q, float), np.array(thp, float), np.array(alq, float)
    # the bhp to invert: the table's own value at a THP drawn around the axis, so the answer is known to lie there (between nodes, not on them)
    if t.thp.size > 1:
        span = t.thp[-1] - t.thp[0]
        tstar = rng.uniform(t.thp[0] - 0.3 * span, t.thp[-1] + 0.3 * span, thp.size)
    else:
        tstar = thp
    bhp_in = np.array([host_lookup(t, q[i], tstar[i], alq[i])[0] for i in range(thp.size)])
    return {"q": q, "thp": thp, "alq": alq, "bhp_in": bhp_in, "kind": np.array(kind), "on_node": np.array(node)}


@functools.lru_cache(maxsize=None)
def host_values(name, n_random=300):
    return evaluate(tables()[name], points(name, n_random))


# ---- decks of the lockstep runs (device wells against host wells on the oracle) ---------------------------------------------------------
def _well_table(table_id, datum_depth, flo_coeff):
    """5-axis FLO_LIQ / WFR_WCT / GFR_GLR producer table around the rates the producer of the 300-cell deck reaches (liquid ~0.01 m3/s, water cut
    ~0.08, gas-liquid ratio ~100): bhp [bar] non-linear in all five variables.  flo_coeff > 0: friction dominates, bhp rises with the rate;
    < 0: the lift-dominated side of a tubing curve, bhp falls with the rate"""
    flo = np.array([0.0005, 0.002, 0.006, 0.014, 0.04])
    thp = BAR * np.array([10.0, 22.0, 50.0, 70.0])
    wfr, gfr, alq = np.array([0.0, 0.04, 0.15, 0.4]), np.array([40.0, 85.0, 140.0, 300.0]), np.array([0.0, 50.0, 120.0])
    T, Wc, G, A, F = np.meshgrid(thp / BAR, wfr, gfr, alq, flo, indexing="ij")
    data = BAR * (150.0 + T + 0.002 * T * T + flo_coeff * F * (1.0 + 2.0 * Wc) + 3.0 * np.sqrt(1e3 * F) + 30.0 * Wc * (1.0 + Wc)
                  - 0.03 * G * (1.0 - 0.5 * Wc) - 0.02 * A * (1.0 + Wc) - 1e-4 * A * A)
    return vfp.VFPProdTable(table_id, datum_depth, vfp.FLO_LIQ, vfp.WFR_WCT, vfp.GFR_GLR, flo, thp, wfr, gfr, alq, data)


def _inj_table(table_id, datum_depth):
    """injector table: bhp [bar] = static head + thp - friction, non-linear in thp and flo"""
    flo, thp = np.array([0.001, 0.005, 0.012, 0.025, 0.05]), BAR * np.array([20.0, 60.0, 100.0, 150.0])
    T, F = np.meshgrid(thp / BAR, flo, indexing="ij")
    return vfp.VFPInjTable(table_id, datum_depth, vfp.FLO_LIQ, flo, thp, BAR * (200.0 + T + 0.001 * T * T - 600.0 * F - 2e4 * F * F))


LOCKSTEP_ALQ = 70.0             # between the ALQ nodes 50 and 120


def lockstep_case(name, thp_limit_bar=None):
    """the 300-cell deck of test_wells_host._limits_setup with the wells of case `name`:
      prod_thp5   the producer on THP control (30 bar, between THP nodes) through the 5-axis table, ALQ between nodes; a decoy table is set first
      inj_thp     the water injector on THP control through an injector table (the producer stays on BHP control)
      bhp_to_thp  the producer on BHP control with a THP limit of thp_limit_bar, through a table whose bhp falls with the rate
    Returns grid, tab, st, wells, tables and a factory of the initial well state."""
    from opmgpu import decks, wells as W
    from test_wells_host import _limits_setup
    grid, tab, st, _, _ = _limits_setup()
    nx, ny, nz = 10, 10, 3
    col = lambda i, j: [i + nx * j + nx * ny * k for k in range(nz)]      # noqa: E731
    WI = 5.0 * float(np.median(grid.trans))
    zi, zp = grid.z[col(0, 0)[0]], grid.z[col(nx - 1, ny - 1)[0]]
    wl = W.Wells()
    inj_ctrl, inj_lim = (W.SURFACE_RATE, 2000.0 / 86400.0, (1.0, 0.0, 0.0)), [(W.BHP, 600 * BAR)]
    prod_ctrl, prod_lim = (W.BHP, 200 * BAR), []
    decoy = tables()["prod5_oil"]           # never used by a well: it only moves the used tables away from blob offset 0
    if name == "prod_thp5":
        tabs = [decoy, _well_table(3, zp - 5.0, 2e3)]
        prod_ctrl, prod_lim = (W.THP, 30 * BAR, None, 3, LOCKSTEP_ALQ), [(W.BHP, 100 * BAR)]
    elif name == "inj_thp":
        tabs = [decoy, _inj_table(4, zi - 5.0)]
        inj_ctrl = (W.THP, 80 * BAR, None, 4, 0.0)
    elif name == "bhp_to_thp":
        tabs = [decoy, _well_table(3, zp - 5.0, -1e3)]
        prod_lim = [(W.THP, thp_limit_bar * BAR, None, 3, LOCKSTEP_ALQ)]
    else:
        raise ValueError(name)
    wl.add_well("INJ", W.INJECTOR, zi, col(0, 0), WI, (1.0, 0.0, 0.0), inj_ctrl, limits=inj_lim)
    wl.add_well("PROD", W.PRODUCER, zp, col(nx - 1, ny - 1)[:2], WI, (0.0, 1.0, 0.0), prod_ctrl, limits=prod_lim)

    def well_state():
        ws = W.WellState(wl, st.p)
        if name == "inj_thp":           # a THP target is no first guess of a rate: start from the rate an earlier rate-controlled step would have left
            ws.qs[0] = [2000.0 / 86400.0, 0.0, 0.0]
            ws.perf_rates[wl.connpos[0]:wl.connpos[1]] = ws.qs[0] / nz
            ws.thp[0] = 80 * BAR
        if name == "bhp_to_thp":
            ws.thp[1] = 70 * BAR        # as an earlier step would have left it: above the limit, so nothing is broken before the first update
        return ws
    return {"grid": grid, "tab": tab, "st": st, "wells": wl, "tables": tabs, "well_state": well_state}


def host_model(oracle, case):
    """WellCoupledModel / StandardWellsHost of a lockstep case on the oracle (no GPU)"""
    from opmgpu import wells as W
    from util import OracleBackend
    prm_o = capi.default_params(linear_solver_reduction=1e-11, linear_solver_maxiter=500)
    ob = OracleBackend(oracle, case["grid"], case["tab"], prm_o, wells=case["wells"].arrays())
    wh = W.StandardWellsHost(case["wells"], case["grid"].z, case["tab"].surface_density[0], vfp_tables=case["tables"])
    return W.WellCoupledModel(ob, wh, case["well_state"]()), ob


LOCKSTEP_DT = 5 * 86400.0


def host_thp_limit(oracle):
    """the THP limit [bar] of case bhp_to_thp, found on the host model: with a limit that is never broken, the producer's thp after the pre-solve
    (reservoir frozen) and after the first Newton update; the limit lies between them, a tenth of the way up, and between two THP nodes"""
    case = lockstep_case("bhp_to_thp", thp_limit_bar=-1e6)
    mo, _ = host_model(oracle, case)
    mo.prepareStep(LOCKSTEP_DT, case["st"])
    mo.assemble(True)
    before = float(mo.ws.thp[1])
    mo, _ = host_model(oracle, case)
    mo.prepareStep(LOCKSTEP_DT, case["st"])
    mo.nonlinearIteration(0, single_precision=False)
    after = float(mo.ws.thp[1])
    limit = after + 0.1 * (before - after)
    assert after < limit < before and 50 * BAR < limit < 70 * BAR, (before, after)
    return limit / BAR


def assert_case_claims(name, case, ws, history):
    """the host side of a finished lockstep run shows that the case tests what it claims.  ws: the host's well state at convergence; history: the
    wells' current controls after every iteration"""
    t = case["tables"][1]
    if name == "prod_thp5":
        q = ws.qs[1]
        flo, wfr, gfr = table_vars(t, q)
        # strictly inside the axes and off their nodes; thp target and alq between nodes
        assert t.flo[0] < flo < t.flo[-1] and t.wfr[0] < wfr < t.wfr[-1] and t.gfr[0] < gfr < t.gfr[-1], (flo, wfr, gfr)
        assert not np.any(np.isin([flo, wfr, gfr], np.concatenate([t.flo, t.wfr, t.gfr])))
        assert t.alq[1] < LOCKSTEP_ALQ < t.alq[2] and t.thp[1] < 30 * BAR < t.thp[2]
        # the control equation's row feels water and gas: d bhp / d q has aqua and vapour entries, through d[1] * dwfr and d[2] * dgfr
        v, dthp, dwfr, dgfr, dalq, dflo = t.bhp(q[0], q[1], q[2], 30 * BAR, LOCKSTEP_ALQ)
        _, dq = t.bhp_dq(q[0], q[1], q[2], 30 * BAR, LOCKSTEP_ALQ)
        assert dq[0] != 0.0 and dq[2] != 0.0 and dwfr != 0.0 and dgfr != 0.0 and dalq != 0.0, (dq, dwfr, dgfr, dalq)
        assert abs(dgfr * vfp.d_gfr(q[0], q[1], q[2], t.gfr_type)[2]) > 1e-3 * abs(dq[2])            # the vapour entry IS the gfr term
        assert all(h[1] == 0 for h in history) and abs(ws.thp[1] - 30 * BAR) <= 1e-5 * 30 * BAR
    elif name == "inj_thp":
        flo = table_vars(t, ws.qs[0])[0]
        assert t.is_injector and t.flo[0] < flo < t.flo[-1] and flo not in t.flo, flo
        assert all(h[0] == 0 for h in history) and abs(ws.thp[0] - 80 * BAR) <= 1e-5 * 80 * BAR and ws.qs[0, 0] > 0.0
    else:
        # BHP control through the first update, THP control from the next assembly on
        assert history[0][1] == 0 and history[1][1] == 1, history


def host_run(oracle, case, max_iter=12):
    """the time step of a lockstep case on the host model alone: (well state at the end, converged, current controls after every iteration)"""
    mo, _ = host_model(oracle, case)
    mo.prepareStep(LOCKSTEP_DT, case["st"])
    history, it = [], 0
    while True:
        conv, _ = mo.nonlinearIteration(it, single_precision=False)
        history.append(mo.ws.current.copy())
        it += 1
        if (conv and it > 1) or it > max_iter:
            return mo.ws, conv, history
