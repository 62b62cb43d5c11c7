"""GPU: SWATINIT on the device -- opmgpu_set_swatinit_scaling (= BlackoilPropsAdFromDeck::setSwatInitScaling), opmgpu_get_pcw and
opmgpu_cap_press (= capPress) -- against the numpy restatement tests/swatinit_reference.py on the fixtures of tests/swatinit_cases.py,
against the known answers of the reference's DeckWithSwatinit on the 20-cell column, bit for bit against the creation path, against the
CPU oracle, and tests/golden/decks/SWATINIT_SMALL.DATA through the report-step driver.

Tolerances, derived, not measured.  Capillary pressures against the restatement: 1e-13 of the largest value -- both sides do the same
handful of double operations (map, interpolate, scale: under ten roundings of 1.1e-16) on a curve whose steepest slope times its range is
about ten times its maximum.  PCW and the target after scaling: 1e-13 relative, the double rounding of two multiplications and a division.
The 12 truth values: 1e-4 relative (they carry 5-7 digits).  Oracle parity: RTOL_JAC of tests/test_gpu_assembly.py."""

import numpy as np
import pytest

from opmgpu import capi, decks
from opmgpu.model import GpuBlackoilModel
from opmgpu.simulator import Simulator
from util import rel_err

import swatinit_cases as cases
import swatinit_reference as ref
from test_swatinit_deck import DECK
from test_swatinit_equil import KNOWN, SWATINIT, column_case, equilibrated

pytestmark = pytest.mark.gpu

RTOL_JAC = 1e-11          # tests/test_gpu_assembly.py: residual and Jacobian blocks of its vertical-scaling cases
RTOL = 1e-13
PRM = dict(ilu_ordering=capi.ORDER_MULTICOLOR)


def _model(g, t):
    return GpuBlackoilModel(g, t, capi.default_params(**PRM))


def _random_sat(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    sw = rng.random(n)
    sg = (1.0 - sw) * rng.random(n)
    sw[:5], sg[5:10] = (0.0, 1.0, 0.3, 0.7, 0.9), 0.0                # table nodes and the ends
    return np.stack([sw, 1.0 - sw - sg, sg], 1)


def _close(got, want, what):
    scale = np.abs(want).max()
    print("%s: max |device - restatement| = %.3e of %.3e" % (what, np.abs(got - want).max(), scale))
    assert np.abs(got - want).max() <= RTOL * scale


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5: capillary pressure and the setter
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["arrays", "plain", "ow_arrays", "ow"])
def test_cap_press_and_setter_against_the_restatement(gpu_lib, kind):
    g, t, st = cases.case(kind)
    assert g.nc > 256 and g.nc % 64 != 0
    m = _model(g, t)
    assert not np.array_equal(m.ordering()[0], np.arange(g.nc))                          # the plan's numbering is not the caller's
    r = ref.Curves(g, t)
    sat = _random_sat(g.nc, 3)
    pcow, pcgo = m.capPress(sat)
    _close(pcow, r.pcow(sat[:, 0]), kind + " pcow")
    if kind.startswith("ow"):
        assert np.all(pcgo == 0.0)
    else:
        _close(pcgo, r.pcgo(sat[:, 2]), kind + " pcgo")
    with pytest.raises(ValueError, match="state"):
        m.capPress()                                                                     # no resident state yet
    m.setState(st)
    res_w, res_g = m.capPress()
    again = m.capPress(st.sat)
    assert np.array_equal(res_w, again[0]) and np.array_equal(res_g, again[1])           # the resident saturations = the same given ones
    pcw0 = m.getPcw()
    assert np.array_equal(pcw0, r.pcw)                                                   # the array given, or the regions' table maxima
    # the setter
    sw_in, target = cases.imposed(g, t)
    before = m.capPress(np.stack([np.minimum(np.maximum(sw_in, r.swl), r.swu), np.zeros(g.nc), np.zeros(g.nc)], 1))[0]
    sw_out = m.setSwatInitScaling(sw_in, target)
    want_sw, scaled = r.apply_swatinit(sw_in, target)
    assert 0.5 * g.nc < scaled.sum() < g.nc and (target < 0).sum() > 10
    assert np.array_equal(sw_out, want_sw)
    pcw1 = m.getPcw()
    nz = r.pcw != 0.0
    print("%s: max relative |PCW - restatement| = %.3e" % (kind, np.abs(pcw1[nz] / r.pcw[nz] - 1.0).max()))
    assert np.allclose(pcw1, r.pcw, rtol=RTOL, atol=0)
    assert np.array_equal(pcw1[~scaled], pcw0[~scaled]) and np.all(pcw1[scaled & (target != before)] != pcw0[scaled & (target != before)])
    after = m.capPress(np.stack([sw_out, np.zeros(g.nc), np.zeros(g.nc)], 1))[0]
    nz = scaled & (target != 0.0)
    print("%s: max relative |pcow(sw_out) - target| in the scaled cells = %.3e" % (kind, np.abs(after[nz] / target[nz] - 1.0).max()))
    assert np.allclose(after[scaled], target[scaled], rtol=RTOL, atol=0)
    keep = ~scaled & (target >= 0)                       # (where the target is negative sw_out = Swu: compare at the clamped saturation)
    assert np.array_equal(after[keep], before[keep])
    at = m.capPress(np.stack([np.minimum(np.maximum(sw_in, r.swl), r.swu), np.zeros(g.nc), np.zeros(g.nc)], 1))[0]
    assert np.array_equal(at[~scaled], before[~scaled])                                  # bit for bit the old curve in every unscaled cell
    s2 = m.getState()
    assert np.array_equal(s2.sat, st.sat) and np.array_equal(s2.p, st.p)                 # the resident state is only read
    m.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6: the column of DeckWithSwatinit, idempotence
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_column_known_answers_and_idempotence(gpu_lib):
    g, t, rec = column_case()
    host = equilibrated(SWATINIT)
    m = _model(g, t)
    assert np.array_equal(m.getPcw(), np.full(20, 0.4 * decks.BAR))
    sw_out = m.setSwatInitScaling(host.sat[:, 0], host.pcow)
    assert np.array_equal(sw_out, host.sat[:, 0])
    pcow = m.capPress(host.sat)[0]
    truth = np.array(KNOWN["pc_scaled_truth"])
    err = np.abs(pcow[:12] / truth - 1.0)
    print("column: largest relative difference to pc_scaled_truth = %.2e" % err.max())
    assert err.max() <= 1e-4
    pcw1 = m.getPcw()
    assert np.allclose(pcw1, host.pcw, rtol=RTOL, atol=0) and np.array_equal(pcw1[12:], np.full(8, 0.4 * decks.BAR))
    # a second call fed the device's own capillary pressures changes nothing
    sat = np.stack([sw_out, 1.0 - sw_out, np.zeros(20)], 1)
    assert np.array_equal(m.setSwatInitScaling(sw_out, m.capPress(sat)[0]), sw_out)
    assert np.allclose(m.getPcw(), pcw1, rtol=RTOL, atol=0)
    # ... while the same TARGET again compounds nothing either (the curve already passes through it), and another target does
    m.setSwatInitScaling(sw_out, 2.0 * m.capPress(sat)[0])
    assert np.allclose(m.getPcw()[:12], 2.0 * pcw1[:12], rtol=RTOL, atol=0)
    m.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7 / 8: bit for bit the creation path, also after a re-plan; parity with the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
def _assembled(g, t, st, steps):
    m = _model(g, t)
    pcw = None
    for what, arg in steps:
        if what == "swatinit":
            m.setSwatInitScaling(*arg)
            pcw = m.getPcw()
        else:
            m.setWells(*arg)
    m.prepareStep(cases.DT, st)
    m.assemble(True)
    out = m.residual(), m.jacobian()[2], pcw if pcw is None else np.array(m.getPcw())
    m.close()
    return out


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("kind", ["arrays", "plain", "stone2", "ow"])
def test_setter_is_bitwise_the_creation_path(gpu_lib, kind):
    g, t, st = cases.case(kind)
    imp = cases.imposed(g, t)
    w = cases.wells(g)
    untouched = _assembled(g, t, st, [])
    scaled = _assembled(g, t, st, [("swatinit", imp)])
    pcw = scaled[2]
    assert not _same(scaled, untouched)                                                  # the scaling acts on this state
    created = _assembled(cases.with_pcw(g, pcw), t, st, [])
    assert _same(scaled, created)
    replanned = _assembled(g, t, st, [("swatinit", imp), ("wells", w)])
    assert np.array_equal(replanned[2], pcw)                                             # the re-plan keeps what the setter left
    assert _same(replanned, _assembled(cases.with_pcw(g, pcw), t, st, [("wells", w)]))
    assert _same(_assembled(g, t, st, [("wells", w), ("swatinit", imp)]), replanned)     # and after the re-plan
    assert not _same(replanned, _assembled(g, t, st, [("wells", w)]))


def test_scaled_assembly_matches_the_oracle(gpu_lib, oracle):
    """the unchanged CPU oracle, given the PCW the setter left, at the tolerance of test_gpu_assembly.py's vertical-scaling cases"""
    for kind in ("arrays", "plain"):
        g, t, st = cases.case(kind)
        scaled = _assembled(g, t, st, [("swatinit", cases.imposed(g, t))])
        go = cases.with_pcw(g, scaled[2])
        rowptr, col = oracle.pattern(go)
        r0, v0, _, _ = oracle.assemble(go, t, cases.DT, st, rowptr, col, scale=tuple(capi.default_params().matbalscale))
        print("%s: oracle parity residual %.2e, Jacobian %.2e" % (kind, rel_err(scaled[0], r0), rel_err(scaled[1], v0)))
        assert rel_err(scaled[1], v0) < RTOL_JAC and rel_err(scaled[0], r0) < RTOL_JAC
        r1, v1, _, _ = oracle.assemble(g, t, cases.DT, st, rowptr, col, scale=tuple(capi.default_params().matbalscale))
        assert rel_err(v1, v0) > 1e-6                                                    # the oracle sees the scaling too


# ---------------------------------------------------------------------------------------------------------------------------------------
# 9: refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu_lib):
    g, t, st = cases.case("arrays")
    sw, pcow = cases.imposed(g, t)
    m = _model(g, t)
    m.setSwatInitScaling(sw, pcow)
    pcw = m.getPcw()
    for which, k, bad, text in ((0, 300 % g.nc, np.nan, "not finite"), (0, 3, np.inf, "not finite"), (1, 200, np.nan, "not finite"), (1, 9, -np.inf, "not finite"),
                                (0, 17, -1e-9, "outside"), (0, g.nc - 1, 1.0 + 1e-9, "outside")):
        a, b = sw.copy(), pcow.copy()
        (a, b)[which][k] = bad
        out = np.full(g.nc, -7.0)
        status = m.lib.opmgpu_set_swatinit_scaling(m.ctx, capi.dptr(a), capi.dptr(b), capi.dptr(out))
        assert status == capi.EINVAL
        msg = m.lib.opmgpu_last_error(m.ctx).decode()
        assert text in msg and ("cell %d" % k) in msg
        assert np.all(out == -7.0) and np.array_equal(m.getPcw(), pcw)
        with pytest.raises(ValueError, match=text):
            m.setSwatInitScaling(a, b)
    with pytest.raises(ValueError):
        m.setSwatInitScaling(sw[:-1], pcow[:-1])
    assert m.lib.opmgpu_set_swatinit_scaling(m.ctx, None, capi.dptr(pcow), None) == capi.EINVAL
    assert m.lib.opmgpu_get_pcw(m.ctx, None) == capi.EINVAL and m.lib.opmgpu_cap_press(m.ctx, None, None) == capi.EINVAL
    assert np.array_equal(m.getPcw(), pcw)
    m.prepareStep(cases.DT, st)
    m.assemble(True)
    got = m.residual(), m.jacobian()[2]
    m.close()
    assert _same(got, _assembled(cases.with_pcw(g, pcw), t, st, []))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 10: through the driver
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_deck_with_swatinit_runs(gpu_lib):
    sim = Simulator(DECK)
    host = sim.state0
    dev = sim.model.getState()
    assert np.array_equal(dev.sat, host.sat) and np.array_equal(dev.p, host.p)           # the initial SWAT is the host EQUIL's
    sw = sim.deck.swatinit()
    assert np.array_equal(dev.sat[36:6 * 36, 0], sw[36:6 * 36])                          # ... which honours SWATINIT above the contact
    pp = host.phase_pressure
    scaled = sim.grid.z < 2530.0
    pcow = sim.model.capPress()[0]
    print("deck: max relative |device pcow - (po - pw)| in the scaled cells = %.3e" % np.abs(pcow[scaled] / (pp[:, 1] - pp[:, 0])[scaled] - 1.0).max())
    assert np.allclose(pcow[scaled], (pp[:, 1] - pp[:, 0])[scaled], rtol=1e-12, atol=0)
    assert np.allclose(sim.model.getPcw(), host.pcw, rtol=RTOL, atol=0)
    reps = sim.run()
    assert [r["days"] for r in reps] == [5.0] and reps[0]["failed"] == 0 and reps[0]["newton"] > 0
    sim.close()
    # a model that cannot take the scaling is refused, not run unscaled
    class Bare:                                                                          # noqa: E306
        def prepareStep(self, dt, st):
            pass
    with pytest.raises(ValueError, match="SWATINIT"):
        Simulator(DECK, model_factory=lambda grid, tables, params: Bare())
