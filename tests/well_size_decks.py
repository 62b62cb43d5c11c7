"""Decks for tests/test_gpu_well_sizes.py: small in cells, large in wells, so that the fixed sizes of the device well model (csrc/wells.hip:
256 threads per well, the 128-perforation tile of k_well_cdp, 64-lane loops over wells, kFusedWells = 256, the 48-well limit of the bordered
pressure level) are crossed while the oracle side stays cheap.

  long_deck()      3 x 3 x 320 cells, nine wells with 1, 64, 127, 128, 129, 255, 256, 257 and 320 perforations (top layer downwards)
  many_deck(nw)    20 x 20 x 2 cells, nw column wells (nw // 6 rate-controlled injectors, oil-rate and BHP producers), reordered so that
                   the well that decides the maxima over the wells and switches control in the pre-solve is the LAST of the list

host_trace(oracle, deck) runs the host well model (opmgpu/wells.py) on the CPU oracle through the first assembly and records what the guard
test_the_cases_are_what_they_claim asserts.      python tests/well_size_decks.py [long | NW ...]      prints that record."""
import os
import sys

import numpy as np

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "opm-simulators-legacy_amd"), _root, os.path.dirname(os.path.abspath(__file__))):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from opmgpu import capi, decks, wells as W  # noqa: E402

LONG_COUNTS = (1, 64, 127, 128, 129, 255, 256, 257, 320)
MANY_SIZES = (48, 49, 64, 65, 256, 257, 300)
# first index of the part of the well list that a second trip of a 64-lane loop / a second workgroup / the unfused pre-solve reaches
TAIL_START = {65: 64, 257: 256, 300: 256}
MANY_LRAT = 10.0          # m3/day of liquid: the special well's limit
# LONG: the two wells without cross-flow.  Well 7 (injector, 257 perforations): only its LAST perforation has a negative drawdown (a layer at
# lower pressure), so the cross-flow decision hangs on index 256 -- the second trip of a 256-thread loop.  Well 8 (producer, 320 perforations):
# only a band of layers at higher pressure inside its first tile has a non-negative drawdown.
CF_WELLS = {7: ("inj", range(256, 257)), 8: ("prod", range(96, 120))}


class Deck:
    def __init__(self, name, grid, tab, st, wl, dt):
        self.name, self.grid, self.tab, self.st, self.wl, self.dt = name, grid, tab, st, wl, dt


def long_deck():
    nx, ny, nz = 3, 3, 320
    dz = 0.5          # 160 m of column: 11 bar of hydrostatic range on 250 bar
    grid = decks.cartesian_grid(nx, ny, nz, dx=50.0, dy=50.0, dz=dz, tops=2500.0, poro=0.25, permx_md=150.0, lognormal_sigma=0.3, seed=7)
    tab = decks.satfunc_standard_tables()
    st = decks.initial_state(grid, tab, p_ref=250 * decks.BAR, z_ref=2500.0, gas_cap_fraction=0.0, gas_only_fraction=0.0)
    col = lambda c, n: [c + nx * ny * k for k in range(n)]          # noqa: E731
    # the pressure bands of the two wells without cross-flow (columns 7 and 8)
    st.p[col(7, nz)[256]] -= 8 * decks.BAR
    for k in CF_WELLS[8][1]:
        st.p[col(8, nz)[k]] += 12 * decks.BAR
    # 20 x permeability x thickness of a layer: rates of tens of m3/day per well, well above tolerance_wells (1e-4 m3/s = 8.6 m3/day), so
    # that a converged pre-solve has found the pattern of flowing perforations and not merely come close
    WI = 20.0 * 150.0 * decks.MD * dz
    day = decks.DAY
    ptop = float(st.p[0])
    wl = W.Wells()
    oil, water = (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)

    def orat(q):
        return (W.SURFACE_RATE, -q / day, oil)
    spec = [  # type, composition, control, limits, allow_cf
        (W.PRODUCER, oil, (W.BHP, ptop - 6 * decks.BAR), [], True),
        (W.PRODUCER, oil, orat(60.0), [(W.BHP, 150 * decks.BAR)], True),
        (W.PRODUCER, oil, (W.BHP, ptop - 4 * decks.BAR), [], True),
        (W.INJECTOR, water, (W.SURFACE_RATE, 250.0 / day, water), [(W.BHP, 400 * decks.BAR)], True),
        (W.PRODUCER, oil, orat(120.0), [(W.BHP, 150 * decks.BAR)], True),
        # the liquid-rate limit is broken in the first pre-solve iteration: a control switch, and a second iteration
        (W.PRODUCER, oil, (W.BHP, ptop - 3 * decks.BAR), [(W.SURFACE_RATE, -100.0 / day, (1.0, 1.0, 0.0))], True),
        (W.PRODUCER, oil, orat(200.0), [(W.BHP, 150 * decks.BAR)], True),
        # 60 m3/day is what the layer at lower pressure takes at about 5.5 bar below the top cell's pressure; a water column (1000 kg/m3)
        # against the reservoir's 700 kg/m3 gains 3.8 bar over 256 layers, so every drawdown above that layer stays positive.  Rate
        # controlled: a BHP-controlled injector without cross-flow starts from q_s = 0 as a dead well (wellbore rate exactly zero), and
        # whether it comes alive is decided by the rounding of a rate of 1e-21 (the reference's rule, StandardWells_impl.hpp:486-506)
        (W.INJECTOR, water, (W.SURFACE_RATE, 60.0 / day, water), [(W.BHP, 400 * decks.BAR)], False),
        (W.PRODUCER, oil, (W.BHP, ptop + 3 * decks.BAR), [], False),
    ]
    for c, (n, (typ, comp, ctrl, limits, cf)) in enumerate(zip(LONG_COUNTS, spec)):
        cells = col(c, n)
        wl.add_well("W%d_%d" % (c, n), typ, grid.z[cells[0]], cells, WI, comp, ctrl, allow_cf=cf, limits=limits)
    return Deck("long", grid, tab, st, wl, 1.0 * day)


def permuted(wl, order, special=None, wi_factor=1.0, more_limits=()):
    """the wells of `wl` in the given order; well `special` with its connection factors scaled and further limits"""
    out = W.Wells()
    for w in order:
        lo, hi = wl.connpos[w], wl.connpos[w + 1]
        s = w == special
        out.add_well(wl.name[w], wl.type[w], wl.depth_ref[w], wl.cells[lo:hi], np.asarray(wl.WI[lo:hi]) * (wi_factor if s else 1.0), wl.comp_frac[w],
                     wl.controls[w][0], allow_cf=wl.allow_cf[w], limits=list(wl.controls[w][1:]) + (list(more_limits) if s else []), current=wl.current0[w])
    return out


def many_deck(nw):
    """column_wells, then one BHP-controlled producer -- the SPECIAL well -- gets four times the connection factor and a liquid-rate limit it
    breaks in the first pre-solve iteration, and moves to the END of the well list.  A liquid-rate control (two phases) does not seed the rates
    when it takes over (updateWellStateWithTarget), so this well alone has a control-equation residual that is not zero and needs a second
    pre-solve iteration; its connection factor gives it the largest flux-equation residual of the assembled system."""
    grid = decks.cartesian_grid(20, 20, 2, dx=100.0, dy=100.0, dz=5.0, tops=2500.0, poro=0.25, permx_md=150.0, lognormal_sigma=0.8, seed=nw)
    tab = decks.satfunc_standard_tables()
    st = decks.initial_state(grid, tab, p_ref=250 * decks.BAR, z_ref=2500.0, gas_cap_fraction=0.0, gas_only_fraction=0.0, perturb=0.002, seed=nw)
    wl = W.column_wells(grid, nw, n_injectors=nw // 6, seed=nw, inj_rate_m3_per_day=60.0, prod_bhp_bar=235.0, prod_oil_rate_m3_per_day=25.0,
                        rate_wells_bhp_limits_bar=(400.0, 150.0))
    special = max(w for w in range(nw) if wl.type[w] == W.PRODUCER and wl.controls[w][0][0] == W.BHP)
    order = [w for w in range(nw) if w != special] + [special]
    return Deck("many%d" % nw, grid, tab, st, permuted(wl, order, special, 4.0, [(W.SURFACE_RATE, -MANY_LRAT / decks.DAY, (1.0, 1.0, 0.0))]), 2.0 * decks.DAY)


class TracingHost(W.StandardWellsHost):
    """the host well model, keeping the well equations' residuals of every evaluation and every control switch"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.residuals, self.switches = [], []

    def converged(self, B_avg):
        self.residuals.append((np.abs(self.flux_eq), np.abs(self.ctrl_eq)))
        return super().converged(B_avg)

    def update_well_controls(self, ws):
        s = super().update_well_controls(ws)
        self.switches.append([w for w, _, _ in s])
        return s


def host_model(oracle, deck, reduction=1e-10):
    from util import OracleBackend
    ob = OracleBackend(oracle, deck.grid, deck.tab, capi.default_params(linear_solver_reduction=reduction, linear_solver_maxiter=8000), wells=deck.wl.arrays())
    wh = TracingHost(deck.wl, deck.grid.z, deck.tab.surface_density[0])
    return W.WellCoupledModel(ob, wh, W.WellState(deck.wl, deck.st.p))


def host_trace(oracle, deck, newton=False):
    """The host well model on the CPU oracle up to and including the first assembly (newton: two whole Newton iterations, the statement that
    host model and oracle converge on this deck by themselves)."""
    wl = deck.wl
    mo = host_model(oracle, deck)
    wh = mo.wh
    mo.prepareStep(deck.dt, deck.st)
    mo.assemble(True)
    conv0 = mo.m.getConvergence()
    wh.converged(mo.m.B_avg)
    n_pre = wh.well_iterations
    # evaluations: n_pre + 1 inside the pre-solve (the last one converged), then the assembled one
    assert len(wh.residuals) == n_pre + 2, (len(wh.residuals), n_pre)
    pre_switches = sorted({w for s in wh.switches[1:1 + n_pre] for w in s})
    perf_well = np.repeat(np.arange(wl.nw), np.diff(np.asarray(wl.connpos)))
    pp = mo.m.perfProps(wl.nperf).reshape(wl.nperf, 9, 4)
    B = np.asarray(mo.m.B_avg)
    out = {"nw": wl.nw, "perforations": np.diff(np.asarray(wl.connpos)).tolist(), "presolve_iterations": n_pre,
           "presolve_switches": pre_switches,
           # the well equations' residuals as getWellConvergence weighs them (B_avg x |flux equation|, |control equation|): in the first
           # evaluation of the pre-solve, in the one after its first control update, and in the assembled system of Newton iteration 0
           "first_flux_argmax": int(np.argmax((wh.residuals[0][0] * B).max(1))),
           "ctrl_argmax": int(np.argmax(wh.residuals[min(1, n_pre)][1])), "ctrl_max": float(wh.residuals[min(1, n_pre)][1].max()),
           "flux_argmax": int(np.argmax((wh.residuals[-1][0] * B).max(1))), "flux_max": (wh.residuals[-1][0] * B).max(0).tolist(),
           "drawdown": pp[:, 0, 0] - (mo.ws.bhp[perf_well] + wh.cdp), "cdp": wh.cdp.copy(), "current": mo.ws.current.copy(), "converged0": bool(conv0)}
    if newton:
        ob = mo.m
        for it in range(2):
            if it:
                mo.assemble(False)
                ob.getConvergence()
                wh.converged(ob.B_avg)
            ob.solveJacobianSystem(single_precision=False)
            wh.recover_and_update(ob.perfDx(wl.nperf), mo.ws)
            ob.updateState()
        s = ob.getState()
        out["newton_ok"] = bool(np.isfinite(s.p).all() and (s.p > 0).all() and np.isfinite(mo.ws.bhp).all())
        out["linear_iterations"] = ob.linear_iterations
    return out


if __name__ == "__main__":
    import time
    from oracle import oracle as orc
    orc.lib()
    np.set_printoptions(linewidth=200, precision=4)
    for arg in sys.argv[1:] or ["long"] + [str(n) for n in MANY_SIZES]:
        t0 = time.time()
        deck = long_deck() if arg == "long" else many_deck(int(arg))
        tr = host_trace(orc, deck, newton=True)
        dd = tr.pop("drawdown"); tr.pop("cdp")
        print(deck.name, {k: v for k, v in tr.items() if k != "current"}, "%.1f s" % (time.time() - t0))
        if arg == "long":
            cp = deck.wl.connpos
            for w, (kind, band) in CF_WELLS.items():
                neg = np.flatnonzero(dd[cp[w]:cp[w + 1]] < 0)
                print("  well %d (%s): %d negative drawdowns, first %d last %d" % (w, kind, neg.size, neg[0], neg[-1]))
