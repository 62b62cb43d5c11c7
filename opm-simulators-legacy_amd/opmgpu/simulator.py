"""Report-step driver on top of the device Newton path: what SimulatorBase::run does around `flow_legacy`'s hot path
(opm/autodiff/SimulatorBase_impl.hpp:90-324), reduced to what an external diff needs:

    deck -> grid / tables / initial state (EQUIL, with SWATINIT) -> [SWATINIT: setSwatInitScaling] -> [THPRES: computeMaxDp of the
    initial state, setThresholdPressures] -> set the state (the order of FlowMain::setupState, FlowMain.hpp:636-692) -> [AQUFETP / AQUCT:
    setAquifers, once] -> for every report
    step of the SCHEDULE: the step's dissolution limits (DRSDT / DRVDT), wells of the step (WellsManager), well state carried over by name, updateSatOilMax + updateSatHyst (:190-192), AdaptiveTimeStepping.step with the NonlinearSolver (:236-253),
    restart + summary output (:300-306).

The physics runs in libopmgpu.so (state resident on the device across sub-steps); this module is host plumbing.  Output goes to
ECLIPSE binary files (opmgpu/eclio.py) that `compareECL` can diff against a `flow_legacy` run of the same deck.
"""
import numpy as np

from . import capi, deck as deckmod, eclio, schedule as schedmod, timestepping as ts, wells as W
from .decks import DAY
from .model import GpuBlackoilModel, NonlinearSolver


class Simulator:
    def __init__(self, deck_path, params=None, output_base=None, device=0, ats=None, vfp_tables=(), model_factory=None, well_model_factory=None,
                 restart=None):
        """model_factory(grid, tables, params) / well_model_factory(model, wells, well_state): other implementations of the model interface
        behind the same driver (the tests run the CPU oracle + host well model through it and diff the two runs' output files like the
        reference's regression tests diff flow_legacy's); default: the device model / the device well model.
        restart = (base, report): start from report step `report` of BASE.UNRST written by an earlier run of the same deck instead of the
        deck's initial state (what tests/run-restart-regressionTest.sh exercises: the restarted run must reproduce the full one within
        abs 2e-1 / rel 4e-5): reservoir state, VAPPARS / hysteresis history, well state by name; the run continues with the SCHEDULE's
        next report step."""
        self.deck = deckmod.read_deck(deck_path)
        self.tables = self.deck.tables()
        self.grid = self.deck.grid()
        self.state0 = self.deck.initial_state(self.tables)
        deck_state0 = self.state0                       # a restart replaces state0; the defaulted THPRES values come from the deck's
        self.start_step, self.t0, self._restart_ws = 0, 0.0, None
        if restart is not None:
            self._load_restart(*restart)
        nx, ny, nz = self.deck.dims
        n = nx * ny * nz
        dx, dy, dz = self.deck._cell_sizes()
        kx = self.deck.array("PERMX", n, np.zeros(n))
        ky = self.deck.array("PERMY", n, kx)
        self.schedule = schedmod.Schedule(self.deck, self.grid, perm_md=(kx, ky), dz=dz.ravel(), dxdy=(dx.ravel(), dy.ravel()),
                                          ntg=self.deck.array("NTG", n, np.ones(n)))
        self.params = params or capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1)
        self.well_model_factory = well_model_factory
        if model_factory is None:
            self.model = GpuBlackoilModel(self.grid, self.tables, self.params, device=device)
            set_state = self.model.setState
        else:
            self.model = model_factory(self.grid, self.tables, self.params)
            set_state = lambda st: self.model.prepareStep(1.0, st)      # noqa: E731
            if self.tables.pvcdo is not None and not isinstance(self.model, GpuBlackoilModel):
                # the tables hold only a constant stand-in for this oil; a model that evaluates them (the CPU oracle behind the host well
                # model) would compute another fluid
                if not hasattr(self.model, "setPvcdo"):
                    raise ValueError("the deck has PVCDO with a compressibility / viscosibility, but the model cannot take the analytic oil (setPvcdo)")
                self.model.setPvcdo(self.tables.pvcdo)
        if self.deck.hysteresis():
            hmodel, killough_a = self.deck.hysteresis_model()
            if hmodel == capi.HYST_KILLOUGH:
                # the scanning curves are the device's own rule (opmgpu_set_hysteresis_model); a model without the setter (the CPU oracle
                # behind the host well model) would run Carlson's
                if not hasattr(self.model, "setHysteresisModel"):
                    raise ValueError("EHYSTR item 2 = 2 (Killough): the model cannot take the hysteresis model (setHysteresisModel)")
                self.model.setHysteresisModel(hmodel, killough_a)
        if self.deck.swatinit() is not None:
            # FlowMain.hpp:683-690: the capillary pressure of the scaled curve at the initial saturations goes to setSwatInitScaling.  Before
            # computeMaxDp, which must see the scaled curve (the reference's two property objects share one material-law manager); from the
            # DECK's equilibration also on a restarted run, like the thresholds.
            if not hasattr(self.model, "setSwatInitScaling"):
                raise ValueError("the deck has SWATINIT, but the model cannot take the scaling (setSwatInitScaling)")
            self.model.setSwatInitScaling(deck_state0.sat[:, 0], deck_state0.pcow)
        self.threshold_pressures = None
        barriers = self.deck.thpres()
        if barriers is None:
            set_state(self.state0)
        else:
            # FlowMain.hpp:675-680 -> SimulatorBase_impl.hpp:467-468: computeMaxDp of the DECK's initial state (setupState runs before a
            # restart file is loaded), thresholdPressures / thresholdPressuresNNC, setThresholdPressures; then the state the run starts from
            if not hasattr(self.model, "setThresholdPressures"):
                raise ValueError("the deck has THPRES, but the model cannot take threshold pressures (setThresholdPressures)")
            max_dp = None
            if any(v is None for v in barriers.values()):
                eql = self.deck.eqlnum()
                set_state(deck_state0)
                nregions = max(int(eql.max()), max(r2 for _, r2 in barriers))          # (a barrier may name a region without cells)
                max_dp = self.model.computeMaxDp(eql, nregions, self.grid.n_face_conn)
            self.threshold_pressures = self.deck.threshold_pressures(self.grid, max_dp)
            self.model.setThresholdPressures(self.threshold_pressures)
            set_state(self.state0)
        # AQUFETP / AQUCT + AQUANCON: installed once, behind the initial state; the context carries them and their state through the
        # report steps' well re-plans (the rule is the device's own, include/opmgpu.h)
        self.aquifers = self.deck.aquifers(self.tables)
        if self.aquifers:
            # a model without the setter (the CPU oracle behind the host well model) would run the deck as a closed box, without a word
            if not hasattr(self.model, "setAquifers"):
                raise ValueError("the deck has analytic aquifers (AQUFETP / AQUCT), but the model cannot take them (setAquifers)")
            if self.start_step > 0:
                raise ValueError("the deck has analytic aquifers: a restarted run is not supported (the restart file does not carry the aquifers' state)")
            self.model.setAquifers(self.aquifers)
        # ROCKCOMP: rock regions and the compaction mode, installed once; the context carries them and the history p_min through the
        # report steps' well re-plans (the rule is the device's own, include/opmgpu.h).  The history starts from the state the run
        # starts from -- on a restarted run from the file's PRESROCK first (run()) --; saveState() then takes every converged sub-step.
        self.rock_regions = self.deck.rock_regions()
        if self.rock_regions is not None:
            # a model without the setter (the CPU oracle behind the host well model) would run table 1 in every cell, without a word
            if not hasattr(self.model, "setRockRegions"):
                raise ValueError("the deck has ROCKCOMP, but the model cannot take rock regions (setRockRegions)")
            self.model.setRockRegions(self.rock_regions)
        self.ats = ats or ts.AdaptiveTimeStepping(initial_timestep_days=1.0)
        if getattr(self, "_restart_dtnx", None) is not None:
            self.ats.suggested_next_timestep = self._restart_dtnx
        self.vfp_tables = vfp_tables
        self.fipnum = self.deck.fipnum()             # REGIONS FIPNUM (None: the field is one region)
        self.out = None
        if output_base:
            # EclOutput truncates BASE.UNRST / .UNSMRY: a restarted run writing over the files it was just started from would destroy the full run's
            import os
            if restart is not None and os.path.abspath(output_base) == os.path.abspath(restart[0]):
                raise ValueError("output_base %r is the restart source: choose another base name for the restarted run's files" % output_base)
            porv = np.zeros(n); porv[self.deck.active] = self.grid.pv
            tops = self.deck.array("TOPS")[:nx * ny] if self.deck.has("TOPS") and self.deck.array("TOPS").size >= nx * ny else None
            cz = (self.deck.array("COORD"), self.deck.array("ZCORN")) if self.deck.has("ZCORN") else None
            self.out = eclio.EclOutput(output_base, (nx, ny, nz), self.grid.active_index, self.schedule.start, cell_sizes=(dx, dy, dz), tops=tops, porv=porv,
                                       coord_zcorn=cz, phases=self.tables.phases)
        self.reports = []

    def _load_restart(self, base, report):
        from .decks import BAR, State
        r = eclio.read_restart(base, report)
        sw = np.asarray(r["SWAT"], float)
        zero = np.zeros_like(sw)
        if self.tables.phases == "wo":                    # a deck without a gas phase writes no SGAS / RS / RV
            r = dict(r, SGAS=zero, RS=zero, RV=zero)
        sg = np.asarray(r["SGAS"], float)
        sat = np.stack([sw, 1.0 - sw - sg, sg], 1)
        hc = np.where(sg > 0, np.where(sat[:, 1] > 0, capi.HC_GAS_AND_OIL, capi.HC_GAS_ONLY), capi.HC_OIL_ONLY).astype(np.int8)     # initHydroCarbonState
        if not self.tables.has_disgas:
            hc[hc == capi.HC_OIL_ONLY] = capi.HC_GAS_AND_OIL
        self.state0 = State(np.asarray(r["PRESSURE"], float) * BAR, sat, np.asarray(r["RS"], float), np.asarray(r["RV"], float), hc)
        self.start_step, self.t0 = report - 1, r["DAYS"] * DAY        # report 1 is the initial state, report k + 1 follows schedule step k - 1
        self._restart_extra = {k: np.asarray(r[k], float) for k in ("SOMAX", "HMDC_OW", "HMDC_GO", "PRESROCK") if k in r}
        self._restart_dtnx = float(r["OPMGDTNX"][0]) * DAY if "OPMGDTNX" in r else None
        if "OPMGXWEL" in r:
            x = np.asarray(r["OPMGXWEL"], float).reshape(-1, 5)
            self._restart_ws = ([str(n).strip() for n in r["OPMGWNAM"]], x, np.asarray(r["OPMGIWEL"], int))

    def run(self, max_steps=None):
        gm = self.model
        t, prev_ws, prev_names = self.t0, None, None
        if self.start_step > 0:
            ex = getattr(self, "_restart_extra", {})
            if "SOMAX" in ex and hasattr(gm, "setSatOilMax"):
                gm.setSatOilMax(ex["SOMAX"])
            if "HMDC_OW" in ex and hasattr(gm, "setHysteresis"):
                gm.setHysteresis(ex["HMDC_OW"], ex["HMDC_GO"])
            if "PRESROCK" in ex and self.rock_regions is not None:
                from .decks import BAR
                gm.setRockHistory(ex["PRESROCK"] * BAR)
        if self.rock_regions is not None:
            gm.updateRockHistory()                        # the initial (or restarted) state is the first the rock has seen
        if self.out:
            self.out.report = self.start_step             # the restarted run numbers its report steps like the full one
            extra0 = {}
            if self.rock_regions is not None:             # (the history of the state the run starts from)
                from .decks import BAR
                extra0["PRESROCK"] = gm.rockHistory() / BAR
            self.out.write_restart(t / DAY, gm.getState(), extra=extra0)
        nsteps = len(self.schedule.steps) if max_steps is None else min(max_steps, len(self.schedule.steps))
        for step in range(self.start_step, nsteps):
            dt = self.schedule.steps[step][0]
            wl = self.schedule.wells(step)
            st = gm.getState()
            ws = W.WellState(wl, st.p)
            if step == self.start_step and self._restart_ws is not None:          # the restart file's well state, by name
                names, x, cur = self._restart_ws
                for w, name in enumerate(wl.name):
                    if str(name)[:8] in names:
                        k = names.index(str(name)[:8])
                        ws.bhp[w], ws.thp[w], ws.qs[w] = x[k, 0], x[k, 1], x[k, 2:5]
                        if cur[k] < len(wl.controls[w]):
                            ws.current[w] = cur[k]
            if prev_ws is not None:                       # WellStateFullyImplicitBlackoil::init(..., prevState): same-name wells keep their state
                for w, name in enumerate(wl.name):
                    if name in prev_names:
                        k = prev_names.index(name)
                        ws.bhp[w], ws.qs[w], ws.thp[w] = prev_ws.bhp[k], prev_ws.qs[k], prev_ws.thp[k]
                        if prev_ws.current[k] < len(wl.controls[w]):
                            ws.current[w] = prev_ws.current[k]
            event = prev_names != list(wl.name)
            if step == self.start_step and self._restart_ws is not None and [str(n)[:8] for n in wl.name] == self._restart_ws[0]:
                event = False                             # the same wells as at the end of the run the restart file comes from
            lim = self.schedule.dissolution[step]         # DRSDT / DRVDT in force (the rule is the device's own, include/opmgpu.h)
            if lim != getattr(self, "_dissolution", (None, False, None)):
                # a model without the setter (the CPU oracle behind the host well model) would let gas re-dissolve at once, without a word
                if not hasattr(gm, "setDissolutionLimits"):
                    raise ValueError("the deck has DRSDT / DRVDT, but the model cannot take dissolution limits (setDissolutionLimits)")
                gm.setDissolutionLimits(lim[0], lim[1], lim[2])
                self._dissolution = lim
            if hasattr(gm, "updateSatOilMax"):
                gm.updateSatOilMax()                      # SimulatorBase_impl.hpp:190-192
                gm.updateHysteresis()
            if wl.nw > 0 and hasattr(gm, "lib"):         # SimulatorBase_impl.hpp:196: computeRESV before the step's solver is built
                from .rateconverter import SurfaceToReservoirVoidage, computeRESV
                if getattr(self, "_rate_converter", None) is None:
                    self._rate_converter = SurfaceToReservoirVoidage(gm)      # one region of all cells (:66), a member like rateConverter_
                computeRESV(self._rate_converter, wl, pvtnum=getattr(self.grid, "pvtnum", None))
            if wl.nw == 0:
                model = gm
            elif self.well_model_factory is not None:
                model = self.well_model_factory(gm, wl, ws)
            else:
                model = W.DeviceWellModel(gm, wl, ws, vfp_tables=self.vfp_tables)
            if wl.nw > 0 and getattr(wl, "groups", None):
                self._install_groups(model, wl)
            host_ws = ws if (wl.nw > 0 and not hasattr(model, "pull_well_state")) else None        # a host well model keeps the well state here
            rep = self.ats.step(t, dt, _Solver(), model, event=event, well_state=host_ws)
            t += dt
            if wl.nw > 0 and hasattr(model, "pull_well_state"):
                ws = model.pull_well_state()
            self.reports.append({"step": step, "days": t / DAY, "substeps": len(rep["substeps"]), "newton": rep["newton_iterations"],
                                 "linear": rep["linear_iterations"], "failed": len(rep["failed"])})
            if hasattr(gm, "computeFluidInPlace"):      # COIP of SimulatorBase_impl.hpp:278: values[region][7] at the end of every report step
                self.reports[-1]["fip"] = gm.computeFluidInPlace(self.fipnum)
            if self.aquifers:                             # per aquifer (W_e, W_s, p_a): cumulative influx, reservoir and surface volume, and its pressure
                we, wsurf, _, pa = gm.aquiferState()
                self.reports[-1]["aquifers"] = [(float(a), float(b), float(c)) for a, b, c in zip(we, wsurf, pa)]
            if self.out:
                extra = {}
                rpt = self.schedule.rptrst[step]
                if any(v > 0 for v in rpt.values()):      # the arrays RPTRST selects of the output record (getRestartData), one evaluation
                    extra.update(eclio.restart_simulator_data(rpt, gm.simulatorData(), self.tables.phases))
                if hasattr(gm, "satOilMax") and self.tables.vap1 + self.tables.vap2 > 0:
                    extra["SOMAX"] = gm.satOilMax()
                if hasattr(gm, "getHysteresis") and self.grid.imbnum is not None:
                    h = gm.getHysteresis()
                    extra["HMDC_OW"], extra["HMDC_GO"] = h[0], h[1]
                if self.rock_regions is not None:         # the compaction history [bar], like PRESSURE
                    from .decks import BAR
                    extra["PRESROCK"] = gm.rockHistory() / BAR
                self.out.write_restart(t / DAY, gm.getState(), extra=extra, wells=wl if wl.nw > 0 else None, well_state=ws if wl.nw > 0 else None,
                                       next_step_days=self.ats.suggested_next_timestep / DAY)
                if wl.nw > 0:
                    # field totals in place and the hydrocarbon-pv weighted pressure (SimulatorBase_impl.hpp:278: COIP at every report step)
                    fip = gm.computeFluidInPlace()[0] if hasattr(gm, "computeFluidInPlace") else None
                    self.out.write_summary(t / DAY, wl, ws, new_report_step=True, fip=fip)
            prev_ws, prev_names = (ws.copy(), list(wl.name)) if wl.nw > 0 else (None, None)
        return self.reports

    def _install_groups(self, model, wl):
        """Group control of the report step.  Guide rates the deck leaves to the potentials (WGRUPCON defaulted, or no WGRUPCON) come from
        computeWellPotentials, called once per report step and only then (BlackoilModelBase_impl.hpp:2576-2619 does so when the deck has
        group controls): |d_g . potential| with a tiny positive floor.  The device well model then takes the groups behind its wells
        (opmgpu_set_well_groups); the host well model reads them from the well list."""
        if hasattr(model, "install_groups"):
            model.install_groups(lambda: model.computeWellPotentials(self.grid.z, self.tables.surface_density[0], self.vfp_tables))
        elif hasattr(model, "computeWellPotentials"):
            W.resolve_guide_rates(wl.groups, lambda: model.computeWellPotentials(from_well_state=True))
        elif any(np.isnan(g) for grp in wl.groups for g in grp.guide):
            raise ValueError("the deck leaves a guide rate to the well potentials, but the well model cannot compute them (computeWellPotentials)")

    def close(self):
        if hasattr(self.model, "close"):
            self.model.close()


class _Solver:
    """NonlinearSolver::step with the reference defaults; AdaptiveTimeStepping expects solver.step(model) -> (newton, linear)"""

    def __init__(self):
        self.ns = NonlinearSolver()

    def step(self, model):
        it, lin_total = 0, 0
        while True:
            converged, lin = model.nonlinearIteration(it, nonlinear_solver=self.ns)
            lin_total += lin
            it += 1
            if not ((not converged and it <= self.ns.max_iter) or it <= self.ns.min_iter):
                break
        if not converged:
            from .model import TooManyIterations
            raise TooManyIterations("Solver convergence failure - Failed to complete a time step within %d iterations." % self.ns.max_iter)
        return it, lin_total
