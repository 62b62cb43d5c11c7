"""Host-side mirror of the reference's model / solver interfaces over the C ABI.

`GpuBlackoilModel` carries the method names and call order of Opm::BlackoilModelBase
(opm/autodiff/BlackoilModelBase_impl.hpp:222-326: prepareStep, nonlinearIteration = assemble ->
getConvergence -> solveJacobianSystem -> updateState) and `GpuNewtonIteration` those of
NewtonIterationBlackoilInterface (NewtonIterationBlackoilInterface.hpp:31-52).  Error behaviour
follows the reference: status codes of the C ABI become the exceptions flow_legacy's time stepper
catches (AdaptiveTimeStepping_impl.hpp:244-281).  All compute happens in libopmgpu.so.
"""
import ctypes as C

import numpy as np

from . import capi


class NumericalIssue(RuntimeError):
    """Opm::NumericalIssue"""


class LinearSolverProblem(RuntimeError):
    """Opm::LinearSolverProblem"""


class ISTLError(RuntimeError):
    """Dune::ISTLError / Dune::MatrixBlockError"""


class TooManyIterations(RuntimeError):
    """Opm::TooManyIterations"""


def _raise(lib, ctx, st):
    if st == capi.OK:
        return
    msg = lib.opmgpu_last_error(ctx)
    msg = msg.decode() if msg else ""
    if st == capi.ENUMERICAL:
        raise NumericalIssue(msg)
    if st == capi.ELINSOLVE:
        raise LinearSolverProblem(msg)
    if st in (capi.EBREAKDOWN, capi.ESINGULAR):
        raise ISTLError(msg)
    if st == capi.EINVAL:
        raise ValueError("opmgpu: invalid argument: " + msg)
    raise RuntimeError("opmgpu status %d: %s" % (st, msg))


class _CprDiagnostics:
    """The pressure hierarchy of the last CPR solve (opmgpu_cpr_levels / _level_get / _vcycle_apply / _apply); needs self.lib, self.ctx
    and an error check self._status(st)."""

    def cpr_levels(self):
        """(level sizes, stored entries per level, wells of the level-0 border)"""
        nl, nw = C.c_int32(0), C.c_int32(0)
        self._status(self.lib.opmgpu_cpr_levels(self.ctx, C.byref(nl), None, None, C.byref(nw)))
        n, nnz = np.zeros(nl.value, np.int32), np.zeros(nl.value, np.int64)
        self._status(self.lib.opmgpu_cpr_levels(self.ctx, C.byref(nl), capi.iptr(n), nnz.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(nw)))
        return n, nnz, nw.value

    def cpr_level(self, level):
        """level `level` as (rowptr, col, val, agg or None, dense inverse or None); level 0 in caller numbering, wells last"""
        n, nnz, _ = self.cpr_levels()
        last = level == len(n) - 1
        rowptr, col, val = np.zeros(n[level] + 1, np.int32), np.zeros(nnz[level], np.int32), np.zeros(nnz[level])
        agg = None if last else np.zeros(n[level], np.int32)
        inv = np.zeros((n[level], n[level])) if last and n[level] <= 96 else None
        self._status(self.lib.opmgpu_cpr_level_get(self.ctx, level, capi.iptr(rowptr), capi.iptr(col), capi.dptr(val), capi.iptr(agg), capi.dptr(inv)))
        return rowptr, col, val, agg, inv

    def cpr_dist_levels(self):
        """(levels, distributed levels) of a decomposed hierarchy; (n, 0) for a rank-local or single-domain one"""
        nl, nd = C.c_int32(0), C.c_int32(0)
        self._status(self.lib.opmgpu_cpr_dist_levels(self.ctx, C.byref(nl), C.byref(nd)))
        return nl.value, nd.value

    def cpr_dist_level(self, level):
        """level `level` of a distributed hierarchy in global numbering: (row ids, rowptr, column ids, values, aggregate ids); this rank's
        owned rows of a distributed level (level 0: caller-local ids, wells at n_local + k), the whole matrix of a replicated one"""
        p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))      # noqa: E731
        cnt = np.zeros(2, np.int64)
        self._status(self.lib.opmgpu_cpr_dist_level_get(self.ctx, level, p64(cnt), None, None, None, None, None))
        nr, nz = int(cnt[0]), int(cnt[1])
        rows, rowptr, cols, val, agg = np.zeros(nr, np.int64), np.zeros(nr + 1, np.int32), np.zeros(nz, np.int64), np.zeros(nz), np.zeros(nr, np.int64)
        self._status(self.lib.opmgpu_cpr_dist_level_get(self.ctx, level, p64(cnt), p64(rows), capi.iptr(rowptr), p64(cols), capi.dptr(val), p64(agg)))
        return rows, rowptr, cols, val, agg

    def cpr_vcycle_apply(self, b):
        b = capi.f64(b)
        x = np.zeros_like(b)
        self._status(self.lib.opmgpu_cpr_vcycle_apply(self.ctx, capi.dptr(b), capi.dptr(x)))
        return x

    def cpr_apply(self, d3):
        d3 = capi.f64(d3)
        v = np.zeros_like(d3)
        self._status(self.lib.opmgpu_cpr_apply(self.ctx, capi.dptr(d3), capi.dptr(v)))
        return v

    def cpr_elliptic_ilu_apply(self, b):
        b = capi.f64(b)
        x = np.zeros_like(b)
        self._status(self.lib.opmgpu_cpr_elliptic_ilu_apply(self.ctx, capi.dptr(b), capi.dptr(x)))
        return x

    def cpr_correction_factors(self):
        a, b = C.c_double(0), C.c_double(0)
        self._status(self.lib.opmgpu_cpr_correction_factors(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value


class GpuNewtonIteration(_CprDiagnostics):
    """B1: computeNewtonIncrement on a BCRS<3x3> system handed over as BSR."""

    def __init__(self, params=None, device=0):
        self.lib = capi.load()
        self.params = params or capi.default_params()
        self.ctx = C.c_void_p()
        st = self.lib.opmgpu_create_solver(C.byref(self.ctx), device, C.byref(self.params))
        if st != capi.OK:
            raise RuntimeError("opmgpu_create_solver failed with status %d (no GPU? there is no CPU fallback)" % st)
        self._iterations = 0
        self.reduction = 0.0

    def close(self):
        if self.ctx:
            self.lib.opmgpu_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def iterations(self):
        return self._iterations

    def _status(self, st):
        _raise(self.lib, self.ctx, st)

    def parallelInformation(self):
        return None         # empty boost::any <=> serial

    def computeNewtonIncrement(self, rowptr, col, val9, rhs3, single_precision):
        nb = self.nb = rowptr.size - 1
        x = np.zeros(3 * nb)
        it, red = C.c_int(0), C.c_double(0)
        st = self.lib.opmgpu_solve_bsr(self.ctx, nb, capi.iptr(rowptr), capi.iptr(col), capi.dptr(capi.f64(val9)),
                                       capi.dptr(capi.f64(rhs3)), int(single_precision), capi.dptr(x), C.byref(it), C.byref(red))
        self._iterations, self.reduction = it.value, red.value
        _raise(self.lib, self.ctx, st)
        return x

    # kernel-level helpers (parity tests / bench)
    def load(self, rowptr, col, val9, single_precision=False):
        nb = rowptr.size - 1
        _raise(self.lib, self.ctx, self.lib.opmgpu_load_bsr(self.ctx, nb, capi.iptr(rowptr), capi.iptr(col), capi.dptr(capi.f64(val9)), int(single_precision)))
        self.nb = nb

    def spmv(self, x3):
        y = np.zeros(3 * self.nb)
        _raise(self.lib, self.ctx, self.lib.opmgpu_spmv(self.ctx, capi.dptr(capi.f64(x3)), capi.dptr(y)))
        return y

    def ilu0_factor(self):
        _raise(self.lib, self.ctx, self.lib.opmgpu_ilu0_factor(self.ctx))

    def ilu0_apply(self, d3):
        v = np.zeros(3 * self.nb)
        _raise(self.lib, self.ctx, self.lib.opmgpu_ilu0_apply(self.ctx, capi.dptr(capi.f64(d3)), capi.dptr(v)))
        return v

    def ilu0_get(self, nnzb):
        lu = np.zeros((nnzb, 9))
        _raise(self.lib, self.ctx, self.lib.opmgpu_ilu0_get(self.ctx, capi.dptr(lu)))
        return lu

    def ordering(self):
        pos, lev = np.zeros(self.nb, np.int32), np.zeros(self.nb, np.int32)
        nl = C.c_int32(0)
        _raise(self.lib, self.ctx, self.lib.opmgpu_get_ordering(self.ctx, capi.iptr(pos), capi.iptr(lev), C.byref(nl)))
        return pos, lev, nl.value

    def time_kernel(self, kernel, reps=20):
        ms = C.c_double(0)
        _raise(self.lib, self.ctx, self.lib.opmgpu_time_kernel(self.ctx, kernel, reps, C.byref(ms)))
        return ms.value


class GpuBlackoilModel(_CprDiagnostics):
    """B2: the BlackoilModel hooks, state resident on the device."""

    def __init__(self, grid, tables, params=None, device=0, wells=None):
        self.lib = capi.load()
        self.grid, self.tables = grid, tables
        self.params = params or capi.default_params()
        self.ctx = C.c_void_p()
        st = self.lib.opmgpu_create(C.byref(self.ctx), device, C.byref(grid.struct()), C.byref(tables.struct()), C.byref(self.params))
        if st != capi.OK:
            why = self.lib.opmgpu_last_error(None)
            raise RuntimeError("opmgpu_create failed with status %d (no GPU? there is no CPU fallback): %s" % (st, why.decode() if why else ""))
        self.nc = grid.nc
        self.max_single_precision_days = 20.0       # BlackoilModelParameters.cpp:95
        self.linear_iterations = 0
        self.dt = None
        self.use_update_stabilization = True        # BlackoilModelParameters.cpp:98
        self.residual_norms_history, self.current_relaxation = [], 1.0
        if getattr(tables, "pvcdo", None) is not None:      # the analytic dead oil the tables cannot express (FluidTables(pvcdo=...))
            self.setPvcdo(tables.pvcdo)
        if wells is not None:
            self.setWells(*wells)

    def close(self):
        if self.ctx:
            self.lib.opmgpu_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _status(self, st):
        self._chk(st)

    def _chk(self, st):
        _raise(self.lib, self.ctx, st)

    def setWells(self, well_connpos, well_cells):
        cp, wc = capi.i32(well_connpos), capi.i32(well_cells)
        self._chk(self.lib.opmgpu_set_wells(self.ctx, cp.size - 1, capi.iptr(cp), capi.iptr(wc)))

    def setState(self, st):
        self._chk(self.lib.opmgpu_set_state(self.ctx, capi.dptr(st.p), capi.dptr(st.sat), capi.dptr(st.rs), capi.dptr(st.rv), capi.bptr(st.hc)))

    def getState(self):
        from .decks import State
        n = self.nc
        st = State(np.zeros(n), np.zeros((n, 3)), np.zeros(n), np.zeros(n), np.zeros(n, np.int8))
        self._chk(self.lib.opmgpu_get_state(self.ctx, capi.dptr(st.p), capi.dptr(st.sat), capi.dptr(st.rs), capi.dptr(st.rv), capi.bptr(st.hc)))
        return st

    # --- BlackoilModelBase hooks -------------------------------------------------------------
    def prepareStep(self, dt, state=None):
        """prepareStep (:222-232): pvdt = pv/dt is folded into assemble(); state upload if given.  With dissolution limits
        (setDissolutionLimits) the caps of this time step are then taken from the resident state: call it again when a failed sub-step has
        restored the saved state and a shorter dt is tried."""
        self.dt = float(dt)
        if state is not None:
            self.setState(state)
        if self.dissolution_limits is not None:
            self._chk(self.lib.opmgpu_begin_dissolution_step(self.ctx, self.dt))
        if self.aquifers is not None:       # the aquifers' A_j, B_j of this time step, likewise from the resident state
            self._chk(self.lib.opmgpu_aquifer_begin_step(self.ctx, self.dt))
            self._aquifer_step_begun = True

    def assemble(self, initial_assembly):
        self._chk(self.lib.opmgpu_assemble(self.ctx, self.dt, int(initial_assembly), None, None, None, None, None))

    def getConvergence(self):
        B, CNV, MB, linf = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
        conv = C.c_int(0)
        st = self.lib.opmgpu_convergence(self.ctx, self.dt, capi.dptr(B), capi.dptr(CNV), capi.dptr(MB), capi.dptr(linf), C.byref(conv))
        self.B_avg, self.CNV, self.MB, self.linf = B, CNV, MB, linf
        self._chk(st)
        return bool(conv.value)

    def referencePrecision(self):
        """The arithmetic the reference's plug-in solves in: residual_.singlePrecision = dt < maxSinglePrecisionTimeStep_
        (BlackoilModelBase_impl.hpp:284) is honoured by the interleaved solver only (NewtonIterationBlackoilInterleaved.cpp:478-480);
        the CPR plug-in never reads it and computes in double (NewtonIterationBlackoilCPR.cpp:117-140)."""
        if self.params.use_cpr:
            return False
        return self.dt < self.max_single_precision_days * 86400.0

    def solveJacobianSystem(self, want_dx=False, single_precision=None):
        if single_precision is None:
            single_precision = self.referencePrecision()
        dx = np.zeros(3 * self.nc) if want_dx else None
        it, red = C.c_int(0), C.c_double(0)
        st = self.lib.opmgpu_solve(self.ctx, int(single_precision), capi.dptr(dx), C.byref(it), C.byref(red))
        self.linear_iterations, self.linear_reduction = it.value, red.value
        self._chk(st)
        return dx

    def updateState(self, dx=None, relax=1.0):
        self._chk(self.lib.opmgpu_update_state(self.ctx, capi.dptr(None if dx is None else capi.f64(dx)), float(relax)))

    # last_state of AdaptiveTimeStepping, kept on the device
    def saveState(self):
        """Keeps the resident state as the last good one.  A begun aquifer step is committed first: the time-step control saves the state
        after every converged sub-step, so this is where the aquifers take their influx of that sub-step, once.  Under irreversible
        compaction (setRockRegions) the state that is saved is a converged one too: the rock takes its pressures into its history."""
        if self._aquifer_step_begun:
            self._chk(self.lib.opmgpu_aquifer_commit_step(self.ctx))
            self._aquifer_step_begun = False
        if self.rock_regions is not None and self.rock_regions.mode == capi.ROCK_IRREVERSIBLE:
            self.updateRockHistory()
        self._chk(self.lib.opmgpu_save_state(self.ctx))

    def restoreState(self):
        """Back to the saved state; a begun aquifer step (the failed sub-step's) is discarded, the committed aquifer state stays."""
        self._chk(self.lib.opmgpu_restore_state(self.ctx))
        self._aquifer_step_begun = False

    def computeFluidInPlace(self, fipnum=None, cells=False, nregions=None):
        """BlackoilModelBase::computeFluidInPlace (BlackoilModelBase_impl.hpp:2263-2445) for the resident state: values[region][7]
        (water, oil, gas, dissolved gas, vaporised oil, pore volume, hydrocarbon-pv weighted pressure); cells=True also returns the
        per-cell arrays [7][nc] (SimulatorData::fip).  Decomposed runs: collective; every rank passes the fipnum of its local cells
        (ghosts included, they are not counted) and the GLOBAL number of regions, and receives the global sums."""
        fn = None if fipnum is None else capi.i32(fipnum)
        dims = nregions if nregions is not None else (1 if fn is None else max(1, int(fn.max())))
        values = np.zeros((dims, 7))
        fc = np.zeros((7, self.nc)) if cells else None
        self._chk(self.lib.opmgpu_compute_fluid_in_place(self.ctx, capi.iptr(fn), dims, capi.dptr(fc), capi.dptr(values)))
        return (values, fc) if cells else values

    def simulatorData(self):
        """BlackoilModelBase's SimulatorData of the resident state (BlackoilModelBase_impl.hpp:662-683, rq_[].b/rho/mu/kr): dict of 16 [nc]
        arrays in SI under the names SimulatorFullyImplicitBlackoilOutput.hpp:512-567 gives them -- 1OVERBW/BO/BG, WAT_/OIL_/GAS_DEN,
        WAT_/OIL_/GAS_VISC, WATKR/OILKR/GASKR (kr itself, not the mobility), RSSAT, RVSAT (saturated, every cell), PBUB, PDEW -- in the
        cell order of getState()."""
        out = np.zeros((capi.SIMDATA_K, self.nc))
        self._chk(self.lib.opmgpu_get_simulator_data(self.ctx, capi.dptr(out)))
        return {name: out[k] for k, name in enumerate(capi.SIMDATA_NAMES)}

    def setThresholdPressures(self, thpres):
        """BlackoilModelBase::setThresholdPressures (BlackoilModelBase_impl.hpp:421-443): the thresholds of ALL connections in the grid's
        connection order (faces, then NNCs), or None to remove them.  Lasts through later setWells / setDeviceWells calls; a negative or
        non-finite value is a ValueError."""
        th = None if thpres is None else capi.f64(thpres)
        if th is not None and th.shape != (self.grid.nconn,):
            raise ValueError("setThresholdPressures: %d values for %d connections" % (th.size, self.grid.nconn))
        self._chk(self.lib.opmgpu_set_threshold_pressures(self.ctx, capi.dptr(th)))

    def setPvcdo(self, pvcdo):
        """PVCDO, the dead oil of constant compressibility and viscosibility (opmgpu_set_pvcdo; the rule is stated in include/opmgpu.h):
        one row (p_ref, B_ref, C_o, mu_ref, C_v) per PVT region in SI, or None to go back to the tabulated oil.  From the call on every
        evaluator of the oil takes the analytic form; it lasts through setWells / setDeviceWells, saved states and a change of
        precision.  A context with dissolved gas, a non-finite entry, B_ref <= 0 or mu_ref <= 0 is a ValueError and changes nothing."""
        o = None if pvcdo is None else capi.f64(pvcdo)
        if o is not None and o.shape != (self.tables.n_pvt, 5):
            raise ValueError("setPvcdo: PVCDO needs one row of five numbers per PVT region (%d regions)" % self.tables.n_pvt)
        self._chk(self.lib.opmgpu_set_pvcdo(self.ctx, capi.dptr(o)))

    def setWellEfficiency(self, factors):
        """Well efficiency factors (WEFAC; opmgpu_set_well_efficiency, the rule is stated in include/opmgpu.h): one factor in (0, 1] per
        device well in the order of opmgpu_set_device_wells, or None for all ones.  The cells see e_w times the well's rates and their
        derivatives; the well equations and the well state do not see it.  Lasts through saved states, a change of precision and a
        re-plan; a new opmgpu_set_device_wells resets it.  No device wells, a non-finite factor or one outside (0, 1] is a ValueError."""
        f = None if factors is None else capi.f64(factors).ravel()
        if f is not None and self.n_device_wells and f.size != self.n_device_wells:
            raise ValueError("setWellEfficiency: %d factors for %d device wells" % (f.size, self.n_device_wells))
        self._chk(self.lib.opmgpu_set_well_efficiency(self.ctx, capi.dptr(f)))

    def getWellEfficiency(self):
        """the factors in force, one per device well"""
        out = np.zeros(max(self.n_device_wells, 1))
        self._chk(self.lib.opmgpu_get_well_efficiency(self.ctx, capi.dptr(out)))
        return out[:self.n_device_wells]

    def setWellGroups(self, groups):
        """Controlled groups of the device wells (opmgpu_set_well_groups; the sharing rule is stated in include/opmgpu.h).  `groups`: a
        sequence of objects with sign (-1 production, +1 injection), target, distr[3], wells (indices of opmgpu_set_device_wells) and
        guide (one positive guide rate per member) -- opmgpu.wells.WellGroup -- or None / empty to remove the groups.  Every member's last
        control must be the group slot.  Lasts through saved states, a change of precision and a re-plan; a new opmgpu_set_device_wells
        removes the groups.  Every refusal of the C entry is a ValueError with its text."""
        groups = list(groups or ())
        if not groups:
            self._chk(self.lib.opmgpu_set_well_groups(self.ctx, 0, None, None, None, None, None, None))
            self.n_well_groups = 0
            return
        ptr = np.concatenate([[0], np.cumsum([len(g.wells) for g in groups])])
        members = np.concatenate([np.asarray(g.wells, np.int64) for g in groups]) if ptr[-1] else np.zeros(0, np.int64)
        guide = np.concatenate([np.asarray(g.guide, float) for g in groups]) if ptr[-1] else np.zeros(0)
        if guide.size != members.size:
            raise ValueError("setWellGroups: %d guide rates for %d member wells" % (guide.size, members.size))
        keep = [capi.i32(ptr), capi.i32(members if members.size else [0]), capi.f64([g.sign for g in groups]), capi.f64([g.target for g in groups]),
                capi.f64(np.asarray([g.distr for g in groups], float).reshape(-1, 3)), capi.f64(guide if guide.size else [1.0])]
        self._chk(self.lib.opmgpu_set_well_groups(self.ctx, len(groups), capi.iptr(keep[0]), capi.iptr(keep[1]), capi.dptr(keep[2]), capi.dptr(keep[3]),
                                                  capi.dptr(keep[4]), capi.dptr(keep[5])))
        self.n_well_groups = len(groups)

    def wellGroupTargets(self):
        """(slot_target[nw], group_rate[ngroups]) of opmgpu_get_well_group_targets: the rule applied on the device to the well state and
        current controls as they stand; NaN for a well in no group."""
        tg, rate = np.zeros(max(self.n_device_wells, 1)), np.zeros(max(self.n_well_groups, 1))
        self._chk(self.lib.opmgpu_get_well_group_targets(self.ctx, capi.dptr(tg), capi.dptr(rate)))
        return tg[:self.n_device_wells], rate[:self.n_well_groups]

    n_well_groups = 0           # groups of the last setWellGroups

    def wellSharedCells(self):
        """(shared_rows, max_wells_per_cell) of the device wells (opmgpu_well_shared_cells): the number of cells perforated by more than one
        well and the most wells found in one cell; (0, 0) for a well list without shared cells.  ValueError without device wells."""
        import ctypes as C
        rows, most = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.opmgpu_well_shared_cells(self.ctx, C.byref(rows), C.byref(most)))
        return rows.value, most.value

    n_device_wells = 0          # wells of the last opmgpu_set_device_wells (DeviceWellModel records it)

    def computeMaxDp(self, eqlnum, nregions, n_face_conn, conns=False):
        """computeMaxDp (opm/simulators/thresholdPressures.hpp:46-298) for the resident state: max_dp[nregions][nregions], the largest
        phase-potential difference over the first n_face_conn connections (the grid faces; NNCs are not scanned) joining each pair of
        the 1-based equilibration regions `eqlnum`; -1.0 = no face joins the pair, 0.0 = joined but no phase counts.  conns=True also
        returns the per-connection plane [nconn].  Decomposed runs: collective, nregions is the global number."""
        eq = capi.i32(eqlnum)
        if eq.shape != (self.nc,):
            raise ValueError("computeMaxDp: eqlnum has %d entries for %d cells" % (eq.size, self.nc))
        out = np.zeros((int(nregions), int(nregions)))
        dp = np.zeros(self.grid.nconn) if conns else None
        self._chk(self.lib.opmgpu_compute_max_dp(self.ctx, capi.iptr(eq), int(nregions), int(n_face_conn), capi.dptr(dp), capi.dptr(out)))
        return (out, dp) if conns else out

    def setSwatInitScaling(self, sw, pcow):
        """BlackoilPropsAdFromDeck::setSwatInitScaling (BlackoilPropsAdFromDeck.cpp:1009-1019): per cell the imposed water saturation and
        the target pcow = p_o - p_w; every cell's maximum oil-water capillary pressure is rescaled by the rule stated in include/opmgpu.h.
        Returns the saturation each cell ends at.  Lasts through later setWells / setDeviceWells calls; calling it twice compounds.  A
        non-finite value or a saturation outside [0, 1] is a ValueError and changes nothing."""
        sw, pcow = capi.f64(sw), capi.f64(pcow)
        if sw.shape != (self.nc,) or pcow.shape != (self.nc,):
            raise ValueError("setSwatInitScaling: one saturation and one capillary pressure per cell (%d cells)" % self.nc)
        out = np.zeros(self.nc)
        self._chk(self.lib.opmgpu_set_swatinit_scaling(self.ctx, capi.dptr(sw), capi.dptr(pcow), capi.dptr(out)))
        return out

    def getPcw(self):
        """each cell's current maximum oil-water capillary pressure [Pa] (PCW, or the table maximum of its saturation region)"""
        out = np.zeros(self.nc)
        self._chk(self.lib.opmgpu_get_pcw(self.ctx, capi.dptr(out)))
        return out

    def capPress(self, sat=None):
        """BlackoilPropsAdFromDeck::capPress: (pcow = p_o - p_w, pcgo = p_g - p_o) of every cell at the saturations sat [nc][3] or, None, at
        the resident state's, through the cell's end-point and vertical scaling"""
        s = None
        if sat is not None:
            s = capi.f64(sat)
            if s.size != 3 * self.nc:
                raise ValueError("capPress: three saturations per cell (%d cells)" % self.nc)
        out = np.zeros((2, self.nc))
        self._chk(self.lib.opmgpu_cap_press(self.ctx, capi.dptr(s), capi.dptr(out)))
        return out[0], out[1]

    def relativeChange(self):
        """BlackoilModelBase::relativeChange(saved, resident) (BlackoilModelBase_impl.hpp:1595-1631)."""
        v = C.c_double(0.0)
        self._chk(self.lib.opmgpu_relative_change(self.ctx, C.byref(v)))
        return v.value

    # satOilMax_ of BlackoilPropsAdFromDeck (VAPPARS); updateSatOilMax is called once per report step (SimulatorBase_impl.hpp:192)
    def setSatOilMax(self, so_max):
        self._chk(self.lib.opmgpu_set_sat_oil_max(self.ctx, capi.dptr(capi.f64(so_max))))

    def updateSatOilMax(self):
        self._chk(self.lib.opmgpu_update_sat_oil_max(self.ctx))

    def satOilMax(self):
        out = np.zeros(self.nc)
        self._chk(self.lib.opmgpu_get_sat_oil_max(self.ctx, capi.dptr(out)))
        return out

    # DRSDT / DRVDT (opmgpu_set_dissolution_limits; the rule is ours and stated in include/opmgpu.h)
    dissolution_limits = None       # (drsdt, free_only, drvdt) in force, rates in 1/s with None = off; None = no limits

    def setDissolutionLimits(self, drsdt=None, free_only=False, drvdt=None):
        """Limits on how fast Rs (drsdt, 1/s; free_only = DRSDT's option FREE) and Rv (drvdt, 1/s) may rise within a time step; None = off,
        both None removes the limits.  prepareStep(dt) then sets the caps of the step.  ValueError with the library's text when refused;
        the previous limits stay in force."""
        self._chk(self.lib.opmgpu_set_dissolution_limits(self.ctx, -1.0 if drsdt is None else float(drsdt), int(bool(free_only)),
                                                         -1.0 if drvdt is None else float(drvdt)))
        on_s, on_v = drsdt is not None and drsdt >= 0, drvdt is not None and drvdt >= 0
        self.dissolution_limits = (float(drsdt) if on_s else None, bool(free_only) and on_s, float(drvdt) if on_v else None) if (on_s or on_v) else None

    def dissolutionCaps(self):
        """(rs_cap, rv_cap) of the current time step, caller cell order; +inf = no cap"""
        rs_cap, rv_cap = np.zeros(self.nc), np.zeros(self.nc)
        self._chk(self.lib.opmgpu_get_dissolution_caps(self.ctx, capi.dptr(rs_cap), capi.dptr(rv_cap)))
        return rs_cap, rv_cap

    def setDissolutionCaps(self, rs_cap=None, rv_cap=None):
        """the caps themselves (restart; tests); None leaves a plane as it is"""
        a = None if rs_cap is None else capi.f64(rs_cap)
        b = None if rv_cap is None else capi.f64(rv_cap)
        self._chk(self.lib.opmgpu_set_dissolution_caps(self.ctx, None if a is None else capi.dptr(a), None if b is None else capi.dptr(b)))

    # Rock regions and irreversible compaction (opmgpu_set_rock_regions; the rule is ours and stated in include/opmgpu.h)
    rock_regions = None             # the regions in force (an object with mode, rocknum, rock_pref, rock_comp, tab_ptr, tab_p, tab_pvmult, tab_transmult); None = none

    def setRockRegions(self, regions):
        """A rock per cell and the compaction mode.  `regions`: an object with mode (capi.ROCK_REVERSIBLE / ROCK_IRREVERSIBLE), rocknum
        ([nc], 0-based), rock_pref and rock_comp ([nregions]), tab_ptr ([nregions + 1]; 0 rows = the ROCK form) and tab_p, tab_pvmult,
        tab_transmult -- opmgpu.decks.RockRegions -- or None to go back to the one rock of the tables.  With ROCK_IRREVERSIBLE saveState()
        takes every saved state into the history; the caller seeds it once with updateRockHistory() on the initial state.  ValueError
        with the library's text when refused; the previous set stays in force."""
        if regions is None:
            self._chk(self.lib.opmgpu_set_rock_regions(self.ctx, None))
            self.rock_regions = None
            return
        rocknum = np.asarray(regions.rocknum)
        if rocknum.shape != (self.nc,):
            raise ValueError("setRockRegions: rocknum has %s entries for %d cells" % (rocknum.shape, self.nc))
        pref, comp = capi.f64(regions.rock_pref), capi.f64(regions.rock_comp)
        ptr = capi.i32(regions.tab_ptr)
        if pref.shape != comp.shape or ptr.size != pref.size + 1:
            raise ValueError("setRockRegions: rock_pref, rock_comp [nregions] and tab_ptr [nregions + 1] differ in length")
        tabs = [capi.f64(np.concatenate([np.asarray(a, float).ravel(), np.zeros(1)])) for a in (regions.tab_p, regions.tab_pvmult, regions.tab_transmult)]
        rows = int(ptr[-1]) if ptr.size else 0
        if any(t.size - 1 != tabs[0].size - 1 for t in tabs) or (ptr.size and rows > tabs[0].size - 1):
            raise ValueError("setRockRegions: tab_p, tab_pvmult, tab_transmult differ in length or are shorter than tab_ptr says")
        s = capi.RockRegionsSpec()
        s.nregions, s.mode = int(pref.size), int(regions.mode)
        rn = capi.i32(rocknum)
        s.rocknum, s.rock_pref, s.rock_comp, s.tab_ptr = capi.iptr(rn), capi.dptr(pref), capi.dptr(comp), capi.iptr(ptr)
        s.tab_p, s.tab_pvmult, s.tab_transmult = (capi.dptr(t) for t in tabs)
        self._chk(self.lib.opmgpu_set_rock_regions(self.ctx, C.byref(s)))
        self.rock_regions = regions

    def updateRockHistory(self):
        """p_min = min(p_min, p) of the resident state, on the device"""
        self._chk(self.lib.opmgpu_update_rock_history(self.ctx))

    def rockHistory(self):
        """p_min per cell, caller cell order; +inf = no pressure taken yet (or no regions)"""
        out = np.zeros(self.nc)
        self._chk(self.lib.opmgpu_get_rock_history(self.ctx, capi.dptr(out)))
        return out

    def setRockHistory(self, p_min):
        """the history itself (restart; tests)"""
        a = capi.f64(p_min)
        if a.shape != (self.nc,):
            raise ValueError("setRockHistory: %s values for %d cells" % (a.shape, self.nc))
        self._chk(self.lib.opmgpu_set_rock_history(self.ctx, capi.dptr(a)))

    def rockMultipliers(self):
        """(pv_mult, trans_mult) of every cell at the resident state, caller cell order"""
        pv, tr = np.zeros(self.nc), np.zeros(self.nc)
        self._chk(self.lib.opmgpu_get_rock_multipliers(self.ctx, capi.dptr(pv), capi.dptr(tr)))
        return pv, tr

    # Analytic aquifers (opmgpu_set_aquifers; the rule is ours and stated in include/opmgpu.h)
    aquifers = None                 # the list in force (objects with kind, p_a0, datum, ... cells, alpha: opmgpu.deck.Aquifer); None = none
    _aquifer_step_begun = False

    def setAquifers(self, aquifers):
        """Fetkovich / Carter-Tracy aquifers as source terms of the water equation.  `aquifers`: a sequence of objects with kind
        (capi.AQUIFER_FETKOVICH / AQUIFER_CARTER_TRACY), p_a0, datum, CtV0, J (Fetkovich) or beta, Tc, td, pd (Carter-Tracy), cells and
        alpha (fractions summing to 1) -- opmgpu.deck.Aquifer -- or None / empty to remove them.  A new set starts with W_e = W_s = t =
        0.  prepareStep(dt) then begins every time step, saveState() commits a converged one, restoreState() discards a failed one.
        ValueError with the library's text when refused; the previous set stays in force."""
        aq = list(aquifers or ())
        if not aq:
            self._chk(self.lib.opmgpu_set_aquifers(self.ctx, None))
            self.aquifers, self._aquifer_step_begun = None, False
            return
        s = capi.AquifersSpec()
        ct = [a.kind == capi.AQUIFER_CARTER_TRACY for a in aq]
        tabs = [np.asarray(a.td, float) if c else np.zeros(0) for a, c in zip(aq, ct)]
        for a, c, t in zip(aq, ct, tabs):
            if c and np.asarray(a.pd, float).shape != t.shape:
                raise ValueError("setAquifers: t_D and P_D of an influence table differ in length")
        keep = dict(kind=capi.i32([a.kind for a in aq]), p_a0=capi.f64([a.p_a0 for a in aq]), datum=capi.f64([a.datum for a in aq]),
                    CtV0=capi.f64([0.0 if c else a.CtV0 for a, c in zip(aq, ct)]), J=capi.f64([0.0 if c else a.J for a, c in zip(aq, ct)]),
                    beta=capi.f64([a.beta if c else 0.0 for a, c in zip(aq, ct)]), Tc=capi.f64([a.Tc if c else 0.0 for a, c in zip(aq, ct)]),
                    tab_ptr=capi.i32(np.concatenate([[0], np.cumsum([t.size for t in tabs])])),
                    tab_td=capi.f64(np.concatenate(tabs + [np.zeros(1)])),
                    tab_pd=capi.f64(np.concatenate([np.asarray(a.pd, float) if c else np.zeros(0) for a, c in zip(aq, ct)] + [np.zeros(1)])),
                    conn_ptr=capi.i32(np.concatenate([[0], np.cumsum([len(a.cells) for a in aq])])),
                    conn_cell=capi.i32(np.concatenate([np.asarray(a.cells, np.int64) for a in aq] + [np.zeros(1, np.int64)])),
                    conn_alpha=capi.f64(np.concatenate([np.asarray(a.alpha, float) for a in aq] + [np.zeros(1)])))
        for a in aq:
            if len(a.cells) != len(a.alpha):
                raise ValueError("setAquifers: %d fractions for %d connected cells" % (len(a.alpha), len(a.cells)))
        s.naq = len(aq)
        for k, v in keep.items():
            setattr(s, k, capi.iptr(v) if v.dtype == np.int32 else capi.dptr(v))
        self._chk(self.lib.opmgpu_set_aquifers(self.ctx, C.byref(s)))
        self.aquifers, self._aquifer_step_begun = aq, False

    def aquiferState(self):
        """(W_e, W_s, t, p_a) per aquifer: cumulative reservoir and surface volume of influx, aquifer time, and the aquifer pressure they imply"""
        n = len(self.aquifers or ())
        out = [np.zeros(max(n, 1)) for _ in range(4)]
        self._chk(self.lib.opmgpu_aquifer_state_get(self.ctx, *[capi.dptr(a) for a in out]))
        return tuple(a[:n] for a in out)

    def setAquiferState(self, W_e=None, W_s=None, t=None):
        """the committed aquifer state (restart; tests); None leaves a column as it is.  A begun step is discarded."""
        arr = [None if v is None else capi.f64(v) for v in (W_e, W_s, t)]
        n = len(self.aquifers or ())
        for a in arr:
            if a is not None and a.shape != (n,):
                raise ValueError("setAquiferState: one value per aquifer (%d aquifers)" % n)
        self._chk(self.lib.opmgpu_aquifer_state_set(self.ctx, *[capi.dptr(a) for a in arr]))
        self._aquifer_step_begun = False

    def aquiferConnections(self):
        """[nconn][6] of the begun step, connections in the listing order: rho0, p0, A, B and, at the resident state, q and qs = b_w q"""
        n = sum(len(a.cells) for a in (self.aquifers or ()))
        out = np.zeros((max(n, 1), capi.AQUIFER_CONN_K))
        self._chk(self.lib.opmgpu_aquifer_connections_get(self.ctx, capi.dptr(out)))
        return out[:n]

    # hysteresis history (SaturationPropsFromDeck::updateSatHyst, called once per report step: SimulatorBase_impl.hpp:190-191)
    def updateHysteresis(self):
        self._chk(self.lib.opmgpu_update_hysteresis(self.ctx))

    def getHysteresis(self):
        """(krnSwMdc_ow, krnSwMdc_go, delta_ow, delta_go), caller cell order"""
        out = [np.zeros(self.nc) for _ in range(4)]
        self._chk(self.lib.opmgpu_get_hysteresis(self.ctx, *[capi.dptr(a) for a in out]))
        return out

    def setHysteresis(self, mdc_ow, mdc_go):
        self._chk(self.lib.opmgpu_set_hysteresis(self.ctx, capi.dptr(capi.f64(mdc_ow)), capi.dptr(capi.f64(mdc_go))))

    def setHysteresisModel(self, model, killough_a=0.1):
        """EHYSTR item 2 / item 4 (opmgpu_set_hysteresis_model, the rule is stated in include/opmgpu.h): capi.HYST_CARLSON, the default
        of every context, or capi.HYST_KILLOUGH with Killough's curvature parameter.  ValueError with the library's text when refused."""
        self._chk(self.lib.opmgpu_set_hysteresis_model(self.ctx, int(model), float(killough_a)))

    def getHysteresisScanning(self):
        """(Sncrt_ow, m_ow, R_ow, Sncrt_go, m_go, R_go) of the scanning curves in force, caller cell order"""
        out = [np.zeros(self.nc) for _ in range(6)]
        self._chk(self.lib.opmgpu_get_hysteresis_scanning(self.ctx, *[capi.dptr(a) for a in out]))
        return out

    def setSolvePrecision(self, single_precision=None):
        """residual_.singlePrecision = dt < maxSinglePrecisionTimeStep (:284), told to the device BEFORE the assembly so that
        the Jacobian is written in the solve's precision."""
        if single_precision is None:
            single_precision = self.referencePrecision()
        self._chk(self.lib.opmgpu_set_solve_precision(self.ctx, int(bool(single_precision))))

    def stabilizeUpdate(self, relax_type, omega):
        self._chk(self.lib.opmgpu_stabilize_update(self.ctx, int(relax_type), float(omega)))

    def nonlinearIteration(self, iteration, single_precision=None, nonlinear_solver=None):
        """nonlinearIteration (BlackoilModelBase_impl.hpp:239-326). Returns (converged, linear_iterations).
        With a `NonlinearSolver` the update is stabilised exactly like the reference's use_update_stabilization path."""
        ns = nonlinear_solver
        if self.fused_iteration and ns is not None:
            return self._fused_iteration(iteration, single_precision, ns)
        if iteration == 0:
            self.residual_norms_history, self.current_relaxation = [], 1.0
        self.setSolvePrecision(single_precision)
        self.assemble(iteration == 0)
        converged = self.getConvergence()
        self.residual_norms_history.append(list(self.linf))          # computeResidualNorms (:1551-1589)
        lin = 0
        if not converged or iteration < (ns.min_iter if ns else 1):
            self.solveJacobianSystem(single_precision=single_precision)
            lin = self.linear_iterations
            if ns is not None and self.use_update_stabilization:
                oscillate, _ = ns.detectOscillations(self.residual_norms_history, iteration)
                if oscillate:
                    self.current_relaxation = max(self.current_relaxation - ns.relax_increment, ns.relax_max)
                self.stabilizeUpdate(ns.relax_type, self.current_relaxation)
            self.updateState()
        return converged, lin

    # the same iteration through ONE library call (opmgpu_nonlinear_iteration): the host round trips between the phases stay inside the
    # library.  Off by default here (the call-by-call sequence above is what the parity tests walk); bench.py switches it on.
    fused_iteration = False

    def _fused_iteration(self, iteration, single_precision, ns):
        if single_precision is None:
            single_precision = self.referencePrecision()
        ctl = capi.NewtonCtl(int(ns.min_iter), int(self.use_update_stabilization), int(ns.relax_type), float(ns.relax_max), float(ns.relax_increment),
                             float(ns.relax_rel_tol))
        conv, lin, relax = C.c_int(0), C.c_int(0), C.c_double(1.0)
        linf = np.zeros(3)
        st = self.lib.opmgpu_nonlinear_iteration(self.ctx, self.dt, int(iteration), int(bool(single_precision)), C.byref(ctl), C.byref(conv), C.byref(lin),
                                                 capi.dptr(linf), C.byref(relax))
        self.linear_iterations, self.linf, self.current_relaxation = lin.value, linf, relax.value
        self._chk(st)
        return bool(conv.value), lin.value

    # --- parity / bench helpers --------------------------------------------------------------
    def residual(self):
        r = np.zeros(3 * self.nc)
        self._chk(self.lib.opmgpu_get_residual(self.ctx, capi.dptr(r)))
        return r

    def jacobian(self):
        n = C.c_int32(0)
        self._chk(self.lib.opmgpu_get_jacobian_nnzb(self.ctx, C.byref(n)))
        rowptr, col, val = np.zeros(self.nc + 1, np.int32), np.zeros(n.value, np.int32), np.zeros((n.value, 9))
        self._chk(self.lib.opmgpu_get_jacobian_bsr(self.ctx, capi.iptr(rowptr), capi.iptr(col), capi.dptr(val)))
        return rowptr, col, val

    def jacobianFloatCopy(self):
        """mixed precision: the float copy of the double Jacobian written with the last assembly, widened, in jacobian()'s block order
        (opmgpu_get_jacobian_float_copy; ValueError when the context holds none at the moment)"""
        n = C.c_int32(0)
        self._chk(self.lib.opmgpu_get_jacobian_nnzb(self.ctx, C.byref(n)))
        val = np.zeros((n.value, 9))
        self._chk(self.lib.opmgpu_get_jacobian_float_copy(self.ctx, capi.dptr(val)))
        return val

    def spmv(self, x3):
        """y = J x with the assembled system (block-interleaved [nc][3]); with device wells J includes their factored
        Schur complement (the rank-7 operator per well), i.e. the operator the linear solver sees."""
        y = np.zeros(3 * self.nc)
        self._chk(self.lib.opmgpu_spmv(self.ctx, capi.dptr(capi.f64(x3)), capi.dptr(y)))
        return y

    def vfp_evaluate(self, table, q, thp, alq, bhp_in):
        """diagnostic: the device's VFP evaluators on table number `table` of the tables set: (bhp [n], d bhp / d q [n, 3], thp of bhp_in [n])"""
        q, thp, alq, bhp_in = (capi.f64(a) for a in (q, thp, alq, bhp_in))
        n = thp.size
        assert q.size == 3 * n and alq.size == n and bhp_in.size == n
        bhp, dq, thp_out = np.zeros(n), np.zeros((n, 3)), np.zeros(n)
        self._status(self.lib.opmgpu_vfp_evaluate(self.ctx, int(table), n, capi.dptr(q), capi.dptr(thp), capi.dptr(alq), capi.dptr(bhp_in),
                                                  capi.dptr(bhp), capi.dptr(dq), capi.dptr(thp_out)))
        return bhp, dq, thp_out

    def perfProps(self, nperf):
        out = np.zeros((nperf, capi.PERF_K))
        self._chk(self.lib.opmgpu_perf_props(self.ctx, capi.dptr(out)))
        return out

    def perfPvtAt(self, press):
        """b (nperf x 3), rsSat, rvSat of the perforated cells at the given pressures (opmgpu_perf_pvt) -- what the host well
        model's computeWellConnectionPressures needs (StandardWells_impl.hpp:218-296)"""
        press = capi.f64(press)
        out = np.zeros((press.size, 5))
        self._chk(self.lib.opmgpu_perf_pvt(self.ctx, capi.dptr(press), capi.dptr(out)))
        return out[:, :3], out[:, 3].copy(), out[:, 4].copy()

    def averageB(self):
        """B_avg of getWellConvergence for the host well model's pre-solve (opmgpu_average_b)"""
        B = np.zeros(3)
        self._chk(self.lib.opmgpu_average_b(self.ctx, capi.dptr(B)))
        return B

    def addWellTerms(self, resid_delta, rc, blocks):
        rc = capi.i32(rc)
        nblk = rc.size // 2
        self._chk(self.lib.opmgpu_add_well_terms(self.ctx, capi.dptr(capi.f64(resid_delta)), nblk, capi.iptr(rc), capi.dptr(capi.f64(blocks))))

    def addWellRhs(self, rhs_delta):
        self._chk(self.lib.opmgpu_add_well_rhs(self.ctx, capi.dptr(capi.f64(rhs_delta))))

    def perfDx(self, nperf):
        out = np.zeros((nperf, 3))
        self._chk(self.lib.opmgpu_perf_dx(self.ctx, capi.dptr(out)))
        return out

    def timings(self):
        a, s, u = C.c_double(0), C.c_double(0), C.c_double(0)
        self.lib.opmgpu_last_timings(self.ctx, C.byref(a), C.byref(s), C.byref(u))
        return a.value, s.value, u.value

    def time_kernel(self, kernel, reps=20):
        ms = C.c_double(0)
        self._chk(self.lib.opmgpu_time_kernel(self.ctx, kernel, reps, C.byref(ms)))
        return ms.value

    def ordering(self):
        pos, lev = np.zeros(self.nc, np.int32), np.zeros(self.nc, np.int32)
        nl = C.c_int32(0)
        self._chk(self.lib.opmgpu_get_ordering(self.ctx, capi.iptr(pos), capi.iptr(lev), C.byref(nl)))
        return pos, lev, nl.value


class NonlinearSolver:
    """NonlinearSolver (NonlinearSolver_impl.hpp:119-301): step loop, oscillation detection, relaxation parameters."""

    def __init__(self, max_iter=10, min_iter=1, relax_type=capi.RELAX_DAMPEN, relax_max=0.5, relax_increment=0.1, relax_rel_tol=0.2):
        self.max_iter, self.min_iter = max_iter, min_iter               # SolverParameters::reset (:183-192)
        self.relax_type, self.relax_max, self.relax_increment, self.relax_rel_tol = relax_type, relax_max, relax_increment, relax_rel_tol

    def detectOscillations(self, norms, it):
        """The rule of NonlinearSolver::detectOscillations (:221-257) -> (oscillate, stagnate); only the three mass-balance norms take part.
        A phase "swings" when its norm is back within relax_rel_tol (relative to the newest value) of its value two iterations ago but not
        of last iteration's; two swinging phases = oscillation.  Stagnation = no phase moved by more than 0.1 % between the two previous
        iterations."""
        if it < 2:
            return False, False
        now, last, before = norms[it], norms[it - 1], norms[it - 2]
        swinging, any_moved = 0, False
        with np.errstate(divide="ignore", invalid="ignore"):
            for ph in range(3):
                to_before = abs(np.float64(now[ph] - before[ph]) / now[ph])
                to_last = abs(np.float64(now[ph] - last[ph]) / now[ph])
                swinging += int(to_before < self.relax_rel_tol < to_last)
                any_moved = any_moved or bool(abs(np.float64(last[ph] - before[ph]) / before[ph]) > 1.0e-3)
        return swinging >= 2, not any_moved

    def step(self, model, single_precision=None):
        """(:119-174). Returns (newton_iterations, linear_iterations); raises TooManyIterations."""
        it, lin_total = 0, 0
        while True:
            converged, lin = model.nonlinearIteration(it, single_precision=single_precision, nonlinear_solver=self)
            lin_total += lin
            it += 1
            if not ((not converged and it <= self.max_iter) or it <= self.min_iter):
                break
        if not converged:
            raise TooManyIterations("Solver convergence failure - Failed to complete a time step within %d iterations." % self.max_iter)
        return it, lin_total


def newton_step(model, max_iter=10, min_iter=1):
    """NonlinearSolver::step (NonlinearSolver_impl.hpp:119-174) with use_update_stabilization=false (plain Newton).
    Returns (newton_iterations, linear_iterations)."""
    it, lin_total = 0, 0
    while True:
        converged, lin = model.nonlinearIteration(it)
        lin_total += lin
        it += 1
        if not ((not converged and it <= max_iter) or it <= min_iter):
            break
    if not converged:
        raise TooManyIterations("Failed to complete a time step within %d iterations." % max_iter)
    return it, lin_total
