// opmgpu.hpp -- C++ host-side mirror of the reference's plug-in interfaces over the C ABI (include/opmgpu.h).
//
// Header-only, no OPM / Eigen / Dune dependency: these are the classes a flow_legacy maintainer derives
// the real adaptors from (INTEGRATION.md shows the OPM-side glue).  Names, call order and error
// behaviour follow the reference:
//   opmgpu::NewtonIterationBlackoilGpu   <->  Opm::NewtonIterationBlackoilInterface
//                                             (opm/autodiff/NewtonIterationBlackoilInterface.hpp:31-52)
//   opmgpu::BlackoilModelGpu             <->  Opm::BlackoilModelBase hooks
//                                             (opm/autodiff/BlackoilModelBase_impl.hpp:222-326)
//   opmgpu::NonlinearSolverGpu::step     <->  Opm::NonlinearSolver::step (NonlinearSolver_impl.hpp:119-174)
// Status codes of the C ABI become the exception types the reference's AdaptiveTimeStepping catches
// (AdaptiveTimeStepping_impl.hpp:244-281).
#ifndef OPMGPU_HOST_HPP
#define OPMGPU_HOST_HPP

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/opmgpu.h"

namespace opmgpu {

struct NumericalIssue : std::runtime_error { using std::runtime_error::runtime_error; };        // Opm::NumericalIssue
struct LinearSolverProblem : std::runtime_error { using std::runtime_error::runtime_error; };   // Opm::LinearSolverProblem
struct ISTLError : std::runtime_error { using std::runtime_error::runtime_error; };             // Dune::ISTLError / MatrixBlockError
struct TooManyIterations : std::runtime_error { using std::runtime_error::runtime_error; };     // Opm::TooManyIterations

inline void throw_on_status(const opmgpu_ctx* ctx, int st)
{
    if (st == OPMGPU_OK) return;
    const std::string msg = ctx ? opmgpu_last_error(ctx) : "";
    switch (st) {
    case OPMGPU_ENUMERICAL: throw NumericalIssue(msg);
    case OPMGPU_ELINSOLVE:  throw LinearSolverProblem(msg);
    case OPMGPU_EBREAKDOWN:
    case OPMGPU_ESINGULAR:  throw ISTLError(msg);
    case OPMGPU_EINVAL:     throw std::logic_error("opmgpu: invalid argument: " + msg);
    default:                throw std::runtime_error("opmgpu status " + std::to_string(st) + ": " + msg);
    }
}

/// BCRSMatrix<MatrixBlock<Scalar,3,3>> + BlockVector handed over as plain arrays
/// (what formInterleavedSystem produces, NewtonIterationBlackoilInterleaved.cpp:110-194, 263-269).
struct BsrSystem {
    int nb = 0;
    std::vector<int32_t> rowptr, col;      // columns ascending per row, diagonal present
    std::vector<double> val9;              // nnzb * 9, row-major blocks  A[row][col][eq][var]
    std::vector<double> rhs3;              // nb * 3, block-interleaved
    bool singlePrecision = false;          // LinearisedBlackoilResidual::singlePrecision
};

/// B1: drop-in for NewtonIterationBlackoilInterleaved's solve stage.
class NewtonIterationBlackoilGpu {
public:
    explicit NewtonIterationBlackoilGpu(const opmgpu_params* prm = nullptr, int device = 0)
    {
        const int st = opmgpu_create_solver(&ctx_, device, prm);
        if (st != OPMGPU_OK) throw std::runtime_error("opmgpu_create_solver failed (no GPU? there is no CPU fallback), status " + std::to_string(st));
    }
    ~NewtonIterationBlackoilGpu() { opmgpu_destroy(ctx_); }
    NewtonIterationBlackoilGpu(const NewtonIterationBlackoilGpu&) = delete;
    NewtonIterationBlackoilGpu& operator=(const NewtonIterationBlackoilGpu&) = delete;

    /// x (nb*3, block-interleaved) with J x = rhs; const like the reference's (mutable internals, :75-79)
    std::vector<double> computeNewtonIncrement(const BsrSystem& sys) const
    {
        std::vector<double> x(size_t(3) * sys.nb, 0.0);
        const int st = opmgpu_solve_bsr(ctx_, sys.nb, sys.rowptr.data(), sys.col.data(), sys.val9.data(), sys.rhs3.data(),
                                        sys.singlePrecision ? 1 : 0, x.data(), &iterations_, &reduction_);
        throw_on_status(ctx_, st);
        return x;
    }
    int iterations() const { return iterations_; }                   // NewtonIterationBlackoilInterface::iterations
    double reduction() const { return reduction_; }
    opmgpu_ctx* handle() const { return ctx_; }

private:
    mutable opmgpu_ctx* ctx_ = nullptr;
    mutable int iterations_ = 0;
    mutable double reduction_ = 0.0;
};

/// ReservoirState view (opm/core/simulator/BlackoilState.hpp:40-90)
struct ReservoirStateView {
    double* pressure; double* saturation; double* gasoilratio; double* rv; int8_t* hydroCarbonState;
};

struct ConvergenceReport { double B_avg[3], CNV[3], MB[3], linf[3]; bool converged; };

/// B2: the BlackoilModel hooks on the device.  The context outlives the model object like the reference's
/// linear solver outlives BlackoilModel (FlowMain.hpp:237 vs SimulatorBase_impl.hpp:201-203).
class BlackoilModelGpu {
public:
    /// grid.trans must be finite and >= 0 (0 is legal and closes the connection): a negative, NaN or infinite value is
    /// OPMGPU_EINVAL at opmgpu_create, and the message thrown here names the connection.
    BlackoilModelGpu(const opmgpu_grid& grid, const opmgpu_tables& tables, const opmgpu_params* prm = nullptr, int device = 0)
    {
        nc_ = grid.nc;
        nconn_ = grid.nconn;
        use_cpr_ = prm && prm->use_cpr;
        const int st = opmgpu_create(&ctx_, device, &grid, &tables, prm);
        if (st != OPMGPU_OK) throw std::runtime_error("opmgpu_create failed (no GPU? there is no CPU fallback), status " + std::to_string(st) + ": " + opmgpu_last_error(nullptr));
    }
    ~BlackoilModelGpu() { opmgpu_destroy(ctx_); }
    BlackoilModelGpu(const BlackoilModelGpu&) = delete;
    BlackoilModelGpu& operator=(const BlackoilModelGpu&) = delete;

    int numPhases() const { return 3; }
    void setWells(int nw, const int32_t* well_connpos, const int32_t* well_cells) { throw_on_status(ctx_, opmgpu_set_wells(ctx_, nw, well_connpos, well_cells)); }

    /// wells on the device (StandardWells restated in csrc/wells.hip): topology + controls, then the WellState fields
    void setDeviceWells(const opmgpu_wells& wells) { throw_on_status(ctx_, opmgpu_set_device_wells(ctx_, &wells)); device_wells_ = wells.nw > 0; }
    /// WEFAC: one efficiency factor in (0, 1] per device well (order of setDeviceWells), empty = all ones.  The perforated cells see e_w times the
    /// well's rates and their derivatives (StandardWells_impl.hpp:1405-1434, BlackoilModelBase_impl.hpp:953-975); the well equations do not.
    /// After setDeviceWells, which resets the factors to ones; lasts through saved states, precision changes and re-plans.
    void setWellEfficiencyFactors(const std::vector<double>& factors) { throw_on_status(ctx_, opmgpu_set_well_efficiency(ctx_, factors.empty() ? nullptr : factors.data())); }
    /// Group rate control shared by guide rates (opmgpu_set_well_groups; the sharing rule is stated in include/opmgpu.h): members of group g are
    /// group_wells[group_ptr[g] .. group_ptr[g+1]) with their guide rates in the same positions; sign -1 production / +1 injection, target in SI,
    /// distr[3 g ..] the phase weights.  Every member's last control is the group slot.  An empty group_ptr removes the groups.  After
    /// setDeviceWells, which removes them; lasts through saved states, precision changes and re-plans.
    void setWellGroups(const std::vector<int32_t>& group_ptr, const std::vector<int32_t>& group_wells, const std::vector<double>& sign,
                       const std::vector<double>& target, const std::vector<double>& distr, const std::vector<double>& guide)
    {
        const int ng = group_ptr.empty() ? 0 : int(group_ptr.size()) - 1;
        throw_on_status(ctx_, opmgpu_set_well_groups(ctx_, ng, group_ptr.data(), group_wells.data(), sign.data(), target.data(), distr.data(), guide.data()));
    }
    /// {slot targets [nw] (NaN for a well in no group), group rates [ngroups]} the rule gives for the well state as it stands
    std::pair<std::vector<double>, std::vector<double>> wellGroupTargets(int nw, int ngroups) const
    {
        std::vector<double> t(nw > 0 ? nw : 1, 0.0), r(ngroups > 0 ? ngroups : 1, 0.0);
        throw_on_status(ctx_, opmgpu_get_well_group_targets(ctx_, t.data(), r.data()));
        t.resize(nw > 0 ? nw : 0); r.resize(ngroups > 0 ? ngroups : 0);
        return { t, r };
    }
    // {cells perforated by more than one well, most wells in one cell}; {0, 0} without shared cells (opmgpu_well_shared_cells)
    std::pair<int, int> wellSharedCells() const { int32_t rows = 0, most = 0; throw_on_status(ctx_, opmgpu_well_shared_cells(ctx_, &rows, &most)); return { int(rows), int(most) }; }
    std::vector<double> wellEfficiencyFactors(int nw) const { std::vector<double> f(nw > 0 ? nw : 1, 1.0); throw_on_status(ctx_, opmgpu_get_well_efficiency(ctx_, f.data())); f.resize(nw > 0 ? nw : 0); return f; }
    void setWellState(const double* bhp, const double* well_rates, const double* perf_press = nullptr, const double* perf_rates = nullptr) { throw_on_status(ctx_, opmgpu_well_state_set(ctx_, bhp, well_rates, perf_press, perf_rates)); }
    void getWellState(double* bhp, double* well_rates, double* perf_press = nullptr, double* perf_rates = nullptr) { throw_on_status(ctx_, opmgpu_well_state_get(ctx_, bhp, well_rates, perf_press, perf_rates)); }
    /// WellStateFullyImplicitBlackoil::currentControls() / thp(); after an assembly also what solveWellEq did (iterations, converged) per well
    void setWellControls(const int32_t* current, const double* thp = nullptr) { throw_on_status(ctx_, opmgpu_well_controls_set(ctx_, current, thp)); }
    void getWellControls(int32_t* current, double* thp = nullptr, int32_t* presolve_iterations = nullptr, int32_t* presolve_converged = nullptr)
    {
        throw_on_status(ctx_, opmgpu_well_controls_get(ctx_, current, thp, presolve_iterations, presolve_converged));
    }
    /// VFPPROD / VFPINJ tables for THP controls (VFPProperties), before setDeviceWells
    void setVfpTables(int n, const opmgpu_vfp_table* tables) { throw_on_status(ctx_, opmgpu_set_vfp_tables(ctx_, n, tables)); }
    /// decomposed runs (after opmgpu_comm_init*, before the first CPR solve): 0 = rank-local pressure hierarchy, 1 = distributed (opmgpu.h)
    void setPressureHierarchy(int mode) { throw_on_status(ctx_, opmgpu_comm_set_pressure_hierarchy(ctx_, mode)); }
    /// once per report step, where SimulatorBase::run calls props.updateSatOilMax / updateSatHyst (SimulatorBase_impl.hpp:190-192)
    void updateSatOilMax() { throw_on_status(ctx_, opmgpu_update_sat_oil_max(ctx_)); }
    void updateSatHyst() { throw_on_status(ctx_, opmgpu_update_hysteresis(ctx_)); }
    /// EHYSTR item 2 / item 4: OPMGPU_HYST_CARLSON (the default) or OPMGPU_HYST_KILLOUGH with Killough's curvature parameter (opmgpu.h)
    void setHysteresisModel(int model, double killough_a = 0.1) { throw_on_status(ctx_, opmgpu_set_hysteresis_model(ctx_, model, killough_a)); }
    /// DRSDT / DRVDT (opmgpu_set_dissolution_limits; the rule is ours and stated in opmgpu.h): rates in 1/s, negative = off.  The caller
    /// begins every time step -- also the retry of a failed one with a shorter dt, after the state has been restored -- with
    /// beginDissolutionStep(dt), which takes the caps from the resident state.  The caps themselves for restart: [nc], any pointer may be null.
    void setDissolutionLimits(double drsdt, bool drsdt_free_only, double drvdt) { throw_on_status(ctx_, opmgpu_set_dissolution_limits(ctx_, drsdt, drsdt_free_only ? 1 : 0, drvdt)); }
    void beginDissolutionStep(double dt) { throw_on_status(ctx_, opmgpu_begin_dissolution_step(ctx_, dt)); }
    void getDissolutionCaps(double* rs_cap, double* rv_cap) { throw_on_status(ctx_, opmgpu_get_dissolution_caps(ctx_, rs_cap, rv_cap)); }
    void setDissolutionCaps(const double* rs_cap, const double* rv_cap) { throw_on_status(ctx_, opmgpu_set_dissolution_caps(ctx_, rs_cap, rv_cap)); }
    /// Rock regions and irreversible compaction (opmgpu_set_rock_regions; the rule is ours and stated in opmgpu.h): nullptr goes back to the
    /// one rock of the tables.  The caller runs updateRockHistory() once on the initial (or restarted) state and after every converged
    /// sub-step; save / restore do not touch the history.  History and multipliers: [nc], caller cell order; a multiplier pointer may be null.
    void setRockRegions(const opmgpu_rock_regions* regions) { throw_on_status(ctx_, opmgpu_set_rock_regions(ctx_, regions)); }
    void updateRockHistory() { throw_on_status(ctx_, opmgpu_update_rock_history(ctx_)); }
    void getRockHistory(double* p_min) { throw_on_status(ctx_, opmgpu_get_rock_history(ctx_, p_min)); }
    void setRockHistory(const double* p_min) { throw_on_status(ctx_, opmgpu_set_rock_history(ctx_, p_min)); }
    void getRockMultipliers(double* pv_mult, double* trans_mult) { throw_on_status(ctx_, opmgpu_get_rock_multipliers(ctx_, pv_mult, trans_mult)); }
    /// Analytic aquifers (opmgpu_set_aquifers; the rule is ours and stated in opmgpu.h): nullptr removes them.  The caller begins every
    /// time step -- also the retry of a failed one, after the state has been restored -- with beginAquiferStep(dt) and commits a
    /// converged one with commitAquiferStep() before it saves the state.  State per aquifer ([naq], any pointer may be null); the
    /// connections' record is [nconn][OPMGPU_AQUIFER_CONN_K].
    void setAquifers(const opmgpu_aquifers* aquifers) { throw_on_status(ctx_, opmgpu_set_aquifers(ctx_, aquifers)); }
    void beginAquiferStep(double dt) { throw_on_status(ctx_, opmgpu_aquifer_begin_step(ctx_, dt)); }
    void commitAquiferStep() { throw_on_status(ctx_, opmgpu_aquifer_commit_step(ctx_)); }
    void getAquiferState(double* W_e, double* W_s, double* t, double* p_a) { throw_on_status(ctx_, opmgpu_aquifer_state_get(ctx_, W_e, W_s, t, p_a)); }
    void setAquiferState(const double* W_e, const double* W_s, const double* t) { throw_on_status(ctx_, opmgpu_aquifer_state_set(ctx_, W_e, W_s, t)); }
    void getAquiferConnections(double* out) { throw_on_status(ctx_, opmgpu_aquifer_connections_get(ctx_, out)); }
    /// Sncrt, m, R of the oil-water and of the gas-oil scanning curves ([nc] each, any pointer may be null)
    void getHysteresisScanning(double* sncrt_ow, double* m_ow, double* r_ow, double* sncrt_go, double* m_go, double* r_go)
    {
        throw_on_status(ctx_, opmgpu_get_hysteresis_scanning(ctx_, sncrt_ow, m_ow, r_ow, sncrt_go, m_go, r_go));
    }
    /// BlackoilModelBase::nonlinearIteration + the NonlinearSolver's update stabilisation in ONE library call (opmgpu_nonlinear_iteration):
    /// the same sequence NonlinearSolverGpu::step issues call by call, without the host round trips between the phases.
    /// Returns true when the iteration found the step converged; throws like the single calls do.
    bool nonlinearIterationOneCall(int iteration, bool single_precision, const opmgpu_newton_ctl& ctl, int* linear_iterations = nullptr)
    {
        int conv = 0, lin = 0;
        throw_on_status(ctx_, opmgpu_nonlinear_iteration(ctx_, dt_, iteration, single_precision ? 1 : 0, &ctl, &conv, &lin, nullptr, nullptr));
        if (linear_iterations) *linear_iterations = lin;
        return conv != 0;
    }
    /// well part of getConvergence (:1769-1779)
    bool wellsConverged(const ConvergenceReport& r)
    {
        if (!device_wells_) return true;
        double flux[3], ctrl = 0.0;
        throw_on_status(ctx_, opmgpu_well_convergence(ctx_, flux, &ctrl));
        bool ok = ctrl < tolerance_well_control_;
        for (int a = 0; a < 3; ++a) ok = ok && (r.B_avg[a] * flux[a] < tolerance_wells_);
        return ok;
    }

    /// prepareStep (:222-232): remembers dt (pvdt = pv/dt is applied in assemble) and uploads the state
    void prepareStep(double dt, const ReservoirStateView& s)
    {
        dt_ = dt;
        throw_on_status(ctx_, opmgpu_set_state(ctx_, s.pressure, s.saturation, s.gasoilratio, s.rv, s.hydroCarbonState));
    }
    /// the next time step from the state that is resident on the device (AdaptiveTimeStepping's sub-steps)
    void prepareStep(double dt) { dt_ = dt; }
    void assemble(bool initial_assembly) { throw_on_status(ctx_, opmgpu_assemble(ctx_, dt_, initial_assembly ? 1 : 0, nullptr, nullptr, nullptr, nullptr, nullptr)); }
    ConvergenceReport getConvergence()
    {
        ConvergenceReport r; int conv = 0;
        const int st = opmgpu_convergence(ctx_, dt_, r.B_avg, r.CNV, r.MB, r.linf, &conv);
        r.converged = conv != 0;
        throw_on_status(ctx_, st);         // NumericalIssue on NaN / too large residual
        return r;
    }
    /// residual_.singlePrecision = dt < maxSinglePrecisionTimeStep (:284) is honoured by the interleaved solver only
    /// (NewtonIterationBlackoilInterleaved.cpp:478-480); the CPR plug-in computes in double whatever it says (NewtonIterationBlackoilCPR.cpp:117-140)
    bool referencePrecisionIsSingle() const { return !use_cpr_ && dt_ < max_single_precision_days_ * 86400.0; }
    /// solveJacobianSystem (:1139-1145)
    void solveJacobianSystem()
    {
        const int single = referencePrecisionIsSingle() ? 1 : 0;
        throw_on_status(ctx_, opmgpu_solve(ctx_, single, nullptr, &linear_iterations_, &linear_reduction_));
    }
    void updateState(double relax = 1.0) { throw_on_status(ctx_, opmgpu_update_state(ctx_, nullptr, relax)); }
    void downloadState(const ReservoirStateView& s) { throw_on_status(ctx_, opmgpu_get_state(ctx_, s.pressure, s.saturation, s.gasoilratio, s.rv, s.hydroCarbonState)); }

    /// nonlinearIteration (:239-326): assemble -> getConvergence -> [solve -> stabilise -> update].
    /// NonlinearSolverType supplies minIter / detectOscillations / relaxIncrement / relaxMax / relaxType like the reference's.
    template <class NonlinearSolverType>
    bool nonlinearIteration(int iteration, const NonlinearSolverType& nonlinear_solver)
    {
        if (iteration == 0) { residual_norms_history_.clear(); current_relaxation_ = 1.0; }    // dx_old is zeroed by the initial assembly
        throw_on_status(ctx_, opmgpu_set_solve_precision(ctx_, referencePrecisionIsSingle() ? 1 : 0));   // :284, before the assembly
        assemble(iteration == 0);
        ConvergenceReport r = getConvergence();
        r.converged = wellsConverged(r) && r.converged;
        residual_norms_history_.push_back({ r.linf[0], r.linf[1], r.linf[2] });               // computeResidualNorms (:1551-1589)
        const bool must_solve = (iteration < nonlinear_solver.minIter()) || !r.converged;
        if (must_solve) {
            solveJacobianSystem();
            if (use_update_stabilization_) {
                bool isOscillate = false, isStagnate = false;
                nonlinear_solver.detectOscillations(residual_norms_history_, iteration, isOscillate, isStagnate);
                if (isOscillate) current_relaxation_ = std::max(current_relaxation_ - nonlinear_solver.relaxIncrement(), nonlinear_solver.relaxMax());
                throw_on_status(ctx_, opmgpu_stabilize_update(ctx_, nonlinear_solver.relaxType(), current_relaxation_));
            }
            updateState();
        }
        return r.converged;
    }
    /// last_state of AdaptiveTimeStepping kept on the device, and BlackoilModelBase::relativeChange (:1595-1631) against it
    void saveState() { throw_on_status(ctx_, opmgpu_save_state(ctx_)); }
    void restoreState() { throw_on_status(ctx_, opmgpu_restore_state(ctx_)); }
    double relativeChange() { double v = 0.0; throw_on_status(ctx_, opmgpu_relative_change(ctx_, &v)); return v; }
    /// BlackoilModelBase::computeFluidInPlace(state, fipnum) (:2263-2445) for the resident state: values[region][7]
    std::vector<std::vector<double>> computeFluidInPlace(const std::vector<int>& fipnum)
    {
        int dims = 1;
        for (int f : fipnum) dims = std::max(dims, f);
        std::vector<int32_t> fn(fipnum.begin(), fipnum.end());
        std::vector<double> flat(std::size_t(dims) * 7, 0.0);
        throw_on_status(ctx_, opmgpu_compute_fluid_in_place(ctx_, fn.empty() ? nullptr : fn.data(), dims, nullptr, flat.data()));
        std::vector<std::vector<double>> values(dims, std::vector<double>(7));
        for (int r = 0; r < dims; ++r) for (int k = 0; k < 7; ++k) values[r][k] = flat[std::size_t(r) * 7 + k];
        return values;
    }
    /// BlackoilModelBase::setThresholdPressures (:421-443): the thresholds of all connections in the grid's connection order (faces, then
    /// NNCs); an empty vector removes them.  std::logic_error for a wrong size, a negative or a non-finite value.
    void setThresholdPressures(const std::vector<double>& threshold_pressures)
    {
        if (!threshold_pressures.empty() && int(threshold_pressures.size()) != nconn_)
            throw std::logic_error("Illegal size of threshold_pressures input, must be equal to number of faces + nncs");
        throw_on_status(ctx_, opmgpu_set_threshold_pressures(ctx_, threshold_pressures.empty() ? nullptr : threshold_pressures.data()));
    }
    /// PVCDO, the dead oil of constant compressibility (opmgpu_set_pvcdo; the rule is stated in opmgpu.h): one row p_ref, B_ref, C_o,
    /// mu_ref, C_v per PVT region, SI, flattened; an empty vector goes back to the tabulated oil.  std::logic_error for a context with
    /// dissolved gas, a non-finite entry, B_ref <= 0 or mu_ref <= 0.  The caller gives one row for each PVT region of the tables.
    void setPvcdo(const std::vector<double>& pvcdo)
    {
        if (pvcdo.size() % 5 != 0) throw std::logic_error("setPvcdo: five numbers per PVT region");
        throw_on_status(ctx_, opmgpu_set_pvcdo(ctx_, pvcdo.empty() ? nullptr : pvcdo.data()));
    }
    /// computeMaxDp (opm/simulators/thresholdPressures.hpp:46-298) for the resident state: max_dp[a][b] over the 1-based regions `eqlnum`,
    /// scanning the first n_face_conn connections (the grid faces); -1 = no face joins the pair.  dp_conn (optional): per connection.
    std::vector<std::vector<double>> computeMaxDp(const std::vector<int>& eqlnum, int nregions, int n_face_conn, std::vector<double>* dp_conn = nullptr)
    {
        if (int(eqlnum.size()) != nc_ || nregions < 1) throw std::logic_error("computeMaxDp: one region per cell and nregions >= 1");
        std::vector<int32_t> eq(eqlnum.begin(), eqlnum.end());
        std::vector<double> flat(std::size_t(nregions) * nregions, -1.0);
        if (dp_conn) dp_conn->assign(std::size_t(nconn_), 0.0);
        throw_on_status(ctx_, opmgpu_compute_max_dp(ctx_, eq.data(), nregions, n_face_conn, dp_conn ? dp_conn->data() : nullptr, flat.data()));
        std::vector<std::vector<double>> m(nregions, std::vector<double>(nregions));
        for (int a = 0; a < nregions; ++a) for (int b = 0; b < nregions; ++b) m[a][b] = flat[std::size_t(a) * nregions + b];
        return m;
    }
    /// BlackoilPropsAdFromDeck::setSwatInitScaling (BlackoilPropsAdFromDeck.cpp:1009-1019; the rule is stated in opmgpu.h): per cell the
    /// imposed water saturation and the target pcow = p_o - p_w; returns the saturation each cell ends at.  std::logic_error for a wrong
    /// size, a non-finite value or a saturation outside [0, 1].
    std::vector<double> setSwatInitScaling(const std::vector<double>& sw, const std::vector<double>& pcow)
    {
        if (int(sw.size()) != nc_ || int(pcow.size()) != nc_) throw std::logic_error("setSwatInitScaling: one saturation and one capillary pressure per cell");
        std::vector<double> sw_out(std::size_t(nc_), 0.0);
        throw_on_status(ctx_, opmgpu_set_swatinit_scaling(ctx_, sw.data(), pcow.data(), sw_out.data()));
        return sw_out;
    }
    /// each cell's current maximum oil-water capillary pressure (PCW, or the table maximum of its saturation region)
    std::vector<double> pcw()
    {
        std::vector<double> v(std::size_t(nc_), 0.0);
        throw_on_status(ctx_, opmgpu_get_pcw(ctx_, v.data()));
        return v;
    }
    /// BlackoilPropsAdFromDeck::capPress: [pcow | pcgo] x nc at the saturations `sat` ([nc][3]) or, nullptr, the resident state's
    std::vector<double> capPress(const std::vector<double>* sat = nullptr)
    {
        if (sat && int(sat->size()) != 3 * nc_) throw std::logic_error("capPress: three saturations per cell");
        std::vector<double> pc(2 * std::size_t(nc_), 0.0);
        throw_on_status(ctx_, opmgpu_cap_press(ctx_, sat ? sat->data() : nullptr, pc.data()));
        return pc;
    }
    /// BlackoilModelBase::getSimulatorData (sd_ of :662-683 and rq_[].b/rho/mu/kr) for the resident state: 16 per-cell arrays in SI under
    /// the names of SimulatorFullyImplicitBlackoilOutput.hpp:512-567, in the cell order of the state
    std::map<std::string, std::vector<double>> simulatorData()
    {
        static const char* const names[OPMGPU_SIMDATA_K] = { "1OVERBW", "1OVERBO", "1OVERBG", "WAT_DEN", "OIL_DEN", "GAS_DEN", "WAT_VISC", "OIL_VISC",
                                                             "GAS_VISC", "WATKR", "OILKR", "GASKR", "RSSAT", "RVSAT", "PBUB", "PDEW" };
        std::vector<double> flat(std::size_t(OPMGPU_SIMDATA_K) * nc_, 0.0);
        throw_on_status(ctx_, opmgpu_get_simulator_data(ctx_, flat.data()));
        std::map<std::string, std::vector<double>> sd;
        for (int k = 0; k < OPMGPU_SIMDATA_K; ++k) sd[names[k]].assign(flat.begin() + std::ptrdiff_t(k) * nc_, flat.begin() + std::ptrdiff_t(k + 1) * nc_);
        return sd;
    }
    void setStepLength(double dt) { dt_ = dt; }
    double relaxation() const { return current_relaxation_; }
    void setUseUpdateStabilization(bool on) { use_update_stabilization_ = on; }
    int linearIterationsLastSolve() const { return linear_iterations_; }
    opmgpu_ctx* handle() const { return ctx_; }

private:
    opmgpu_ctx* ctx_ = nullptr;
    int nc_ = 0;
    int nconn_ = 0;
    bool use_cpr_ = false;
    double dt_ = 0.0, max_single_precision_days_ = 20.0, linear_reduction_ = 0.0;
    int linear_iterations_ = 0;
    bool use_update_stabilization_ = true;              // BlackoilModelParameters.cpp:98
    bool device_wells_ = false;
    double tolerance_wells_ = 1e-4, tolerance_well_control_ = 1e-7;    // BlackoilModelParameters.cpp:88-89
    double current_relaxation_ = 1.0;
    std::vector<std::array<double, 3>> residual_norms_history_;
};

/// NonlinearSolver (NonlinearSolver_impl.hpp:119-301): step loop, oscillation detection, relaxation parameters
/// RateConverter::SurfaceToReservoirVoidage (RateConverterLegacy.hpp:407-770) over the resident state: defineState takes the regions'
/// sums from the library (collective in decomposed runs), calcCoeff evaluates the PVT tables on the device at the region's average state.
/// `region` empty = one region 0 of all cells, what SimulatorBase builds (SimulatorBase_impl.hpp:66) and asks for (:548).
class SurfaceToReservoirVoidageGpu {
public:
    SurfaceToReservoirVoidageGpu(opmgpu_ctx* ctx, const std::vector<int>& region = {}, int n_ranks = 1)
        : ctx_(ctx), n_ranks_(n_ranks)
    {
        ids_ = region;
        std::sort(ids_.begin(), ids_.end());
        ids_.erase(std::unique(ids_.begin(), ids_.end()), ids_.end());
        if (ids_.empty()) ids_.push_back(0);
        index_.reserve(region.size());
        for (int r : region) index_.push_back(int32_t(std::lower_bound(ids_.begin(), ids_.end(), r) - ids_.begin()));
        attr_.assign(ids_.size(), Attributes{ 0.0, 0.0, 0.0 });          // Attributes(): all zero (:684-692)
    }
    /// calcAverages (:718-768).  p is cleared before the loop, rs and rv are NOT (:733-737): they start from the previous call's averages
    /// (on every rank of a parallel run) -- restated as found.
    void defineState()
    {
        std::vector<double> sums(4 * ids_.size(), 0.0);
        throw_on_status(ctx_, opmgpu_region_state_sums(ctx_, index_.empty() ? nullptr : index_.data(), int(ids_.size()), sums.data()));
        for (std::size_t k = 0; k < ids_.size(); ++k) {
            const double n = sums[4 * k + 3];
            attr_[k].pressure = sums[4 * k + 0] / n;
            attr_[k].rs = (n_ranks_ * attr_[k].rs + sums[4 * k + 1]) / n;
            attr_[k].rv = (n_ranks_ * attr_[k].rv + sums[4 * k + 2]) / n;
        }
    }
    /// calcCoeff (:495-548): q_rT = sum_p coeff[p] q_s[p], phases water, oil, gas
    template <class Coeff> void calcCoeff(int r, int pvtRegionIdx, Coeff& coeff) const
    {
        const std::size_t k = std::size_t(std::lower_bound(ids_.begin(), ids_.end(), r) - ids_.begin());
        if (k >= ids_.size() || ids_[k] != r) throw std::invalid_argument("SurfaceToReservoirVoidageGpu::calcCoeff: unknown region");
        const int32_t reg = pvtRegionIdx;
        double c[3];
        throw_on_status(ctx_, opmgpu_voidage_coefficients(ctx_, 1, &attr_[k].pressure, &attr_[k].rs, &attr_[k].rv, &reg, c));
        for (int p = 0; p < 3; ++p) coeff[p] = c[p];
    }
    struct Attributes { double pressure, rs, rv; };
    const Attributes& attributes(int r) const { return attr_[std::size_t(std::lower_bound(ids_.begin(), ids_.end(), r) - ids_.begin())]; }

private:
    opmgpu_ctx* ctx_;
    int n_ranks_;
    std::vector<int> ids_;
    std::vector<int32_t> index_;
    std::vector<Attributes> attr_;
};

struct NonlinearSolverGpu {
    int max_iter = 10, min_iter = 1;                                          // SolverParameters::reset (:183-192)
    int relax_type = OPMGPU_RELAX_DAMPEN;
    double relax_max = 0.5, relax_increment = 0.1, relax_rel_tol = 0.2;
    int minIter() const { return min_iter; }
    int maxIter() const { return max_iter; }
    int relaxType() const { return relax_type; }
    double relaxMax() const { return relax_max; }
    double relaxIncrement() const { return relax_increment; }
    double relaxRelTol() const { return relax_rel_tol; }

    /// The rule of NonlinearSolver::detectOscillations (NonlinearSolver_impl.hpp:221-257) in this library's words.  A phase's residual norm
    /// "swings" when this iteration's value is back within relax_rel_tol of where it stood TWO iterations ago while it differs by more
    /// than that from LAST iteration's; the update oscillates when at least two of the three phases swing.  It stagnates when no phase's
    /// norm moved by more than 0.1 % between the two previous iterations.  All differences are relative (to the newest value for the
    /// swing test, to the oldest for the stagnation test).
    void detectOscillations(const std::vector<std::array<double, 3>>& norms, int it, bool& oscillate, bool& stagnate) const
    {
        oscillate = false; stagnate = false;
        if (it < 2) return;
        const std::array<double, 3>&now = norms[it], &last = norms[it - 1], &before = norms[it - 2];
        int swinging = 0;
        bool any_moved = false;
        for (int ph = 0; ph < 3; ++ph) {
            const double to_before = std::abs((now[ph] - before[ph]) / now[ph]);
            const double to_last = std::abs((now[ph] - last[ph]) / now[ph]);
            if (to_before < relax_rel_tol && relax_rel_tol < to_last) ++swinging;
            if (std::abs((last[ph] - before[ph]) / before[ph]) > 1.0e-3) any_moved = true;
        }
        oscillate = swinging >= 2;
        stagnate = !any_moved;
    }

    int step(BlackoilModelGpu& model) const
    {
        int iteration = 0; bool converged = false;
        do {
            converged = model.nonlinearIteration(iteration, *this);
            ++iteration;
        } while ((!converged && iteration <= max_iter) || iteration <= min_iter);
        if (!converged) throw TooManyIterations("Failed to complete a time step within " + std::to_string(max_iter) + " iterations.");
        return iteration;
    }
};

/// PIDTimeStepControl / AdaptiveSimulatorTimer (opm-core, not in the reference tree: restated) and
/// AdaptiveTimeStepping::stepImpl (AdaptiveTimeStepping_impl.hpp:183-372) around the device-resident Newton loop.
struct PIDTimeStepControl {
    double tol = 1e-1, errors[3] = { 1e-1, 1e-1, 1e-1 };
    int target_iterations = 0;                         // > 0: the "pid+iteration" variant
    double computeTimeStepSize(double dt, int iterations, double relative_change)
    {
        errors[0] = errors[1]; errors[1] = errors[2]; errors[2] = relative_change;
        for (double e : errors) if (!std::isfinite(e)) throw NumericalIssue("non-finite relative change in the time step control");
        double est;
        if (errors[2] > tol) est = dt * tol / errors[2];
        else est = dt * std::pow(errors[1] / errors[2], 0.075) * std::pow(tol / errors[2], 0.175) * std::pow(errors[0] * errors[0] / errors[1] / errors[2], 0.01);
        if (target_iterations > 0 && iterations > target_iterations) est *= double(target_iterations) / double(iterations);
        return est;
    }
};

struct AdaptiveTimeSteppingGpu {
    double restart_factor = 0.33, growth_factor = 2.0, max_growth = 3.0, max_time_step = 365.0 * 86400.0;     // :101-112
    int solver_restart_max = 10;
    double min_time_step_fraction = 1e-12;             // NOT in the reference: a failed sub-step shorter than this fraction of the report step ends it (the
                                                       // reference's loop resets its restart counter after every converged sub-step and can shrink for ever); 0 = off
    double suggested_next_timestep = 86400.0;
    PIDTimeStepControl control;
    std::vector<double> substeps;                      // of the last report step
    int failed_substeps = 0;

    static double clip(double est, double remaining, double max_step)        // AdaptiveSimulatorTimer::provideTimeStepEstimate
    {
        double dt = std::min(est, max_step);
        if (remaining > 0) {
            if (1.05 * dt > remaining) { dt = remaining; if (dt > max_step) dt = 0.5 * remaining; return dt; }
            if (1.5 * dt > remaining) dt = 0.5 * remaining;
        }
        return dt;
    }
    /// one report step of length `timestep` [s] from the model's resident state
    void step(double timestep, const NonlinearSolverGpu& solver, BlackoilModelGpu& model)
    {
        if (suggested_next_timestep < 0) suggested_next_timestep = restart_factor * timestep;
        double done = 0.0, dt = clip(suggested_next_timestep, timestep, max_time_step);
        model.saveState();
        substeps.clear();
        int restarts = 0;
        while (timestep - done > 1e-9 * std::max(1.0, timestep)) {
            bool converged = false; int linear = 0;
            try {
                model.setStepLength(dt);
                solver.step(model);
                linear = model.linearIterationsLastSolve();
                converged = true;
            }
            catch (const TooManyIterations&) {}
            catch (const LinearSolverProblem&) {}
            catch (const NumericalIssue&) {}
            catch (const std::runtime_error&) {}
            if (converged) {
                done += dt; substeps.push_back(dt);
                double est = std::min(control.computeTimeStepSize(dt, linear, model.relativeChange()), max_growth * dt);
                if (restarts > 0) { est = std::min(growth_factor * dt, est); restarts = 0; }
                dt = clip(est, timestep - done, max_time_step);
                model.saveState();
            } else {
                ++failed_substeps;
                if (min_time_step_fraction > 0 && dt < min_time_step_fraction * timestep) throw NumericalIssue("Solver failed to converge with a time step of " + std::to_string(dt) + " s: giving up.");
                if (restarts >= solver_restart_max) throw NumericalIssue("Solver failed to converge after cutting timestep " + std::to_string(restarts) + " times.");
                dt = clip(restart_factor * dt, timestep - done, max_time_step);
                model.restoreState();
                ++restarts;
            }
        }
        suggested_next_timestep = std::isfinite(dt) ? dt : timestep;
    }
};

} // namespace opmgpu
#endif
