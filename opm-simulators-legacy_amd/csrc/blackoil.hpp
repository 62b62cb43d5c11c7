// blackoil.hpp -- device-resident fully-implicit black-oil model (assembly, convergence, update).
//
// GPU replacement of BlackoilModelBase::{assemble, getConvergence, updateState}
// (opm/autodiff/BlackoilModelBase_impl.hpp:757-913, 1633-1857, 1147-1389) and of the Eigen
// AutoDiffBlock machinery underneath them: instead of O(100) sparse-matrix products per assembly
// the chain rule is applied per cell / per connection and the 3x3 blocks are written straight
// into the solver's SELL-64 matrix.
#ifndef OPMGPU_BLACKOIL_HPP
#define OPMGPU_BLACKOIL_HPP

#include "linsolver.hpp"

namespace opmgpu {

struct HystArgs;
struct CellPlanes;      // the resident state as a cell evaluator reads it (fluid_eval.hpp)
// The device form of the fluid tables: the caller's struct and, next to it, the per-segment slopes of its 1-D tables (TabX), every array
// in one blob of 8-byte words (BlackoilDevice::d_tab).  The pointer fields hold device pointers, or word offsets into the blob.
struct TabX {
    const double *swof_dkrw, *swof_dkrow, *swof_dpcow, *sgof_dkrg, *sgof_dkrog, *sgof_dpcgo;
    const double *oil_drs, *oil_dinvb_sat, *oil_dinvbmu_sat, *oil_col_dinvb, *oil_col_dinvbmu;
    const double *gas_drvsat, *gas_dinvb_sat, *gas_dinvbmu_sat, *gas_col_dinvb, *gas_col_dinvbmu;
    // PVCDO (opmgpu_set_pvcdo): [n_pvt_regions][5] rows p_ref, B_ref, C_o, mu_ref, C_v of the dead oil of constant compressibility, in the
    // blob behind everything else.  Not set: NULL in the device-pointer form (the evaluators off the Newton path branch on it), word 0 in
    // the offset form, where nobody reads it: the kernels that take that form are instantiated for the oil (KM_PVCDO).
    const double* oil_pvcdo;
};
// Rock regions (opmgpu_set_rock_regions) add NO field to the device form: while they are set nobody reads the one rock of opmgpu_tables,
// so its fields carry the regions instead (RockView in fluid_eval.hpp says how) -- every kernel's argument block, and with it the code of
// every instantiation a context without regions runs, is what it was.
// stone_som: Stone I's residual oil saturation Som = min(SOWCR, SOGCR) of every cell (internal numbering), a device pointer in EVERY form of
// the tables (it is no table: a per-cell plane that rides here so that each launch site of eval_cell sees it); null unless the model is
// OPMGPU_KRO_STONE1.  The model itself and the per-region exponent are t.threephase_model and t.stone1_exponent (in the blob).
struct DevTables { opmgpu_tables t; TabX x; const double* stone_som; };

// per-cell VALUE planes a row's neighbours read (doubles, stride nbp): phase pressures p_w, p_g (p_o is the state's pressure), the
// densities, b * mobility, rs, rv.  No derivative plane exists: a row differentiates its connections with respect to its own
// variables only and writes the neighbour's off-diagonal block itself (k_assemble_rows).
enum { VP_PW = 0, VP_PG = 1, VP_RHO = 2 /* + phase */, VP_U = 5 /* + phase */, VP_RS = 8, VP_RV = 9, VP_COUNT = 10 };

// the saturation-function model a cell-evaluating kernel is instantiated for (eval_cell), chosen on the host: BlackoilDevice::kmodel()
// KM_PVCDO, or-ed to any of the three: the oil is the analytic dead oil of opmgpu_set_pvcdo and not the tabulated one (km_pvcdo; km_model
// gives the saturation-function model alone).  A template parameter like the model and for the same reason.
// KM_KILLOUGH: the default three-phase law whose non-wetting scanning curves are Killough's (opmgpu_set_hysteresis_model) -- a model of its
// own and not a branch, so that the kernels of every other context are the ones they were: only it loads the m / R planes of the history.
// KM_DRDT, or-ed to KM_DEFAULT, KM_STONE or KM_KILLOUGH (never with KM_OW or KM_PVCDO: refused): the cell's saturated rs / rv are capped by the
// dissolution limits of opmgpu_set_dissolution_limits (DRSDT / DRVDT; km_drdt) -- a template parameter for the same reason: a context
// without limits runs exactly the instantiations it ran before the limits existed.
// KM_ROCK, or-ed to any of the four models (never with KM_PVCDO or KM_DRDT: refused): the cell's pore-volume and transmissibility multipliers
// come from its rock region's table, evaluated at min(p, p_min) under irreversible compaction (opmgpu_set_rock_regions; km_rock) -- a
// template parameter once more, so that a context without rock regions runs exactly the instantiations it ran before they existed.
enum { KM_DEFAULT = 0, KM_STONE = 1, KM_OW = 2, KM_KILLOUGH = 3, KM_PVCDO = 4, KM_DRDT = 8, KM_ROCK = 16 };
constexpr int km_model(int km) { return km & 3; }
constexpr bool km_pvcdo(int km) { return (km & KM_PVCDO) != 0; }
constexpr bool km_drdt(int km) { return (km & KM_DRDT) != 0; }
constexpr bool km_rock(int km) { return (km & KM_ROCK) != 0; }

constexpr int kRedPart = 32;        // d_red: [0, 32) results, per-workgroup partials behind them

class BlackoilDevice {
public:
    BlackoilDevice(hipStream_t s, LinSolver& ls, const opmgpu_grid* g, const opmgpu_tables* t, const opmgpu_params* prm);
    ~BlackoilDevice();
    // every transmissibility finite and >= 0 (0 is legal), else HipError(OPMGPU_EINVAL) naming the connection; host only, no device call.
    // The SELL planes carry the row's side of a connection in the SIGN of T and mark a well-fill entry with NaN: a negative value would
    // be assembled as |T| and a NaN one as a closed connection
    static void check_transmissibilities(const opmgpu_grid* g);

    int set_wells(int nw, const int32_t* connpos, const int32_t* cells);
    void set_state(const double* p, const double* sat, const double* rs, const double* rv, const int8_t* hc);
    void get_state(double* p, double* sat, double* rs, double* rv, int8_t* hc);
    void fluid_in_place(const int32_t* fipnum, int dims, double* fip_cells, double* values);      // computeFluidInPlace (:2263-2445)
    void set_pvcdo(const double* pvcdo);                                                          // the analytic dead oil (PVCDO) per PVT region; nullptr = the tabulated oil
    void set_threshold_pressures(const double* thpres);                                            // setThresholdPressures (:421-443); nullptr = none
    void compute_max_dp(const int32_t* eqlnum, int nregions, int n_face_conn, double* dp_conn, double* max_dp);      // computeMaxDp (opm/simulators/thresholdPressures.hpp:46-298)
    void set_swatinit_scaling(const double* sw, const double* pcow, double* sw_out);              // setSwatInitScaling (BlackoilPropsAdFromDeck.cpp:1009-1019)
    void get_pcw(double* pcw) const;                                                               // each cell's maximum oil-water capillary pressure
    void cap_press(const double* sat, double* pc);                                                 // capPress: [pcow | pcgo] of given / the resident saturations
    void simulator_data(double* out);                                                              // SimulatorData of the resident state (:662-683, rq_[].b/rho/mu/kr)
    void region_state_sums(const int32_t* region, int nregions, double* sums);                   // RateConverter calcAverages (RateConverterLegacy.hpp:718-768)
    void voidage_coefficients(int n, const double* p, const double* rs, const double* rv, const int32_t* pvtreg, double* coeff);   // calcCoeff (:495-548)
    void assemble(double dt, bool initial);
    template <class MS> void assemble_kernels(double dt, bool initial, MS* A, bool props_only = false);
    bool assemble_single = false;      // precision of the coming solve (opmgpu_set_solve_precision)
    int convergence(double dt, double* B3, double* CNV3, double* MB3, double* linf3, int* converged);
    void perf_props(double* out);
    void perf_pvt(const double* press, double* out);                 // host well model: PVT of the perforated cells at given pressures
    void perf_pvt_device(const double* press_dev, double* out_dev, const int32_t* gate);
    void average_b(double* B3);
    void binv_sums_device(double* out13_dev, double* scratch_dev);
    int add_well_terms(const double* resid_delta, int nblk, const int32_t* rc, const double* blocks);
    void add_well_rhs(const double* rhs_delta);
    void perf_dx(double* out);
    // right-hand side of the scaled system into the solver's b vector (precision S)
    template <class S> void build_rhs();
    template <class S> void store_dx();                 // solver x -> resident dx (double, internal planes); no copy when the solver wrote it there itself
    double* dx_device() { return d_dx.p; }              // the resident dx: what a double solve may be handed as LinSolver::solution_mirror
    void dx_to_host(double* dx);                        // resident dx -> host, equation-major caller order
    void update_state(const double* dx_host, double relax);
    void stabilize_update(int relax_type, double omega);
    void save_state();
    void restore_state();
    double relative_change();
    void update_sat_oil_max();
    void set_sat_oil_max(const double* v);
    void get_sat_oil_max(double* v);
    // DRSDT / DRVDT (the rule: opmgpu_set_dissolution_limits in include/opmgpu.h); the first two throw HipError(OPMGPU_EINVAL) with the reason
    void set_dissolution_limits(double drsdt, int free_only, double drvdt);
    void begin_dissolution_step(double dt);
    void get_dissolution_caps(double* rs_cap, double* rv_cap);
    void set_dissolution_caps(const double* rs_cap, const double* rv_cap);
    bool has_dissolution_limits() const { return drdt_on(); }
    // rock regions and irreversible compaction (the rule: opmgpu_set_rock_regions in include/opmgpu.h); all throw HipError(OPMGPU_EINVAL) with the reason
    void set_rock_regions(const opmgpu_rock_regions* spec);     // nullptr removes them
    void update_rock_history();
    void get_rock_history(double* p_min);
    void set_rock_history(const double* p_min);
    void get_rock_multipliers(double* pv_mult, double* trans_mult);
    bool has_rock_regions() const { return rock_on(); }
    // analytic aquifers (aquifer.hip; the rule: opmgpu_set_aquifers in include/opmgpu.h); all throw HipError with the reason
    struct AquiferDev;
    void set_aquifers(const opmgpu_aquifers* spec);         // nullptr or naq == 0 removes them
    void aquifer_begin_step(double dt);
    void aquifer_commit_step();
    void aquifer_state_get(double* We, double* Ws, double* t, double* pa);
    void aquifer_state_set(const double* We, const double* Ws, const double* t);
    void aquifer_connections_get(double* out);
    int aquifer_counts(int* nconn) const;                   // the number of aquifers (0 without) and of their connections
    bool has_aquifers() const;
    int update_hysteresis();
    int set_hysteresis(const double* mdc_ow, const double* mdc_go);
    int get_hysteresis(double* mdc_ow, double* mdc_go, double* d_ow, double* d_go);
    int set_hysteresis_model(int model, double killough_a);     // throws HipError(OPMGPU_EINVAL) with the reason
    int get_hysteresis_scanning(double* sncrt_ow, double* m_ow, double* r_ow, double* sncrt_go, double* m_go, double* r_go);
    void get_residual(double* r);
    // wells on the device (wells.hip)
    struct WellsDev;
    struct VfpDev;
    int set_device_wells(const opmgpu_wells* spec);
    int set_well_efficiency(const double* factors);         // [nw] in (0, 1] or NULL = ones; throws HipError(OPMGPU_EINVAL) with the reason
    int get_well_efficiency(double* factors) const;
    // controlled groups (the rule: opmgpu_set_well_groups in include/opmgpu.h); both throw HipError(OPMGPU_EINVAL) with the reason
    int set_well_groups(int ngroups, const int32_t* group_ptr, const int32_t* group_wells, const double* sign, const double* target,
                        const double* distr, const double* guide);
    int get_well_group_targets(double* slot_target, double* group_rate);
    int well_group_count() const;
    int well_shared_cells(int32_t* shared_rows, int32_t* max_wells_per_cell) const;      // throws HipError(OPMGPU_EINVAL) without device wells
    int shared_well_rows() const;                           // rows perforated by several wells (0 without device wells)
    int well_state_set(const double* bhp, const double* qs, const double* perf_press, const double* perf_rates);
    int well_state_get(double* bhp, double* qs, double* perf_press, double* perf_rates);
    int well_convergence(double* flux3, double* ctrl);
    // the well residuals ride on convergence()'s read-back (one host round trip instead of two per Newton iteration); valid until the
    // next assembly
    bool well_words_sources(const void*& e, int& ne, const void*& f) const;
    std::vector<uint32_t> well_words;
    bool well_words_valid = false;
    // decomposed runs: the wells' six convergence numbers, max-all-reduced with the cells' (h_red[13..18] after convergence())
    void well_conv_pack(double* d_out6);
    bool well_red_valid = false;
    bool has_device_wells() const;        // a device well model is attached (on this or, in a multi-rank run, on any rank)
    int set_vfp_tables(int n, const opmgpu_vfp_table* tabs);
    int vfp_evaluate(int t, int n, const double* q, const double* thp, const double* alq, const double* bhp_in, double* bhp_out, double* dbhp_dq, double* thp_out);
    int well_controls_set(const int32_t* current, const double* thp);
    int well_controls_set_targets(const double* target, const double* distr);
    int well_controls_get(int32_t* current, double* thp, int32_t* pre_its, int32_t* pre_conv);
    void wells_recover();                                   // recoverVariable: well part of the increment from the resident dx
    bool device_wells = false;
    int n_owned_cells = 0;            // multi-GPU: caller cells [0, n_owned) are owned (set by attach_comm), else nc
    double time_assemble(int reps, int props_only);
    void attach_comm(CommBase* c, int n_owned);
    const Plan& plan() const { return ls.plan; }

    int nc = 0, nconn = 0;
    opmgpu_params prm;
    double last_dt = 0.0;
    bool has_state = false, has_dx = false, has_rhs_extra = false, has_saved = false;
    int nperf = 0;

private:
    void upload_tables(const opmgpu_tables* t);
    void upload_blob(const std::vector<double>& blob);
    void perf_props_device();
    void wells_assemble(bool initial);
    // the part of wells_assemble() that reads only the state (perforation properties, updateWellControls): on Newton iterations after the
    // first it runs on a side stream next to the reservoir assembly (returns true; wells_assemble() then starts behind it)
    bool wells_prologue_async(bool initial);
    void wells_prologue();
    hipStream_t well_stream = nullptr;
    hipEvent_t ev_well[2] = { nullptr, nullptr };
    bool well_prologue_done = false;
    void wells_update(double relax, bool dx_from_host);
    void wells_stabilize(int sor, double omega);
    void wells_connection_pressures(const int32_t* gate);
    void wells_saved_state(bool restore);
    void wells_save() { wells_saved_state(false); }
    void wells_restore() { wells_saved_state(true); }
    void wells_rebind();
    void wells_free();
    void vfp_free();
    AquiferDev* aq = nullptr;
    void aquifer_free();
    void aquifer_rebind();                                  // the connections' rows in the current plan; discards a begun step
    void aquifer_discard();                                 // a begun step that is not committed (restore_state)
    void aquifer_assemble();                                // the aquifers' terms of a begun step, behind wells_assemble()
    void aquifer_launch_rates(int apply);
    int aquifer_rows(const int32_t** rows) const;           // the distinct connected rows while a step has begun, else 0
    WellsDev* wd = nullptr;
    VfpDev* vfp = nullptr;
    std::vector<double> h_surface_density;
    void rebuild_structure();
    void upload_thpres_plane();
    // decomposed runs: sum (or max) of v[0..n) over the ranks in place, through the device; nothing without a communicator
    void host_allreduce(double* v, int n, bool max);
    void check_global_region_count(int n, const char* who);     // throws unless n is the same (the GLOBAL number) on every rank

    hipStream_t stream;
    LinSolver& ls;
    // host copies of the static inputs (caller numbering)
    std::vector<int32_t> h_conn, h_pvtnum, h_satnum, h_well_connpos, h_well_cells;
    std::vector<int32_t> h_entry_conn;      // connection of every SELL entry of the current plan, -1 = none (diagonal, padding, well fill)
    std::vector<double> h_trans, h_pv, h_z, h_thpres;
    double gravity = 0.0, pvsum = 0.0, pvsum_global = 0.0;
    bool use_thpres = false;
    // ENDSCALE: per-cell scaled end points (caller numbering), unscaled points per saturation region
    bool use_eps = false;           // any saturation-function scaling: horizontal end points and / or vertical maxima
    bool has_endpoints = false, scalecrs = false, use_hyst = false, has_iendpoints = false;
    std::vector<double> h_eps[8], h_unscaled, h_eps_v[5], h_ieps[8];
    std::vector<int32_t> h_imbnum;
    DevArray<double> d_eps, d_eps_u0, d_somax, d_saved, d_ieps, d_ieps_u0, d_hist;     // d_hist: the HP_COUNT planes of the history (fluid_eval.hpp)
    // DRSDT / DRVDT: the rates [1/s] (negative = off) and DRSDT's option.  With a limit on, d_somax holds three planes of stride nbp,
    // so_max | rs_cap | rv_cap (the caps ride where so_max rides: no kernel has an argument more); without, so_max alone.  Like so_max
    // the caps are no part of the state that save / restore copy, and a re-plan carries them over.
    double drsdt = -1.0, drvdt = -1.0;
    bool drsdt_free_only = false;
    bool drdt_on() const { return drsdt >= 0.0 || drvdt >= 0.0; }
    void resize_somax(bool with_caps);
    // Rock regions: the host copy of what opmgpu_set_rock_regions took (rocknum in the caller's order; empty = none).  With regions
    // d_somax holds two planes so_max | p_min and d_satnum two planes satnum | rocknum (stride nbp; rock_pmin_of / rocknum_of): like the
    // dissolution caps they ride where an argument of every evaluating kernel rides already.  p_min is no part of the state that
    // save / restore copy, and a re-plan carries it over.
    std::vector<int32_t> h_rocknum, h_rock_ptr;
    std::vector<double> h_rock_ref, h_rock_tab;
    int rock_mode = 0;
    bool rock_on() const { return !h_rocknum.empty(); }
    void upload_rock_tables();              // the blob with or without the regions' tables behind it
    opmgpu_tables plain_rock_;              // the rock fields of dto_.t as upload_tables formed them (offset form): what removing the regions puts back
    void upload_region_numbers();           // d_satnum (satnum | rocknum) for the current plan
    int hyst_model = OPMGPU_HYST_CARLSON;    // opmgpu_set_hysteresis_model: no part of the state, of the plan or of the tables
    double killough_a = 0.1;
    void launch_hyst_update(int force);
    std::vector<double> hist_planes() const;
    DevArray<int32_t> d_imbnum;
    DevArray<double> d_stone_som;            // DevTables::stone_som
    HystArgs hyst_args() const;
    CellPlanes cell_planes() const;
    void build_eps_planes(const std::vector<double>* ep8, bool have_points, bool imbibition, std::vector<double>& planes) const;
    std::vector<double> eps_region_table(bool have_points) const;
    void upload_drainage_eps();
    std::vector<double> h_tabmax;
    DevArray<int8_t> d_saved_hc;
    const double* eps_planes() const { return use_eps ? d_eps.p : nullptr; }
    // device: tables
    DevTables dto_;                          // pointer fields = WORD OFFSETS into the blob: for the kernels that may stage it in LDS (resolve_tables)
    DevTables dtp_;                          // pointer fields = device pointers into the blob: for every other kernel
    DevArray<double> d_tab;                  // all table arrays in one blob of 8-byte words (staged in LDS by the property kernels)
    std::vector<double> h_tab;               // the blob as upload_tables formed it (without PVCDO rows): what set_pvcdo appends to
    int tab_words = 0;
    static constexpr int kTabLdsMaxBytes = 24 * 1024;     // 6 workgroups x 24 KiB fit the 160 KiB LDS of a CU: no occupancy lost
    // chooses the kernels' KM instantiations (eval_cell)
    int kmodel() const { return kmodel_plain() | (drdt_on() ? KM_DRDT : 0) | (rock_on() ? KM_ROCK : 0); }
    int kmodel_plain() const { return (oil_water() ? KM_OW : (dto_.t.threephase_model != OPMGPU_KRO_DEFAULT ? KM_STONE : (use_hyst && hyst_model == OPMGPU_HYST_KILLOUGH ? KM_KILLOUGH : KM_DEFAULT))) | (dtp_.x.oil_pvcdo ? KM_PVCDO : 0); }
    bool oil_water() const { return dto_.t.active_phases == OPMGPU_PHASES_OIL_WATER; }
    int tab_lds_words() const { return tab_words * 8 <= kTabLdsMaxBytes ? tab_words : 0; }
    size_t tab_lds_bytes() const { return size_t(tab_lds_words()) * 8; }
    // device: static per-cell / per-connection (internal numbering for cells)
    bool dual_written = false;      // mixed precision: this assembly also wrote the float copy of its double Jacobian
    DevArray<double> d_pv, d_tr_e, d_thp_e;      // per SELL entry: +-transmissibility (sign = side, NaN = well fill), threshold pressure; d_zc: cell depths (g dz is formed in the kernel)
    DevArray<int32_t> d_pvtnum, d_satnum, d_perf_cells;
    // device: state (internal numbering)
    DevArray<double> d_p, d_sw, d_so, d_sg, d_rs, d_rv;
    DevArray<int8_t> d_hc;
    // device: work
    void launch_cell_values();
    DevArray<double> d_gather;      // decomposed runs: [ranks][19] table of getConvergence's sums and maxima (one all-reduce)
    DevArray<double> d_vals, d_accum0, d_R, d_bpart, d_zc, d_dx, d_dx_old, d_red, d_perf, d_rhs_extra;
    double* h_red = nullptr;
    std::vector<double> hbuf;
    std::vector<int8_t> hbuf8;
};

} // namespace opmgpu
#endif
