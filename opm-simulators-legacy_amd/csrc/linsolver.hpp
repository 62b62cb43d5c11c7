// linsolver.hpp -- device block-ILU0 + BiCGStab on a SELL-64 3x3-block matrix.
//
// GPU replacement of the reference's inner solve:
//   ISTLSolver::solve -> ParallelOverlappingILU0 + Dune::BiCGSTABSolver  (ISTLSolver.hpp:124-189,250-274)
// in float or double (NewtonIterationBlackoilInterleaved.cpp:478-480).
#ifndef OPMGPU_LINSOLVER_HPP
#define OPMGPU_LINSOLVER_HPP

#include "amg.hpp"
#include "common.hpp"
#include "plan.hpp"

namespace opmgpu {

struct DevPlan {
    int nb = 0, nbp = 0, nslices = 0, nentries = 0, nlevels = 0, nnzb = 0;
    DevArray<int32_t> slice_ptr, col, src, entry_of_block, nat, pos, trip_ptr, trip_l, trip_u, trip_t, tpos, flux_perm;
    DevArray<int16_t> rowlen, nlower;
    DevArray<int8_t> simple;
    std::vector<int32_t> level_ptr;
    void upload(const Plan& P, hipStream_t s);
};

enum { VEC_BLOCK_INTERLEAVED = 0, VEC_EQUATION_MAJOR = 1 };

// Device-resident control block of one BiCGStab solve.  Every kernel of the iteration starts with
// `if (ctl->done) return;` so the host can enqueue iterations ahead of the convergence result.
struct SolveCtl {
    double rho[2];        // <rt,r> of the previous / current iteration (double-buffered by parity)
    double alpha, omega;
    double norm0_2;       // ||r0||^2
    double norm2;         // ||r||^2 at the last convergence test
    double thresh2;       // (reduction * ||r0||)^2
    int done;             // 1 = stop (converged or breakdown)
    int flag;             // 0 ok, 1 = |h| < eps, 2 = |rho| or |omega| <= eps
    int iters;            // dune's ceil(it) at convergence
    int decided;          // iteration whose kernel set `done` (identical on all ranks)
};

// Multi-GPU hooks (dist.hip): owner mask, halo exchange of a plane vector, all-reduce of a few doubles.
struct CommBase {
    virtual ~CommBase() {}
    virtual void halo_exchange_f(float* v, hipStream_t s) = 0;
    virtual void halo_exchange_d(double* v, hipStream_t s) = 0;
    virtual void allreduce_sum(double* dbuf, int n, hipStream_t s) = 0;
    virtual void allreduce_max(double* dbuf, int n, hipStream_t s) = 0;
    // an all-reduce (sum) and a halo exchange that do not depend on each other as ONE operation where the transport can (dist.hip)
    virtual void allreduce_sum_halo_f(double* dbuf, int n, float* v, hipStream_t s) { allreduce_sum(dbuf, n, s); halo_exchange_f(v, s); }
    virtual void allreduce_sum_halo_d(double* dbuf, int n, double* v, hipStream_t s) { allreduce_sum(dbuf, n, s); halo_exchange_d(v, s); }
    virtual const int8_t* owner_mask() const = 0;     // [nbp] internal numbering, 1 = owned
    virtual void check_async() {}          // asynchronous transport errors -> HipError(OPMGPU_ECOMM)
    virtual int my_rank() const = 0;
    virtual int num_ranks() const = 0;
    // owner rank of every local row (internal numbering; ghosts: the rank they are received from)
    virtual void subdomain_of_rows(const Plan& P, std::vector<int32_t>& sub) const = 0;
    // coarse-space unknown of every local row when every rank splits its owned cells into m index-range blocks: rank * m + block for
    // owned rows, the OWNER's value for ghost rows (one halo exchange); blk = own block of a row or -1 (ghost / padding)
    virtual void coarse_blocks_of_rows(const Plan& P, int m, hipStream_t s, std::vector<int32_t>& sub, std::vector<int8_t>& blk) = 0;
    // caller-supplied coarse blocks of the owned cells (opmgpu_comm_set_coarse_blocks): > 0 = their number per rank; such blocks keep every
    // well inside ONE block (the caller's contract), so they are used in runs with wells too
    virtual int user_coarse_blocks() const { return 0; }
    // distributed pressure hierarchy (amg.hip): level 0's neighbours and send / receive lists in internal rows, and a byte exchange with
    // per-call lists (per neighbour q: sbytes[q] from sb + soff[q], rbytes[q] into rb + roff[q]), enqueued on s
    virtual void level0_lists(const Plan& P, std::vector<int32_t>& neigh, std::vector<int32_t>& sptr, std::vector<int32_t>& srows,
                              std::vector<int32_t>& rptr, std::vector<int32_t>& rrows) const = 0;
    virtual void exchange_bytes(const std::vector<int32_t>& neigh, const char* sb, const std::vector<int64_t>& soff, const std::vector<int64_t>& sbytes,
                                char* rb, const std::vector<int64_t>& roff, const std::vector<int64_t>& rbytes, hipStream_t s) = 0;
    int n_owned_global = 0;
};

// Low-rank part of the operator: A_total = A + sum over wells of P_w Q_w (rank 7 per well: the Schur complement of the
// well equations plus the mixture coupling of the perforations, wells.hip).  Applied matrix-free inside k_spmv after
// k_lowrank_reduce has formed t_w = Q_w x; ILU0 and the AMG see A only.
struct LowRankOp {
    int nw = 0, nperf = 0;
    const int32_t* connpos = nullptr;      // [nw+1]
    const int32_t* perf_row = nullptr;     // [nperf] internal row of every perforation
    const int32_t* perf_well = nullptr;    // [nperf]
    const int32_t* perf_of_row = nullptr;  // [nbp] FIRST (lowest-index) perforation of a row or -1
    const int32_t* perf_next = nullptr;    // [nperf] next perforation of the same row (a cell of several wells) or -1
    const double* P = nullptr;             // [nperf][3][7], rows already matbal-scaled
    const double* Q = nullptr;             // [nperf][7][3]
    double* t = nullptr;                   // [nw][7] scratch
    // for the bordered pressure system of the CPR stage (one bhp unknown per well, amg.hpp): d cq_s / d (cell, mixture, bhp) per
    // perforation as the well assembly saved them ([nperf][21]: F 3x3, M 3x3, fb 3), the control equation's gradient per well
    // ([nw][4]: d g / d qs (3), d g / d bhp), and the matbal scaling of the cell rows
    const double* Fsave = nullptr;
    const double* ctrl_row = nullptr;
    double scale[3] = { 1.0, 1.0, 1.0 };
    // well efficiency factors [nw] (WEFAC): P carries them already (wells.hip, phase E); Fsave holds the UNWEIGHTED derivatives, which the
    // well equations need, so a reader that builds a CELL-row term from Fsave multiplies by eff itself (k_cpr_border's column)
    const double* eff = nullptr;
};

template <class S>
struct SolverWork {
    DevArray<S> A;      // float copy of the matrix (unused for double: the double matrix is used in place)
    DevArray<S> LU;
    DevArray<S> Apre;   // OPMGPU_EMULATE_RANKS: matrix copy without the blocks across the emulated cuts
    DevArray<S> r, rt, p, v, t, y, x, b, z, hx;  // z: scratch of the CPR second stage; hx: halo staging of x_p (multi-GPU)
    DevArray<S> kry;                             // GMRES: Krylov basis, (restart + 1) vectors
    DevArray<S> kryz;                            // flexible GMRES: the preconditioned basis z_i = M^-1 v_i, restart vectors
    DevArray<S> csT;                             // coarse space: per row, sum of its pressure entries towards each neighbour slot
    DevArray<S> cxc;                             // coarse-space part of the pressure correction (constant per subdomain)
    DevArray<S> cprw;                            // [3][nbp] per-cell weights of the pressure equation (formEllipticSystem)
    DevArray<S> cprw_orig;                       // cpr_reference_transform: the weights L was built from (cprw itself then selects the transformed pressure row)
    std::unique_ptr<AmgHierarchy<S>> amg;         // CPR pressure stage (built on first use)
    DevArray<S> plu;                             // point ILU0 of the pressure matrix A_p (cpr_use_amg = 0, elliptic.inl)
    DevArray<S> ellv;                            // work vectors of the elliptic part's inner Krylov method
    bool allocated = false;
};

// called between the library's own objects only and naming a type of the C ABI: kept out of the shared library's dynamic symbols
#define OPMGPU_LOCAL __attribute__((visibility("hidden")))

struct SolveResult { int status = 0; int iterations = 0; double reduction = 0.0; bool converged = false; };

// Two readings of opmgpu_params that the solve's driver, the early factorisation and the diagnostic entry points share.
// Under CPR the second stage's ILU0 takes the CPR preconditioner's own relaxation (cpr_relax, NewtonIterationBlackoilCPR.hpp:59) times
// cpr_stage2_relax, not the interleaved solver's ilu_relaxation
inline double cpr_stage2_relaxation(const opmgpu_params& prm) { return prm.cpr_relax * prm.cpr_stage2_relax; }
// block ILU(n) instead of the ILU0 (fillilu.inl): cpr_ilu_n under CPR, the interleaved solver's ilu_fillin_level otherwise; -1 = outside 0..8
inline int fill_level_of(const opmgpu_params& prm) { const int n = prm.use_cpr ? prm.cpr_ilu_n : prm.ilu_fillin_level; return n < 0 || n > 8 ? -1 : n; }
constexpr const char* kFillLevelRange = "cpr_ilu_n / ilu_fillin_level must be in 0..8";

class LinSolver {
public:
    explicit LinSolver(hipStream_t s);
    ~LinSolver();

    // (re)plan when the pattern changes; returns OPMGPU_* status
    int set_pattern(int nb, const int32_t* rowptr, const int32_t* col, int ordering);
    bool has_pattern() const { return plan.nb > 0; }

    // matrix values: from a host BSR (B1) -- the assembly kernels write Ad directly (B2)
    void load_host_bsr(const double* val9);
    double* matrix_d() { return Ad.p; }
    float* matrix_f();                 // float matrix buffer (allocates the float work set on first use)
    bool matrix_is_float = false;      // the current matrix values live in the float buffer only (assembled for a float solve)
    void widen_matrix();               // float buffer -> double buffer (getters, or a double solve after a float assembly)
    void zero_matrix() { Ad.zero(stream); }
    // make the matrix available in precision S (float: converts Ad -> wf.A)
    template <class S> void prepare(bool matrix_changed = true);
    template <class S> const S* matrix();
    template <class S> const S* pre_matrix();      // what the preconditioner is built from (== matrix() unless OPMGPU_EMULATE_RANKS)
    // global coarse space of the pressure stage: one unknown per subdomain (0/1 = off)
    int coarse_nsub = 0;
    DevArray<int32_t> cs_sub;      // [nbp] subdomain of every row (ghost rows: their owner's)
    DevArray<double> cs_buf;       // A_c | A_c^-1 | restricted residual
    struct CsSlots { int n; int8_t slot_of_sub[64]; int32_t sub_of_slot[8]; } cs_slots;   // real multi-GPU: this rank's own + neighbour subdomains
    const void* cs_for = nullptr;  // communicator / plan the subdomain data was built for
    int cs_m = 1;                  // coarse unknowns per rank (index-range blocks of its owned cells; OPMGPU_COARSE_BLOCKS, multi-GPU only)
    int cs_blocks_req = 4;
    bool run_has_wells = false;    // set by opmgpu_set_device_wells on EVERY rank of a run with wells (also ranks that own none)
    int cs_emulated_ns = 0;
    DevArray<int8_t> cs_blk;       // [nbp] own block of every row, -1 = not owned
    bool coarse_single_ok = false; // set by the model: the system has no wells at all (B1 matrices: unknown -> false)
    DevArray<double> cs_well_tot;
    int coarse_mode = 1;           // OPMGPU_COARSE: 0 off, 1 on with >= 2 subdomains, 2 on always (tests)
    void coarse_domains();
    template <class S> void coarse_begin();
    template <class S> void coarse_setup(bool rowparts_done);
    int emulate_ranks = 1, emulate_what = 3;      // bit 0: cut the ILU0's matrix, bit 1: the AMG's, bit 2: the stage-2 residual's (= no x_p halo exchange)
    bool pre_stale = true;

    template <class S> int factor(bool wait = true);                                // ILU0 numeric factorisation
    int factor_status() const { return (h_flags[0] & 1) ? OPMGPU_ESINGULAR : OPMGPU_OK; }   // valid after a stream synchronisation
    template <class S> void ilu_apply(const S* d, S* v, double relax, const SolveCtl* ctl = nullptr, const S* d0 = nullptr, const S* xp = nullptr, const S* a_fp = nullptr);
    template <class S> void spmv(const S* x, S* y);
    template <class S> void spmv_at(const S* x, S* y, const S* val, const int32_t* col);    // the same operator on another copy of the matrix arrays
    // CPR (solver_approach=cpr): build / refresh the pressure AMG for the current matrix; two-stage apply
    template <class S> void cpr_prepare();
    template <class S> void cpr_reweigh_rows(const int32_t* d_rows, int nrows);   // weights of these rows again, from the current matrix
    void drop_hierarchies();            // the wells changed: the bordered pressure hierarchy is rebuilt from the next matrix
    // The elliptic part the way the reference's CPR plug-in documents it (NewtonIterationBlackoilCPR.hpp:59-63; elliptic.inl): an inner
    // BiCGStab / CG on A_p, preconditioned by a point ILU0 of A_p (cpr_use_amg = 0) or by the AMG cycle.  inner = false (cpr_max_ell_iter
    // = 0): one application of the AMG cycle, no inner method.  Set from opmgpu_params by every solve().
    struct EllipticCfg { bool inner = false, use_amg = true, bicgstab = true; double tol = 1e-2; int maxit = 25; double relax = 1.0; } ell;
    long ell_solves = 0, ell_iterations = 0;     // inner solves / inner iterations since the context was created (opmgpu_cpr_elliptic_stats)
    DevArray<double> ell_parts;
    template <class S> void elliptic_factor();
    template <class S> void elliptic_solve();
    template <class S> void elliptic_ilu_apply(const S* d, S* out);   // out = relax (LU)^-1 d: the point ILU0 of A_p (border rows: their diagonal)
    template <class S> void cpr_apply(const S* d, S* v, double relax, const SolveCtl* ctl, const double* cr_given = nullptr);
    // Diagnostics of the pressure hierarchy (cpr_inspect.inl; the opmgpu_cpr_* entry points): host arrays in caller numbering, OPMGPU_* status
    template <class S> AmgHierarchy<S>* cpr_hierarchy();      // the hierarchy of the last CPR solve in precision S, or nullptr
    template <class S> int cpr_levels(int32_t* nlevels, int32_t* n, int64_t* nnz, int32_t* nw);
    template <class S> int cpr_level_get(int level, int32_t* rowptr, int32_t* col, double* val, int32_t* agg, double* dense_inv);
    template <class S> int cpr_dist_level_get(int level, int64_t* counts, int64_t* row_gid, int32_t* rowptr, int64_t* col_gid, double* val, int64_t* agg_gid);
    template <class S> int cpr_vcycle_apply_host(const double* b, double* x);
    template <class S> int cpr_apply_host(const double* d3, double* v3, double relax);
    template <class S> int cpr_elliptic_ilu_apply_host(const double* b, double* x);
    // opmgpu_params.cpr_reference_transform: the reference's CPR formulation (NewtonIterationUtilities.cpp:253-287 formEllipticSystem,
    // NewtonIterationBlackoilCPR.cpp:117-131): the WHOLE system is row-transformed by the per-cell matrix L -- first row = the sum of the
    // dominant equations (the pressure equation), scaled by 200 bar; second / third row = the water / gas equation, or the oil equation
    // where a weak oil equation was swapped out of the sum -- and the Krylov method iterates on, and measures, L A x = L b.  The matrix
    // (once per matrix), the wells' low-rank rows and the right-hand side b (every solve) are transformed in place; the CPR weights then
    // select the transformed pressure row.  The solution x is that of the untransformed system.
    template <class S> void cpr_reference_transform();
    bool ref_transformed = false;      // the resident matrix is L A (reset by whoever writes a new matrix)
    // The scaling of the coarse-grid corrections, chosen per TIME STEP by what it does to the iteration counts (DESIGN sections 4b, 11): two
    // settings; a whole time step runs under one of them and is scored by its linear iterations per Newton iteration (one solve's count
    // follows the Newton iteration's index more than the setting -- round 3's first, per-solve form of this policy was misled by that);
    // the second setting is kept only while its steps need `margin` fewer iterations, and the setting not in use is tried again for one
    // step in `period`.  Preconditioner-only: every solve still meets its reduction; the counts are global, so every rank of a decomposed
    // run decides alike.  OPMGPU_AMG_ADAPT=0: the fixed 1.9.
    struct CorrectionPolicy {
        bool on = true;
        // a LADDER of settings: index kBase (1.9) and the one above (2.3) are the pair of round 3 and all a deck ever sees while nothing goes
        // wrong; the two below exist for decks on which the scaled correction is not a contraction at all (round 4: the Norne-like deck --
        // 60 % inactive cells at random, NNCs, 36 wells -- fails 76 of 105 sub-steps at 1.9 and none at 1.0 .. 1.3: profiles/r04_ay_*).
        // A FAILED solve is repeated at once with the plain Galerkin correction (arm 0) and bans its own and every larger factor for `ban`
        // time steps; many iterations without a failure make the policy look one arm down once; scoring picks among what was tried.
        static constexpr int kArms = 4, kBase = 2;
        double arm[kArms] = { 1.0, 1.45, 1.9, 2.3 };
        double avg[kArms] = { -1.0, -1.0, -1.0, -1.0 }; // running mean of (linear iterations / solve) of the steps run under each setting (< 0: none yet)
        int banned_until[kArms] = { 0, 0, 0, 0 };       // in scored time steps
        double margin = 0.93, trouble_its = 12.0;
        int cur = kBase, steps = 0, period = 8, ban = 12;
        int step_its = 0, step_solves = 0;
        bool step_failed = false;
        bool active = false;            // set by cpr_prepare: this solve's factors come from the policy
        bool external = false;          // the current matrix came through load_host_bsr (B1): one solve per "time step", nothing to score -- fixed base setting
        bool allowed(int k) const { return k >= 0 && k < kArms && steps >= banned_until[k]; }
        void fail_at_current(int iterations);      // a solve failed under arm `cur` (> 0): penalty, ban, tallies reset, cur = 0
    } corr_policy;
    void correction_policy_choose();
    void correction_policy_report(int iterations, bool converged);
    // x0 = 0; rhs in work<S>().b; solution in work<S>().x
    // opmgpu_params.cpr_reference_transform = 2 (pointilu.inl): the reference's second stage under CPR, a POINT ILU0 of the transformed system as
    // a scalar equation-major matrix, on its own sparsity plan
    struct PointIlu {
        Plan plan; DevPlan dp;
        DevArray<int64_t> gather;      // [nentries of the scalar plan] offset of the block component in the SELL-64 block matrix, -1 = padding
        DevArray<int32_t> vmap;        // [nbp of the scalar plan] plane * nbp + row of the block vectors, -1 = padding
        DevArray<double> val, lu, d, v;
        bool built = false, stale = true;
        int for_nb = 0, for_nnzb = 0, for_ordering = -1, for_plan_id = -1;
    } pilu;
    // block ILU(n) with level-of-fill (fillilu.inl): opmgpu_params.cpr_ilu_n / ilu_fillin_level.  fill_level > 0 reroutes factor<S>() and
    // ilu_apply<S>() to the filled pattern's own plan; 0 = the ILU0 on the matrix's pattern
    template <class S> struct FillWork { DevArray<S> val, lu, d, v; };
    struct FillIlu {
        Plan plan; DevPlan dp;
        DevArray<int32_t> src;         // [nentries of the filled plan] entry of the block in the matrix's SELL-64 layout, -1 = fill / padding
        DevArray<int32_t> vmap;        // [nb] row of the matrix's plan for each row of the filled plan
        FillWork<float> wf; FillWork<double> wd;
        template <class S> FillWork<S>& work();
        bool built = false;
        int for_level = -1, for_ordering = -1, for_plan_id = -1, nnzb_filled = 0;
    } fill;
    int fill_level = 0;                // the kind of the resident factors (what ilu_apply / get_lu_bsr read): set by solve(), and by opmgpu_ilu0_factor before its factor<S>()
    void fill_setup();
    template <class S> int fill_factor(bool wait);
    template <class S> void fill_apply(const S* d, S* v, double relax, const SolveCtl* ctl);
    std::string breakdown_note;        // what the last OPMGPU_EBREAKDOWN was (for the error text)
    int plan_id = 0;                   // counts re-plans (set_pattern)
    void point_ilu_setup();
    void point_ilu_factor();
    void point_ilu_apply(const double* d, double* v, double relax);
    // opmgpu_params.preconditioner_single: a double solve whose preconditioner lives in the FLOAT work set (wf: float matrix copy, float ILU0
    // factors, float pressure hierarchy); the Krylov method converts the vector it hands over and the one it gets back (now.mixed).
    bool float_copy_valid = false;       // wf.A holds the current matrix (written by mixed_prepare; reset by whoever writes a new matrix)
    void mixed_prepare(bool matrix_changed);
    void cpr_prepare_mixed();
    template <class S> void precond_apply(const S* d, S* out, double relax, const SolveCtl* ctl, bool cpr, const double* cr_given = nullptr);
    template <class S> SolveResult bicgstab(const opmgpu_params& prm);
    template <class S> SolveResult gmres(const opmgpu_params& prm);      // newton_use_gmres: restarted, left-preconditioned
    // The driver of a linear solve (solve.inl): the loaded matrix, right-hand side in work<S>().b, solution in work<S>().x.  It checks prm,
    // configures this solve (`now`, ell, fill_level, wb_relax), factorises unless factor_ahead() has, runs the Krylov method and its retries.
    // Returns the status; OPMGPU_EINVAL = refused (its text in err, nothing solved), otherwise res is the last solver run's and err its text, if any
    template <class S> OPMGPU_LOCAL int solve(const opmgpu_params& prm, bool matrix_changed, SolveResult& res, std::string& err);
    // This solve: what solve() derives from prm and the loaded matrix for the solvers, cpr_prepare() and cpr_apply() to read.  Nobody outside
    // the solver writes it.
    struct ThisSolve {
        bool mixed = false;                    // preconditioner_single in effect: the preconditioner of this double solve is the float work set's
        bool point_stage2 = false;             // cpr_reference_transform = 2: the point ILU0 is the second stage
        const void* border_weights = nullptr; double border_colscale = 1.0;      // weights (and scale) of the bordered pressure column when cprw are the transformed system's unit weights
        bool factor_deferred = false;          // factor_async() is started by cpr_prepare() behind its pass over the matrix
    } now;

    // host <-> device vector staging (caller numbering <-> internal, component-major planes)
    template <class S> void vec_from_host(const double* h, int layout, S* d);
    template <class S> void vec_to_host(const S* d, int layout, double* h);
    // device double vector in caller layout -> internal S vector and back (no PCIe)
    template <class S> void vec_in(const double* dsrc, int layout, S* d);
    template <class S> void vec_out(const S* d, int layout, double* ddst);

    void get_matrix_bsr(const double* sell, double* val9);          // Ad-like (double) SELL -> host BSR
    void get_float_copy_bsr(double* val9);                          // the float copy of a double matrix (mixed precision) -> host BSR, widened
    template <class S> void get_lu_bsr(double* val9);

    template <class S> SolverWork<S>& work();
    template <class S> void ensure_work();

    // timing of a single kernel on this stream (HIP events), ms per launch
    double time_kernel(int kernel, int reps, int single_precision);
    KernelTimers kt;               // in-situ timing of kernel classes during real iterations (opmgpu_kernel_timing)
    DevArray<char> cold;           // OPMGPU_K_SPMV_COLD: extra copies of the matrix values + column indices

    Plan plan;
    DevPlan dp;
    hipStream_t stream;
    DevArray<double> Ad;
    DevArray<double> stage;        // host-BSR staging / vector staging
    DevArray<double> partials;     // 6 partial arrays of npart doubles + 8 all-reduced scalars
    DevArray<int32_t> flags;
    DevArray<double> gmbuf;        // GMRES: Hessenberg matrix, s, cs, sn, y
    SolveCtl* h_ctl = nullptr;     // host-mapped status copy (device publishes, host polls after an event)
    SolveCtl* h_ctl_dev = nullptr; // device alias of h_ctl
    int* h_tick = nullptr;         // host-mapped sequence word of the status checks (wait_tick)
    int* h_tick_dev = nullptr;
    int tick_seq = 0;
    bool poll_status = true;       // OPMGPU_POLL=0: synchronise the stream instead
    void wait_tick(int tick);
    // Small device results to the host without hipStreamSynchronize's interrupt round trip: one workgroup copies up to two word ranges
    // into a host-mapped buffer and writes the tick word the host spins on (wait_tick).  Returns the host copy (valid until the next call).
    const uint32_t* fetch_words(const void* src0, int nwords0, const void* src1 = nullptr, int nwords1 = 0, const void* src2 = nullptr, int nwords2 = 0);
    uint32_t* h_pub = nullptr;     // host-mapped
    uint32_t* h_pub_dev = nullptr;
    static constexpr int kPubWords = 8192;
    DevArray<SolveCtl> ctl;        // device-resident control block read by every kernel
    int32_t* h_flags = nullptr;    // pinned
    int cur_ordering = -1;
    int npart = 0;                 // entries per partial array
    CommBase* comm = nullptr;      // not owned; nullptr = single GPU
    LowRankOp lowrank;             // nw == 0: none
    DevArray<int8_t> light_ok;     // multi-GPU: rows that keep the closed form (owned, no ghost neighbour)
    const CommBase* light_ok_for = nullptr;
    DevArray<int8_t> gm_light;     // GMRES closed form: level-0 rows without a perforation (built once per well plan, gmres())
    const int32_t* gm_light_for = nullptr; int gm_light_plan = -1;      // the perf_of_row map / plan it was built from (wells_rebind -> drop_hierarchies resets)
    template <class S> void lowrank_reduce(const S* x, const SolveCtl* ctl);
    // Stage 2 of the CPR preconditioner sees the wells: the ILU0 is of A, the operator is A + sum_w P_w Q_w.  Woodbury with
    // the block-diagonal of the ILU0 standing in for its inverse on the (few) perforated rows:
    //   (M + P Q)^-1 ~ M^-1 - Y (I + Q Y)^-1 Q M^-1,   Y = omega D^-1 P   (D^-1: the ILU0's inverted diagonal blocks of the perforated rows)
    // Y and the 7 x 7 inverses are formed behind every factorisation (k_wb_setup), one launch per application applies the correction
    // (k_wb_apply).  Under GMRES only (BiCGStab's closed-form rows assume x = M^-1 p with the plain ILU0).  OPMGPU_WELL_WOODBURY=1.
    DevArray<double> wb_buf;       // [nperf][3][7] Y | [nw][49] inverses
    bool well_woodbury = false, wb_active = false;
    bool wb_suspended = false;     // the correction was asked for and is off while wells share a cell (wells_rebind)
    double wb_relax = 0.9;         // the ILU0's relaxation factor (omega above), set by solve() / factor_ahead() before the factorisation
    // k_spmv shortcut on level-0 rows, which have no lower entries (half of all rows with the 2-colour ordering): no matrix traffic there.
    // BiCGStab: (A M^-1 p)_i from p and the second stage's input; left-preconditioned GMRES in double with relaxation 1: (A v_i)_i =
    // gamma_i base_i with one device-resident scalar per column (linsolver.hip, k_spmv; the conditions: bicgstab() / gmres()).
    // A/B switch for both: OPMGPU_CLOSED=0, read when the solver is created
    bool closed_form_level0 = true;
    // Passes and launches a GMRES solve does not need (krylov.inl, gmres()): x is not cleared (the first cycle's
    // combination starts from the literal 0), the combination also stores to the caller's solution_mirror, the clear of gmbuf rides in
    // k_ctl_init, no k_gm_reset_s behind that clear, and the V-cycle's restriction runs eight lanes per aggregate.  The same bits as the
    // plain launches.  A/B switch: OPMGPU_LEAN_SOLVE=0, read when the solver is created
    bool lean_solve = true;
    bool plain_setup() const;              // what every item below asks of the set-up: single GPU, no emulated ranks, plain ILU0 second stage, no Woodbury correction
    bool lean_conditions() const { return lean_solve && plain_setup(); }
    // Optional second destination of a double GMRES solve's solution (same layout as work<double>().x), set by the caller before the solve
    // and taken by the first gmres() call behind it; mirror_written: that call stored every entry of x there too
    double* solution_mirror = nullptr;
    bool mirror_written = false;
    // The pressure part cancels on the level-0 rows (cpr_apply, ilu_apply): in a two-level plan with every relaxation
    // factor 1 a level-0 row's entry of M^-1 d, pressure correction included, is D^-1 (d - sum A_rb (M^-1 d)_b) with d the application's
    // input -- the top level's forward sweep adds x_p to its rows, the level-0 backward sweep starts from d, k_cpr_add_p is not launched.
    // Rounds differently from the plain sequence.  Double GMRES solves only.  A/B switch: OPMGPU_CPR_CANCEL_P=0, read when the solver is created
    bool cpr_cancel_p = true;
    bool cancel_p_now = false;             // this solve's applications take that path (set by the solvers)
    // The top level's part of the stage-2 residual travels through the ILU0 factor (cpr_apply, ilu_apply): a top row i of
    // a two-level plan has lower entries to level-0 rows only and L_ir = A_ir A_rr^-1, so its forward sweep
    // y_i = z_i - sum_r L_ir z_r, z = d - A [x_p; 0; 0], is (d_i - A_ii[:,0] x_p,i) - sum_r L_ir s_r with s_r the level-0 row's residual
    // without its own diagonal term.  k_cpr_presidual_l0 forms s on the level-0 rows alone, the sweep its own rows' part; z on the top
    // rows is never formed.  On the cancellation's conditions, and with it on.  Rounds differently again.  A/B switch: OPMGPU_CPR_FACTOR_P=0,
    // read when the solver is created
    bool cpr_factor_p = true;
    bool cpr_halo_xp = true;        // multi-GPU CPR: halo-exchange the pressure correction before stage 2 (A/B: OPMGPU_CPR_HALO_XP=0)
    int amg_lag = 1, amg_age = 0;   // A/B: OPMGPU_AMG_LAG
    // refresh policy of the coarse operators of the pressure hierarchy (see cpr_prepare); OPMGPU_AMG_LAG_COARSE
    int coarse_lag = 1, coarse_age = 0;
    bool new_step_hint = true;     // set by the caller for the first matrix of a time step (and for every external matrix)
    bool refreshed = true;         // the current solve runs on freshly built coarse operators
    int last_its = 0, its_ref = 0; // iterations of the last solve / of the solve right after the last refresh
    int last_verify_rounds = 0;    // GMRES with gmres_verify_residual: how often the true residual sent the last solve back to work
    bool weights_from_assembly = false;   // cprw of the current matrix was written by the assembly kernel (k_flux), not by k_cpr_weights
    bool lu_copy_upper = false;    // factor(): also store the U entries that equal A's (diagnostic read-back of the factors)
    bool lag_allowed = true, force_refresh = false;
    int step_matrix = 0;           // matrices seen since the time step began
    int lag_block = 0;             // > 0: time steps during which the coarse operators follow every matrix again
    int cpr_weight_mode = 0;        // 0 = formEllipticSystem's 0/1 dominance weights (reference); 1 = quasi-IMPES (A/B: OPMGPU_CPR_WEIGHTS=1)
    bool cpr_speculate = false;     // CPR: enqueue the next iteration before the convergence result is known (A/B: OPMGPU_CPR_SPECULATE=1)
    hipEvent_t ev[2] = { nullptr, nullptr };
    // multi-GPU: the halo exchange of the SpMV input runs on its own stream while the rows without a ghost neighbour are multiplied
    // (k_spmv phase 1); the rows next to a cut follow the exchange (phase 2).  A/B: OPMGPU_HALO_OVERLAP=0 serialises them on `stream`.
    bool halo_overlap = true;
    // ILU0 factorisation on a second stream next to the set-up of the pressure stage (both only read the matrix); the first ILU0
    // application joins.  A/B: OPMGPU_FACTOR_OVERLAP
    bool factor_overlap = true, factor_pending = false;
    // The ILU0 factorisation of a freshly ASSEMBLED matrix starts at the end of the assembly (behind the wells' diagonal contributions), on its
    // own stream: it then runs next to getConvergence, the host's decision and the first pass of the pressure stage's set-up instead of next
    // to the small levels' Galerkin sums, which it slowed from ~25 to ~200 us (profiles/r04_e trace).  A call that turns out converged has
    // factorised for nothing (device time only; such a call is 0.5 ms against 2.8).  factor_ahead() is the model's call at the end of its
    // assembly: it decides whether this matrix qualifies and in which precision the solve will want the factors, runs `matrix_final` (what
    // the model still owes the matrix copy the factorisation reads) and starts it; solve() then does not start another.
    // A/B: OPMGPU_FACTOR_EARLY=0
    bool factor_early_on = true;
    enum Ahead { AHEAD_NONE, AHEAD_FLOAT, AHEAD_DOUBLE } ahead = AHEAD_NONE;      // the factors factor_ahead() started for the current matrix
    OPMGPU_LOCAL void factor_ahead(const opmgpu_params& prm, bool host_wells, const std::function<void()>& matrix_final);
    DevArray<double> cgs_parts;          // decomposed GMRES, classical Gram-Schmidt: (restart + 1) partial arrays + their all-reduced sums
    hipStream_t factor_stream = nullptr;
    hipEvent_t ev_factor[2] = { nullptr, nullptr };
    template <class S> void factor_async();
    void join_factor();
    // multi-GPU CPR with the subdomain coarse space: the restricted residual of the vector a preconditioner application starts from is
    // carried by the BiCGStab recurrences (it is linear in the vector), so only <W_b, A y> has to be summed over the ranks -- together
    // with the scalar products the iteration all-reduces anyway: 3 all-reduces per iteration instead of 5.  A/B: OPMGPU_CS_RECUR=0.
    bool cs_recur = true;
    // Decomposed CPR: level 0 of the pressure cycle on the GLOBAL matrix -- the iterate's ghost entries are refreshed from their owners before
    // the down leg's residual and before every post-smoothing sweep (AmgHierarchy::level0_halo; one more halo exchange each, 2 per
    // application under GMRES, 3 under BiCGStab).  The rank-local hierarchy is what fails on heterogeneous decks (SPE10-like: 4.7 -> 46
    // iterations when only the AMG's matrix is cut, 9 with level 0 uncut: profiles/r04_ag_emulate_l0_global.log); on smooth decks the
    // counts are the single-domain ones without it.  opmgpu_params has no field for it: OPMGPU_CPR_L0_HALO=1 / 0, default 1 (on).
    bool cpr_l0_halo = true, cpr_l0_halo_down = true;
    // Decomposed CPR, opmgpu_comm_set_pressure_hierarchy (default OPMGPU_CPR_GLOBAL_AMG, read at comm init): 0 = the rank-local cycle above with
    // the Nicolaides coarse space, 1 = the distributed hierarchy of amg.hpp (every level global; no coarse space, level 0's exchanges are
    // the hierarchy's own).  No effect on one rank.
    int cpr_hier_mode = 0;
    bool dist_hierarchy() const { return comm && comm->num_ranks() > 1 && cpr_hier_mode == 1 && !ell.inner; }
    DevArray<double> cs_state;     // [2 ns]: restricted residual of p, of r
    hipStream_t halo_stream = nullptr;
    hipEvent_t ev_halo[2] = { nullptr, nullptr };

private:
    SolverWork<double> wd;
    SolverWork<float> wf;
};

template <> SolverWork<double>& LinSolver::work<double>();
template <> SolverWork<float>& LinSolver::work<float>();
template <> void LinSolver::prepare<double>(bool);
template <> void LinSolver::prepare<float>(bool);
template <> const double* LinSolver::matrix<double>();
template <> const float* LinSolver::matrix<float>();

} // namespace opmgpu
#endif
