// amg.hpp -- pressure stage of the CPR preconditioner: plain-aggregation AMG V-cycle on the device.
//
// GPU counterpart of the reference's `solver_approach=cpr` (NewtonIterationBlackoilCPR.cpp:79-185):
//   * elliptic (pressure) system = sum of the scaled phase equations, pressure column
//     (formEllipticSystem, NewtonIterationUtilities.cpp:197-287 -- its default L = [1 1 1]; the per-cell
//     diagonal-dominance fallback is not restated),
//   * stage 1: one AMG V-cycle on it (the reference uses dune-istl's aggregation AMG through
//     opm-simulators' CPRPreconditioner -- external, restated from the published algorithm: greedy
//     strength-based aggregation, piecewise-constant prolongation, Galerkin coarse operators),
//   * stage 2: block ILU0 on the full system (linsolver.hip).
// The aggregation hierarchy (pure structure) is built on the host ONCE per sparsity pattern from the first
// matrix and reused; every new matrix only re-runs the numeric Galerkin sums on the device (deterministic:
// each coarse entry sums a fixed list of fine entries in a fixed order).
#ifndef OPMGPU_AMG_HPP
#define OPMGPU_AMG_HPP

#include <functional>
#include <memory>
#include <vector>

#include "common.hpp"
#include "plan.hpp"

namespace opmgpu {

struct SolveCtl;
struct CommBase;
struct HostCsr;          // host csr of one level during setup (amg.hip)

template <class S>
struct AmgLevel {
    int n = 0, nslices = 0, nentries = 0;
    // matrix in scalar SELL-64 (same indexing as the block plan: entry e = (slice_base + slot) * 64 + lane)
    const int32_t* slice_ptr = nullptr;      // device
    const int32_t* col = nullptr;            // device
    DevArray<int32_t> own_slice_ptr, own_col;   // coarse levels own their structure (level 0 borrows the block plan's)
    DevArray<int32_t> diag_entry;               // [n]
    DevArray<S> val, dinv, x, b, r, x2;
    // transfer to the next coarser level
    DevArray<int32_t> agg;                      // [n] coarse index of every row
    DevArray<int32_t> agg_ptr, agg_rows;        // rows of every aggregate (restriction, fixed order)
    DevArray<int32_t> contrib_ptr, contrib_idx; // fine entries summed into every coarse entry (Galerkin), entries sorted by trip count
    DevArray<int32_t> contrib_diag;             // per (sorted) coarse entry: its row if it is the diagonal one, else -1
    int n_coarse = 0, nentries_coarse = 0, galerkin_lpe = 1;
    std::vector<int32_t> h_rowlen;              // coarse levels: real slots of every row (host copy, diagnostics; level 0: the plan's rowlen)
    // Level 0 only -- BORDERED operator [A_p Bc; Cr Dw]: one extra unknown per well (its bhp) that couples the well's perforated cells
    // like the reference's explicit Schur complement does, without filling the borrowed block-plan structure with a clique per well.
    // Vectors of a bordered level have n + nw entries (well k at index n + k); the border values live behind the SELL values:
    // val[nentries + j] = column entry of perforation j (row perf_row[j], column n + well), val[nentries + nperf + j] = row entry
    // (row n + well, column perf_row[j]), val[nentries + 2 nperf + k] = diagonal of well k.
    // The wells' rows stay singletons on every level down to the coarsest, whose dense inverse holds kDenseMax = 96 rows: setup() builds the
    // border for at most kDenseMax / 2 = 48 wells and none beyond (the wells then act through their cells' diagonal terms only).
    int nw = 0, nperf = 0;
    const int32_t* b_connpos = nullptr;         // [nw+1]  (device, owned by the well model)
    const int32_t* b_perf_row = nullptr;        // [nperf]
    const int32_t* b_perf_of_row = nullptr;     // [>= n] first perforation of a row or -1
    const int32_t* b_perf_next = nullptr;       // [nperf] next perforation of the same row or -1 (a cell of several wells: one border column each)
    const int32_t* b_perf_well = nullptr;       // [nperf]
    int ntot() const { return n + nw; }
    // Distributed level of a decomposed hierarchy (AmgHierarchy::setup with a communicator).  Level 0: the rows are the
    // plan's, ghost rows included (identity rows); levels >= 1: n = owned rows (wells last), followed in every vector by `nghost` ghost
    // entries (the neighbours' coarse unknowns this rank's rows couple to).  The ghost entries of the iterate are refreshed from their
    // owners by xchg_*: pack xchg_send, exchange with xchg_neigh, unpack into xchg_recv (level 0: x and b of the ghost rows).
    bool dist = false;
    int nghost = 0;
    int64_t goff = 0, nglobal = 0;              // global numbering of the owned rows: goff + local index (levels >= 1; wells included)
    std::vector<int64_t> h_gid;                 // levels >= 1: global id of every local entry, ghosts included (diagnostics)
    std::vector<int8_t> h_owned;                // level 0: owned plan rows (host copy)
    std::vector<int32_t> xchg_neigh;
    std::vector<int64_t> xchg_soff, xchg_scnt, xchg_roff, xchg_rcnt;      // in elements, per neighbour
    std::vector<int64_t> xchg_bytes[2][4];      // the same in bytes for 4- [0] and 8-byte [1] entries: send offset, count, receive offset, count
    DevArray<int32_t> xchg_send, xchg_recv;
    DevArray<double> xchg_sbuf, xchg_rbuf;
    int next() const { return n + nw + nghost; }    // entries of a vector of this level
};

// host description of the border handed to AmgHierarchy::setup
struct AmgBorderSpec {
    int nw = 0, nperf = 0;
    std::vector<int32_t> connpos, perf_row;     // internal rows
    std::vector<double> bcol, crow, dw;         // representative values (first matrix) for the aggregation strengths
    const int32_t *d_connpos = nullptr, *d_perf_row = nullptr, *d_perf_of_row = nullptr, *d_perf_well = nullptr, *d_perf_next = nullptr;
};

template <class S>
class AmgHierarchy {
public:
    explicit AmgHierarchy(hipStream_t s) : stream(s) {}
    ~AmgHierarchy()
    {
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        for (auto e : ev_inv) if (e) (void)hipEventDestroy(e);
        if (inv_stream) (void)hipStreamDestroy(inv_stream);
    }
    AmgHierarchy(const AmgHierarchy&) = delete;
    AmgHierarchy& operator=(const AmgHierarchy&) = delete;
    // structure from the block plan + the level-0 pressure values (host copy, entry-indexed); builds all levels
    void setup(const Plan& P, const int32_t* d_slice_ptr, const int32_t* d_col, const std::vector<double>& ap_host, const AmgBorderSpec* border = nullptr);
    int border_nw() const { return levels.empty() ? 0 : levels[0]->nw; }
    bool ready() const { return !levels.empty(); }
    // numeric phase for a new matrix: level-0 values are already in levels[0].val
    // after_level0: called once the level 0 -> 1 sums are enqueued (or at once when there is nothing of the kind)
    void galerkin(bool coarse_levels = true, const std::function<void()>& after_level0 = {});
    // x0 = Vcycle(b0) with b0 in levels[0].b; result in levels[0].x
    // level0_presmoothed: levels[0].x already holds omega D^-1 b (the caller's kernel did the first sweep)
    void vcycle(const SolveCtl* ctl, bool level0_presmoothed = false);
    // the same cycle replayed from a captured hipGraph (OPMGPU_AMG_GRAPH=1; A/B knob)
    void vcycle_graph(const SolveCtl* ctl, bool level0_presmoothed);
    hipGraphExec_t graph_exec = nullptr;
    const SolveCtl* graph_ctl = nullptr;
    double graph_key[7] = { 0, 0, 0, 0, 0, 0, 0 };
    bool graph_pre = false, use_graph = false;
    std::vector<std::unique_ptr<AmgLevel<S>>> levels;
    DevArray<double> dense_inv;      // coarsest: explicit inverse (double), n_c x n_c (border rows included when level 0 is the coarsest)
    // the inversion runs on inv_stream behind the work that follows galerkin(); the first user of dense_inv joins it
    hipStream_t inv_stream = nullptr;
    hipEvent_t ev_inv[2] = { nullptr, nullptr };
    bool inv_pending = false, inv_overlap = true;
    void join_inverse();
    int n_coarsest = 0;
    std::vector<int> level_sizes;
    hipStream_t stream;
    // Measured on MI355X over omega x pdamp x npre x npost (tools/amg_sweep.py, 100^3 decks with sigma_lnK = 0.5 and 2.0): the
    // plain-aggregation correction is too small by a factor ~2 (dune-istl scales it by 1.6 for the same reason); 1.9 / 0.9 / 1+2
    // sweeps was the best setting that helped on both decks (-19 % and -7 % time per Newton iteration).  Env OPMGPU_AMG_* override.
    double omega = 0.9;           // damped-Jacobi weight
    double pdamp = 1.9;           // coarse-grid correction scaling (dune-istl's prolongation damping factor); see LinSolver::cpr_prepare for 2.2
    double pdamp0 = 1.9;          // ... of the correction into level 0 (OPMGPU_AMG_PDAMP0)
    bool pdamp_user = false;      // OPMGPU_AMG_PDAMP given: no automatic choice
    // Set by the first application of this hierarchy (LinSolver::cpr_apply).  Until then cpr_prepare assigns its fixed factors (1.9, or 2.2 into
    // level 0) whenever the correction policy does not choose; afterwards such matrices keep what pdamp0 / pdamp hold.
    bool factors_kept = false;
    // Decomposed runs (set by LinSolver per application, empty otherwise): called with level 0's iterate before every level-0 operation
    // that reads neighbours' entries of it -- the residual of the down leg and each post-smoothing sweep.  The callback refreshes the ghost
    // entries from their owners (one halo exchange) so that level 0 of the cycle works on the GLOBAL pressure matrix; the coarse levels
    // stay rank-local.  With the hook set the cycle takes the unfused level-0 launches (smooth / residual / prolong / sweeps).
    std::function<void(S* x, S* b)> level0_halo;
    bool level0_halo_down = true;          // false: only the post-smoothing sweeps see the neighbours (A/B: OPMGPU_CPR_L0_HALO=2)
    int npre = 1, npost = 2;      // smoothing sweeps before / after the coarse-grid correction
    int npost0 = 2;               // post-smoothing sweeps on level 0 (cheap per sweep there; coarse levels are launch-latency bound)
    bool npost0_user = false;     // OPMGPU_AMG_NPOST0 given: the solvers do not choose (BiCGStab 2, GMRES 1)
    int coarse_sweeps = 4;        // pairs of Jacobi sweeps standing in for the coarsest solve when it is too big for the dense inverse
    bool fuse = true;             // launch fusions of the V-cycle (A/B: OPMGPU_AMG_FUSE=0)
    bool lane_restrict = false;   // restriction with eight lanes per aggregate (k_amg_restrict_lanes; same bits): set by LinSolver per solve, part of the graph's key
    bool use_gs = false;          // level 0: Gauss-Seidel by colour instead of damped Jacobi when the row order has two colours (OPMGPU_AMG_GS)
    int gs_n0 = 0;                // rows [0, gs_n0) are the first colour (0 = no two-colour order)
    bool gs_level0() const { return use_gs && gs_n0 > 0 && npre == 1; }
    double omega0() const { return gs_level0() ? 1.0 : omega; }      // weight of the caller's fused first sweep on level 0
    // Distributed hierarchy (opmgpu_comm_set_pressure_hierarchy mode 1): set dcomm before setup().  Levels [0, ndist) are distributed
    // (aggregates inside a rank, Galerkin products keep the couplings to the neighbours' aggregates); level ndist, the first whose global
    // size is at most kTailRows, and all coarser ones are replicated on every rank (the tail).  ndist = 0: the rank-local hierarchy.
    static constexpr int kTailRows = 384;
    int tail_rows = kTailRows;               // OPMGPU_AMG_TAIL_ROWS (A/B and tests: a smaller value keeps more levels distributed)
    CommBase* dcomm = nullptr;
    int ndist = 0;
    int64_t tail_off = 0, tail_own = 0;      // this rank's rows of the first tail level
    int64_t tail_nnz = 0;                    // csr entries of the first tail level
    DevArray<int32_t> tail_pos;              // per own Galerkin entry of the last distributed level: its csr position in the first tail level
    DevArray<int32_t> tail_dev;              // [tail_nnz] SELL slot of every csr entry of the first tail level
    DevArray<double> tail_buf;               // zero-padded partial sums: Galerkin values / restricted right-hand side of the tail
    static constexpr int kReduceChunk = 4096;
private:
    void setup_dist(const Plan& P, HostCsr& A, std::unique_ptr<AmgLevel<S>>& L, int& npin, std::vector<int8_t>& pinmark, int max_levels);
    void allreduce_chunked(double* d, int64_t n);      // all-reduces of at most kReduceChunk doubles (32 KiB messages)
    template <class T> void xchg(AmgLevel<S>& F, T* x, T* b, const SolveCtl* ctl);
    // the launches of the cycle (amg.hip): row_op chooses the row kernel of a level, the others are built on it
    template <int MODE> void row_op(AmgLevel<S>& F, const SolveCtl* ctl, const S* xc = nullptr, S pdamp = S(0));
    void smooth0(AmgLevel<S>& F, S w, const SolveCtl* ctl);
    void first_residual(AmgLevel<S>& F, bool presmoothed, const SolveCtl* ctl);
    void sweep(AmgLevel<S>& F, const SolveCtl* ctl);
};

} // namespace opmgpu
#endif
