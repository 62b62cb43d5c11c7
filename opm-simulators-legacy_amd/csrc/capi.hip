// capi.hip -- the extern "C" boundary of libopmgpu.so (include/opmgpu.h).
//
// Every entry point catches C++ exceptions and converts them to the status codes the reference-side
// shim maps back to the exception flow_legacy's time stepper expects.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <array>
#include <memory>
#include <string>

#include "blackoil.hpp"
#include "dist.hpp"
#include "linsolver.hpp"

using namespace opmgpu;

struct opmgpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    opmgpu_params prm;
    std::unique_ptr<LinSolver> ls;
    std::unique_ptr<BlackoilDevice> model;
    std::string err;
    int cur_single = 0;          // precision of the loaded / prepared matrix
    bool matrix_loaded = false;
    bool factored = false;
    // phase timings (assemble, solve, update): events recorded around the phase, resolved only when opmgpu_last_timings asks --
    // a synchronisation at the end of every call would leave the GPU idle until the host has enqueued the next phase
    double t_phase[3] = { 0, 0, 0 };
    hipEvent_t evp[3][2] = { { nullptr, nullptr }, { nullptr, nullptr }, { nullptr, nullptr } };
    bool ev_pending[3] = { false, false, false };
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::unique_ptr<RcclComm> comm;   // multi-GPU (dist.hip); empty = single GPU
    // opmgpu_nonlinear_iteration: residual_norms_history_ / current_relaxation_ of BlackoilModelBase (:244-247, :300-315)
    std::vector<std::array<double, 3>> norm_history;
    double relaxation = 1.0;
    // opmgpu_iteration_marks: one event at the end of every opmgpu_nonlinear_iteration call and one pair per phase, kept per call (nothing
    // is synchronised while the marks are on; opmgpu_iteration_marks_get resolves them afterwards)
    struct IterMark { hipEvent_t end = nullptr; hipEvent_t ph[3][2] = { { nullptr, nullptr }, { nullptr, nullptr }, { nullptr, nullptr } }; int solved = 0, lin = 0, status = 0; };
    bool marks_on = false;
    hipEvent_t mark_start = nullptr;
    std::vector<IterMark> marks;
    IterMark* cur_mark = nullptr;
    // events of the marks are recycled through a pool (a caller that leaves the marks on for a long run does not create seven new events per
    // call for ever), and the list is capped: beyond kMaxMarks calls the marks stop being recorded (n_calls of marks_get keeps counting)
    static constexpr size_t kMaxMarks = 16384;
    long marks_dropped = 0;
    std::vector<hipEvent_t> mark_pool;
    hipEvent_t mark_event() { if (!mark_pool.empty()) { hipEvent_t e = mark_pool.back(); mark_pool.pop_back(); return e; } hipEvent_t e = nullptr; return hipEventCreate(&e) == hipSuccess ? e : nullptr; }
    void marks_clear(bool destroy = false) {
        for (IterMark& m : marks) { if (m.end) mark_pool.push_back(m.end); for (auto& pr : m.ph) for (auto& e : pr) if (e) mark_pool.push_back(e); }
        marks.clear(); cur_mark = nullptr; marks_dropped = 0;
        if (mark_start) { mark_pool.push_back(mark_start); mark_start = nullptr; }
        if (destroy) { for (hipEvent_t e : mark_pool) (void)hipEventDestroy(e); mark_pool.clear(); }
    }
};

namespace {

int fail(opmgpu_ctx* c, int code, const std::string& msg) { if (c) c->err = msg; return code; }

template <class F> int guarded(opmgpu_ctx* c, F&& f)
{
    try {
        if (c) { if (hipSetDevice(c->device) != hipSuccess) return fail(c, OPMGPU_ENODEVICE, "hipSetDevice failed"); }
        return f();
    } catch (const HipError& e) { return fail(c, e.code, e.what()); }
    catch (const std::bad_alloc&) { return fail(c, OPMGPU_ENOMEM, "host allocation failed"); }
    catch (const std::exception& e) { return fail(c, OPMGPU_EINVAL, e.what()); }
}

int make_ctx(opmgpu_ctx** out, int device, const opmgpu_params* params)
{
    if (!out) return OPMGPU_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1 || device < 0 || device >= n) return OPMGPU_ENODEVICE;   // no CPU fallback
    std::unique_ptr<opmgpu_ctx> c(new opmgpu_ctx());
    c->device = device;
    if (params) c->prm = *params; else opmgpu_default_params(&c->prm);
    if (hipSetDevice(device) != hipSuccess) return OPMGPU_ENODEVICE;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return OPMGPU_ENODEVICE;
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) return OPMGPU_ENODEVICE;
    for (auto& pr : c->evp) for (auto& e : pr) if (hipEventCreate(&e) != hipSuccess) return OPMGPU_ENODEVICE;
    try { c->ls.reset(new LinSolver(c->stream)); } catch (const HipError& e) { return e.code; }
    *out = c.release();
    return OPMGPU_OK;
}

enum { PH_ASSEMBLE = 0, PH_SOLVE = 1, PH_UPDATE = 2 };
struct Timed {
    opmgpu_ctx* c; int ph;
    hipEvent_t e1 = nullptr;
    Timed(opmgpu_ctx* c_, int phase) : c(c_), ph(phase) {
        if (c->cur_mark) {                  // iteration marks: this call's own event pair (resolved by opmgpu_iteration_marks_get)
            hipEvent_t e0 = c->mark_event();
            e1 = c->mark_event();
            if (e0 && e1) {
                // a phase that runs twice in one call (never today) keeps its last pair
                for (auto& e : c->cur_mark->ph[ph]) if (e) { c->mark_pool.push_back(e); e = nullptr; }
                c->cur_mark->ph[ph][0] = e0; c->cur_mark->ph[ph][1] = e1;
                (void)hipEventRecord(e0, c->stream);
                return;
            }
            e1 = nullptr;
        }
        c->ev_pending[ph] = false; (void)hipEventRecord(c->evp[ph][0], c->stream);
    }
    ~Timed() { if (e1) { (void)hipEventRecord(e1, c->stream); return; } (void)hipEventRecord(c->evp[ph][1], c->stream); c->ev_pending[ph] = true; }
};

// the precision dispatch of this file: f(float()) for a single-precision matrix / solve, f(double()) otherwise
template <class F> auto by_precision(bool single, F&& f) { if (single) return f(float()); return f(double()); }

// what the status of LinSolver::solve means for the context: a refused call (OPMGPU_EINVAL) leaves `factored` untouched, a singular diagonal
// block clears it, every other return sets it
int solved(opmgpu_ctx* c, int st) { if (st != OPMGPU_EINVAL) c->factored = st != OPMGPU_ESINGULAR; return st; }

// the CPR diagnostics read the hierarchy of the last CPR solve in the precision it ran in
bool cpr_float(opmgpu_ctx* c) { return c->cur_single == 1 || c->ls->now.mixed; }

} // namespace

static thread_local std::string create_err;      // why the thread's last opmgpu_create was refused (that context is gone): opmgpu_last_error(NULL)

extern "C" {

const char* opmgpu_version(void) { return "opmgpu 0.1 (gfx950, HIP, SELL-64 block-ILU0/BiCGStab + black-oil assembly)"; }

int opmgpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void opmgpu_default_params(opmgpu_params* p)
{
    if (!p) return;
    p->dp_max_rel = 0.3; p->ds_max = 0.2; p->dr_max_rel = 1e9;                 // BlackoilModelParameters.cpp:76-102
    p->max_residual_allowed = 1e7; p->tolerance_mb = 1e-5; p->tolerance_cnv = 1e-2;
    p->matbalscale[0] = 1.1169; p->matbalscale[1] = 1.0031; p->matbalscale[2] = 0.0031;   // BlackoilModelBase_impl.hpp:139
    p->linear_solver_reduction = 1e-2; p->linear_solver_maxiter = 150;                    // FlowLinearSolverParameters
    p->ilu_relaxation = 0.9; p->ilu_ordering = OPMGPU_ORDER_MULTICOLOR; p->ignore_convergence_failure = 0; p->use_cpr = 0;
    p->newton_use_gmres = 0; p->linear_solver_restart = 40;                                // NewtonIterationBlackoilCPR.cpp:61-64
    p->solve_welleq_initially = 1; p->tolerance_wells = 1e-4; p->tolerance_well_control = 1e-7; p->dbhp_max_rel = 1.0; p->update_equations_scaling = 0; p->gmres_verify_residual = 0; p->cpr_reference_transform = 0;   // BlackoilModelParameters.cpp:80-96
    p->cpr_relax = 1.0; p->cpr_ilu_n = 0; p->cpr_use_amg = 0; p->cpr_use_bicgstab = 1;       // NewtonIterationBlackoilCPR.hpp:59-63
    p->ilu_fillin_level = 0;                                                                   // ISTLSolver.hpp:205
    p->cpr_solver_tol = 1e-2; p->cpr_stage2_relax = 1.0; p->preconditioner_single = 0; p->cpr_max_ell_iter = 25;                                       // external CPRPreconditioner (recollection, see opmgpu.h)
}

int opmgpu_create_solver(opmgpu_ctx** ctx, int device, const opmgpu_params* params) { return make_ctx(ctx, device, params); }

int opmgpu_create(opmgpu_ctx** ctx, int device, const opmgpu_grid* grid, const opmgpu_tables* tables, const opmgpu_params* params)
{
    create_err.clear();
    if (!grid || !tables || grid->nc <= 0 || grid->nconn < 0) return OPMGPU_EINVAL;
    // refused before any device call (so also where there is no device): a decomposed context takes its local grid through here as well
    try { BlackoilDevice::check_transmissibilities(grid); }
    catch (const HipError& e) { if (ctx) *ctx = nullptr; create_err = e.what(); return e.code; }
    const int st = make_ctx(ctx, device, params);
    if (st != OPMGPU_OK) return st;
    opmgpu_ctx* c = *ctx;
    const int st2 = guarded(c, [&]() { c->model.reset(new BlackoilDevice(c->stream, *c->ls, grid, tables, &c->prm)); return OPMGPU_OK; });
    if (st2 != OPMGPU_OK) { create_err = c->err; opmgpu_destroy(c); *ctx = nullptr; }
    return st2;
}

void opmgpu_destroy(opmgpu_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->model.reset(); c->ls.reset(); c->comm.reset();
    c->marks_clear(true);
    for (auto& pr : c->evp) for (auto& e : pr) if (e) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* opmgpu_last_error(const opmgpu_ctx* c) { return c ? c->err.c_str() : (create_err.empty() ? "null context" : create_err.c_str()); }

int opmgpu_set_wells(opmgpu_ctx* c, int nw, const int32_t* well_connpos, const int32_t* well_cells)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        c->matrix_loaded = false;
        if (c->comm && nw > 0) return fail(c, OPMGPU_EINVAL, "wells are not supported in multi-GPU mode yet");
        return c->model->set_wells(nw, well_connpos, well_cells);
    });
}

int opmgpu_set_state(opmgpu_ctx* c, const double* p, const double* sat, const double* rs, const double* rv, const int8_t* hc)
{
    if (!c || !c->model || !p || !sat || !rs || !rv || !hc) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->set_state(p, sat, rs, rv, hc); return OPMGPU_OK; });
}
int opmgpu_get_state(opmgpu_ctx* c, double* p, double* sat, double* rs, double* rv, int8_t* hc)
{
    if (!c || !c->model || !c->model->has_state) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->get_state(p, sat, rs, rv, hc); return OPMGPU_OK; });
}

int opmgpu_assemble(opmgpu_ctx* c, double dt, int initial, const double* p, const double* sat, const double* rs, const double* rv, const int8_t* hc)
{
    if (!c || !c->model || !(dt > 0.0)) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        if (p || sat || rs || rv || hc) {
            if (!(p && sat && rs && rv && hc)) return fail(c, OPMGPU_EINVAL, "state pointers must be all set or all NULL");
            c->model->set_state(p, sat, rs, rv, hc);
        }
        if (!c->model->has_state) return fail(c, OPMGPU_EINVAL, "no reservoir state on the device");
        c->t_phase[PH_SOLVE] = 0.0; c->t_phase[PH_UPDATE] = 0.0;       // a Newton iteration that converges here runs no solve / update
        c->ev_pending[PH_SOLVE] = false; c->ev_pending[PH_UPDATE] = false;
        {
            Timed t(c, PH_ASSEMBLE);
            c->model->assemble(dt, initial != 0);
        }
        c->matrix_loaded = true; c->factored = false; c->cur_single = -1; c->ls->ref_transformed = false;
        return int(OPMGPU_OK);
    });
}

int opmgpu_cpr_elliptic_stats(opmgpu_ctx* c, int64_t* solves, int64_t* iterations)
{
    if (!c || !c->ls) return OPMGPU_EINVAL;
    if (solves) *solves = c->ls->ell_solves;
    if (iterations) *iterations = c->ls->ell_iterations;
    return OPMGPU_OK;
}

int opmgpu_cpr_correction_factors(opmgpu_ctx* c, double* into_level0, double* below)
{
    if (!c || !c->ls) return OPMGPU_EINVAL;
    return by_precision(cpr_float(c), [&](auto tag) {
        auto* H = c->ls->cpr_hierarchy<decltype(tag)>();
        if (!H) return int(OPMGPU_EINVAL);
        if (into_level0) *into_level0 = H->pdamp0;
        if (below) *below = H->pdamp;
        return int(OPMGPU_OK);
    });
}

// diagnostics of the CPR pressure hierarchy (LinSolver, cpr_inspect.inl)
int opmgpu_cpr_elliptic_ilu_apply(opmgpu_ctx* c, const double* b, double* x)
{
    if (!c || !c->ls || !b || !x) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return by_precision(cpr_float(c), [&](auto tag) { return c->ls->cpr_elliptic_ilu_apply_host<decltype(tag)>(b, x); }); });
}
int opmgpu_cpr_levels(opmgpu_ctx* c, int32_t* nlevels, int32_t* n, int64_t* nnz, int32_t* nw)
{
    if (!c || !c->ls || !nlevels) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return by_precision(cpr_float(c), [&](auto tag) { return c->ls->cpr_levels<decltype(tag)>(nlevels, n, nnz, nw); }); });
}
int opmgpu_cpr_level_get(opmgpu_ctx* c, int level, int32_t* rowptr, int32_t* col, double* val, int32_t* agg, double* dense_inv)
{
    if (!c || !c->ls) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return by_precision(cpr_float(c), [&](auto tag) { return c->ls->cpr_level_get<decltype(tag)>(level, rowptr, col, val, agg, dense_inv); }); });
}
int opmgpu_cpr_dist_levels(opmgpu_ctx* c, int32_t* nlevels, int32_t* ndist)
{
    if (!c || !c->ls || !nlevels || !ndist) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return by_precision(cpr_float(c), [&](auto tag) {
        auto* H = c->ls->cpr_hierarchy<decltype(tag)>();
        if (H) { *nlevels = int32_t(H->levels.size()); *ndist = H->ndist; }
        return int(H ? OPMGPU_OK : OPMGPU_EINVAL);
    }); });
}
int opmgpu_cpr_dist_level_get(opmgpu_ctx* c, int level, int64_t* counts, int64_t* row_gid, int32_t* rowptr, int64_t* col_gid, double* val, int64_t* agg_gid)
{
    if (!c || !c->ls) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return by_precision(cpr_float(c), [&](auto tag) { return c->ls->cpr_dist_level_get<decltype(tag)>(level, counts, row_gid, rowptr, col_gid, val, agg_gid); }); });
}
int opmgpu_cpr_vcycle_apply(opmgpu_ctx* c, const double* b, double* x)
{
    if (!c || !c->ls || !b || !x) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return by_precision(cpr_float(c), [&](auto tag) { return c->ls->cpr_vcycle_apply_host<decltype(tag)>(b, x); }); });
}
int opmgpu_cpr_apply(opmgpu_ctx* c, const double* d3, double* v3)
{
    if (!c || !c->ls || !d3 || !v3) return OPMGPU_EINVAL;
    if (!c->factored) return fail(c, OPMGPU_EINVAL, "no factored CPR solve yet");
    const double relax = cpr_stage2_relaxation(c->prm);          // what solve() hands the solvers under CPR
    return guarded(c, [&]() { return by_precision(cpr_float(c), [&](auto tag) { return c->ls->cpr_apply_host<decltype(tag)>(d3, v3, relax); }); });
}

int opmgpu_get_matbalscale(opmgpu_ctx* c, double* scale3)
{
    if (!c || !c->model || !scale3) return OPMGPU_EINVAL;
    for (int a = 0; a < 3; ++a) scale3[a] = c->model->prm.matbalscale[a];
    return OPMGPU_OK;
}

int opmgpu_set_solve_precision(opmgpu_ctx* c, int single_precision)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    c->model->assemble_single = single_precision != 0;
    return OPMGPU_OK;
}

int opmgpu_perf_props(opmgpu_ctx* c, double* out)
{
    if (!c || !c->model || !out) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->perf_props(out); return OPMGPU_OK; });
}

int opmgpu_add_well_terms(opmgpu_ctx* c, const double* resid_delta, int nblk, const int32_t* schur_rc, const double* schur_blocks)
{
    if (!c || !c->model || nblk < 0 || (nblk > 0 && (!schur_rc || !schur_blocks))) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->factored = false; c->cur_single = -1; return c->model->add_well_terms(resid_delta, nblk, schur_rc, schur_blocks); });
}

int opmgpu_add_well_rhs(opmgpu_ctx* c, const double* rhs_delta)
{
    if (!c || !c->model || !rhs_delta) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->add_well_rhs(rhs_delta); return OPMGPU_OK; });
}
int opmgpu_perf_dx(opmgpu_ctx* c, double* out)
{
    if (!c || !c->model || !out || !c->model->has_dx) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->perf_dx(out); return OPMGPU_OK; });
}

int opmgpu_convergence(opmgpu_ctx* c, double dt, double* B_avg3, double* CNV3, double* MB3, double* linf3, int* converged)
{
    if (!c || !c->model || !c->matrix_loaded) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        const int st = c->model->convergence(dt, B_avg3, CNV3, MB3, linf3, converged);
        if (st == OPMGPU_ENUMERICAL) c->err = "NaN or too large residual";
        return st;
    });
}

int opmgpu_solve(opmgpu_ctx* c, int single_precision, double* dx, int* iters, double* reduction)
{
    if (!c || !c->model || !c->matrix_loaded) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        SolveResult res;
        int st;
        {
            Timed t(c, PH_SOLVE);
            struct MirrorScope { LinSolver& ls; ~MirrorScope() { ls.solution_mirror = nullptr; ls.mirror_written = false; } } scope{ *c->ls };      // (also when the solve throws)
            st = by_precision(single_precision != 0, [&](auto tag) {
                using S = decltype(tag);
                c->ls->ensure_work<S>(); c->model->build_rhs<S>();
                if (sizeof(S) == 8) c->ls->solution_mirror = c->model->dx_device();          // a GMRES solve stores its solution there too: store_dx then has nothing to copy
                const int s = solved(c, c->ls->solve<S>(c->prm, true, res, c->err));
                if (s == OPMGPU_OK || s == OPMGPU_ELINSOLVE) c->model->store_dx<S>();
                return s;
            });
        }
        c->cur_single = single_precision ? 1 : 0;
        if (iters) *iters = res.iterations;
        if (reduction) *reduction = res.reduction;
        if (dx && (st == OPMGPU_OK || st == OPMGPU_ELINSOLVE)) c->model->dx_to_host(dx);
        return st;
    });
}

int opmgpu_update_state(opmgpu_ctx* c, const double* dx, double relax)
{
    if (!c || !c->model || !c->model->has_state) return OPMGPU_EINVAL;
    if (!dx && !c->model->has_dx) return fail(c, OPMGPU_EINVAL, "no resident Newton increment");
    return guarded(c, [&]() {
        Timed t(c, PH_UPDATE);
        c->model->update_state(dx, relax);
        return OPMGPU_OK;
    });
}

int opmgpu_set_device_wells(opmgpu_ctx* c, const opmgpu_wells* wells)
{
    if (!c || !c->model || !wells) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        c->matrix_loaded = false;
        // multi-GPU: a well lives on ONE rank (the reference hands the wells to loadBalance for the same reason,
        // RedistributeDataHandles.hpp:559-560): every perforated cell must be an owned cell of this rank
        if (c->comm && wells->nw > 0 && wells->well_connpos && wells->well_cells)
            for (int j = 0; j < wells->well_connpos[wells->nw]; ++j)
                if (wells->well_cells[j] >= c->model->n_owned_cells) return fail(c, OPMGPU_EINVAL, "multi-GPU: a well perforates a ghost cell; keep every well on one rank");
        c->ls->run_has_wells = true; c->ls->cs_for = nullptr;       // the coarse space of the pressure stage keeps one unknown per rank then
        const int st = c->model->set_device_wells(wells);
        if (st != OPMGPU_OK) return fail(c, st, "invalid well specification (missing array or cell out of range)");
        return st;
    });
}
int opmgpu_set_well_efficiency(opmgpu_ctx* c, const double* factors)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    // the next assembly reads the new factors; a matrix loaded or factored before the call is that of the old ones
    return guarded(c, [&]() { const int st = c->model->set_well_efficiency(factors); c->matrix_loaded = false; return st; });
}
int opmgpu_set_well_groups(opmgpu_ctx* c, int ngroups, const int32_t* group_ptr, const int32_t* group_wells, const double* sign, const double* target,
                           const double* distr, const double* guide)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    // the next assembly takes the well equations' targets from the groups: a matrix loaded or factored before the call is the old one's
    return guarded(c, [&]() { const int st = c->model->set_well_groups(ngroups, group_ptr, group_wells, sign, target, distr, guide); c->matrix_loaded = false; return st; });
}
int opmgpu_get_well_group_targets(opmgpu_ctx* c, double* slot_target, double* group_rate)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return c->model->get_well_group_targets(slot_target, group_rate); });
}
int opmgpu_well_shared_cells(opmgpu_ctx* c, int32_t* shared_rows, int32_t* max_wells_per_cell)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return c->model->well_shared_cells(shared_rows, max_wells_per_cell); });
}
int opmgpu_get_well_efficiency(opmgpu_ctx* c, double* factors)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    if (!factors) return fail(c, OPMGPU_EINVAL, "opmgpu_get_well_efficiency: factors is NULL");
    return guarded(c, [&]() { return c->model->get_well_efficiency(factors); });
}
int opmgpu_well_state_set(opmgpu_ctx* c, const double* bhp, const double* qs, const double* perf_press, const double* perf_rates)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return c->model->well_state_set(bhp, qs, perf_press, perf_rates); });
}
int opmgpu_well_state_get(opmgpu_ctx* c, double* bhp, double* qs, double* perf_press, double* perf_rates)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return c->model->well_state_get(bhp, qs, perf_press, perf_rates); });
}
int opmgpu_set_vfp_tables(opmgpu_ctx* c, int n, const opmgpu_vfp_table* tables)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        const int st = c->model->set_vfp_tables(n, tables);
        return st == OPMGPU_OK ? st : fail(c, st, "invalid VFP table (missing axis / data, empty axis, or more than 64 THP values)");
    });
}
int opmgpu_vfp_evaluate(opmgpu_ctx* c, int table, int n, const double* q, const double* thp, const double* alq, const double* bhp_in,
                        double* bhp_out, double* dbhp_dq, double* thp_out)
{
    if (!c || !c->model || n < 0 || (n > 0 && (!q || !thp || !alq || !bhp_in || !bhp_out || !dbhp_dq || !thp_out))) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        const int st = c->model->vfp_evaluate(table, n, q, thp, alq, bhp_in, bhp_out, dbhp_dq, thp_out);
        return st == OPMGPU_OK ? st : fail(c, st, "no VFP tables set, or no table with that index");
    });
}
int opmgpu_well_controls_set(opmgpu_ctx* c, const int32_t* current, const double* thp)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return c->model->well_controls_set(current, thp); });
}
int opmgpu_well_controls_set_targets(opmgpu_ctx* c, const double* target, const double* distr)
{
    if (!c || !c->model || (!target && !distr)) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return c->model->well_controls_set_targets(target, distr); });
}
int opmgpu_well_controls_get(opmgpu_ctx* c, int32_t* current, double* thp, int32_t* pre_its, int32_t* pre_conv)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return c->model->well_controls_get(current, thp, pre_its, pre_conv); });
}
int opmgpu_perf_pvt(opmgpu_ctx* c, const double* pressure, double* out)
{
    if (!c || !c->model || !pressure || !out || !c->model->has_state) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->perf_pvt(pressure, out); return OPMGPU_OK; });
}
int opmgpu_average_b(opmgpu_ctx* c, double* B3)
{
    if (!c || !c->model || !B3 || !c->matrix_loaded) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->average_b(B3); return OPMGPU_OK; });
}
int opmgpu_well_convergence(opmgpu_ctx* c, double* flux3, double* ctrl)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        const int st = c->model->well_convergence(flux3, ctrl);
        // the statuses the reference's time stepper catches, with a text: a singular 4 x 4 well block is Dune::MatrixBlockError's case (the inverse in
        // eliminateVariable / solveWellEq), the other marks are NumericalIssue's (StandardWells_impl.hpp:742-748, NonlinearSolver_impl.hpp:165)
        if (st == OPMGPU_ESINGULAR) return fail(c, st, "singular well equation block (no open perforation can carry the well's flow)");
        if (st == OPMGPU_ENUMERICAL) return fail(c, st, "well model: non-finite or too large well residual, no consistent control, or the pre-solve gave up");
        return st;
    });
}

static int nonlinear_iteration_body(opmgpu_ctx* c, double dt, int iteration, int single_precision, const opmgpu_newton_ctl* ctl, int* converged,
                                    int* linear_iterations, double* linf3, double* relaxation, int* solved);

int opmgpu_nonlinear_iteration(opmgpu_ctx* c, double dt, int iteration, int single_precision, const opmgpu_newton_ctl* ctl, int* converged,
                               int* linear_iterations, double* linf3, double* relaxation)
{
    if (!c || !c->model || !ctl || !converged || iteration < 0) return OPMGPU_EINVAL;
    int solved = 0, lin = 0;
    if (!c->marks_on) return nonlinear_iteration_body(c, dt, iteration, single_precision, ctl, converged, linear_iterations ? linear_iterations : &lin, linf3, relaxation, &solved);
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, OPMGPU_ENODEVICE, "hipSetDevice failed");
    if (c->marks.size() >= opmgpu_ctx::kMaxMarks) {      // the list is full: the call runs unmarked
        ++c->marks_dropped;
        return nonlinear_iteration_body(c, dt, iteration, single_precision, ctl, converged, linear_iterations ? linear_iterations : &lin, linf3, relaxation, &solved);
    }
    if (!c->mark_start) { c->mark_start = c->mark_event(); if (!c->mark_start) return OPMGPU_ENODEVICE; (void)hipEventRecord(c->mark_start, c->stream); }
    c->marks.emplace_back();
    c->cur_mark = &c->marks.back();
    if (!linear_iterations) linear_iterations = &lin;
    const int st = nonlinear_iteration_body(c, dt, iteration, single_precision, ctl, converged, linear_iterations, linf3, relaxation, &solved);
    opmgpu_ctx::IterMark& m = c->marks.back();
    m.solved = solved; m.lin = *linear_iterations; m.status = st;
    m.end = c->mark_event();
    if (m.end) (void)hipEventRecord(m.end, c->stream);
    c->cur_mark = nullptr;
    return st;
}

int opmgpu_iteration_marks(opmgpu_ctx* c, int enable)
{
    if (!c) return OPMGPU_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, OPMGPU_ENODEVICE, "hipSetDevice failed");
    c->marks_clear();
    c->marks_on = enable != 0;
    return OPMGPU_OK;
}

int opmgpu_iteration_marks_get(opmgpu_ctx* c, int max_calls, double* call_ms, int32_t* solved, int32_t* linear_iterations, double* phase_ms, int* n_calls)
{
    if (!c || !n_calls || max_calls < 0) return OPMGPU_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, OPMGPU_ENODEVICE, "hipSetDevice failed");
    const int n = std::min<int>(max_calls, int(c->marks.size()));
    *n_calls = int(c->marks.size() + c->marks_dropped);
    if (n > 0 && c->marks[n - 1].end && hipEventSynchronize(c->marks[n - 1].end) != hipSuccess) return fail(c, OPMGPU_ENODEVICE, "hipEventSynchronize failed");
    hipEvent_t prev = c->mark_start;
    for (int i = 0; i < n; ++i) {
        const opmgpu_ctx::IterMark& m = c->marks[i];
        float ms = 0.f;
        if (call_ms) { call_ms[i] = (prev && m.end && hipEventElapsedTime(&ms, prev, m.end) == hipSuccess) ? double(ms) : -1.0; }
        if (solved) solved[i] = m.solved;
        if (linear_iterations) linear_iterations[i] = m.lin;
        if (phase_ms) for (int ph = 0; ph < 3; ++ph) {
            float pm = 0.f;
            phase_ms[3 * i + ph] = (m.ph[ph][0] && m.ph[ph][1] && hipEventSynchronize(m.ph[ph][1]) == hipSuccess && hipEventElapsedTime(&pm, m.ph[ph][0], m.ph[ph][1]) == hipSuccess) ? double(pm) : 0.0;
        }
        if (m.end) prev = m.end;
    }
    return OPMGPU_OK;
}

static int nonlinear_iteration_body(opmgpu_ctx* c, double dt, int iteration, int single_precision, const opmgpu_newton_ctl* ctl, int* converged,
                                    int* linear_iterations, double* linf3, double* relaxation, int* solved)
{
    if (iteration == 0) { c->norm_history.clear(); c->relaxation = 1.0; }
    if (int(c->norm_history.size()) != iteration) return fail(c, OPMGPU_EINVAL, "opmgpu_nonlinear_iteration: iterations of a time step must be consecutive from 0");
    *converged = 0;
    if (linear_iterations) *linear_iterations = 0;
    int st = opmgpu_set_solve_precision(c, single_precision);
    if (st == OPMGPU_OK) st = opmgpu_assemble(c, dt, iteration == 0 ? 1 : 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (st != OPMGPU_OK) return st;
    double B[3], CNV[3], MB[3], linf[3];
    int conv = 0;
    st = opmgpu_convergence(c, dt, B, CNV, MB, linf, &conv);
    if (st != OPMGPU_OK) return st;
    if (c->model->has_device_wells()) {                    // getWellConvergence (:1769-1779)
        double flux[3], ctrl = 0.0;
        st = opmgpu_well_convergence(c, flux, &ctrl);
        if (st != OPMGPU_OK) return st;
        bool ok = ctrl < c->prm.tolerance_well_control;
        for (int a = 0; a < 3; ++a) ok = ok && (B[a] * flux[a] < c->prm.tolerance_wells);
        conv = conv && ok;
    }
    c->norm_history.push_back({ linf[0], linf[1], linf[2] });
    if (linf3) for (int a = 0; a < 3; ++a) linf3[a] = linf[a];
    *converged = conv;
    if (!conv || iteration < ctl->min_iter) {
        int its = 0;
        *solved = 1;
        st = opmgpu_solve(c, single_precision, nullptr, &its, nullptr);
        if (linear_iterations) *linear_iterations = its;
        if (st != OPMGPU_OK) return st;
        if (ctl->use_update_stabilization) {
            // the oscillation rule of NonlinearSolver_impl.hpp:221-257 (only the three mass-balance norms take part): a phase swings when its
            // norm is back within relax_rel_tol of its value two iterations ago but not of last iteration's; two swinging phases oscillate
            bool oscillate = false;
            if (iteration >= 2) {
                const auto &now = c->norm_history[iteration], &last = c->norm_history[iteration - 1], &before = c->norm_history[iteration - 2];
                int swinging = 0;
                for (int ph = 0; ph < 3; ++ph) {
                    const double to_before = std::fabs((now[ph] - before[ph]) / now[ph]), to_last = std::fabs((now[ph] - last[ph]) / now[ph]);
                    if (to_before < ctl->relax_rel_tol && ctl->relax_rel_tol < to_last) ++swinging;
                }
                oscillate = swinging >= 2;
            }
            if (oscillate) c->relaxation = std::max(c->relaxation - ctl->relax_increment, ctl->relax_max);
            st = opmgpu_stabilize_update(c, ctl->relax_type, c->relaxation);
            if (st != OPMGPU_OK) return st;
        }
        st = opmgpu_update_state(c, nullptr, 1.0);
    }
    if (relaxation) *relaxation = c->relaxation;
    return st;
}

int opmgpu_save_state(opmgpu_ctx* c)
{
    if (!c || !c->model || !c->model->has_state) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->save_state(); return OPMGPU_OK; });
}
int opmgpu_restore_state(opmgpu_ctx* c)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    if (!c->model->has_saved) return fail(c, OPMGPU_EINVAL, "no saved state (opmgpu_save_state; a well re-plan discards it)");
    return guarded(c, [&]() { c->model->restore_state(); return OPMGPU_OK; });
}
int opmgpu_compute_fluid_in_place(opmgpu_ctx* c, const int32_t* fipnum, int nregions, double* fip_cells, double* values)
{
    if (!c || !c->model || !values || nregions < 1) return OPMGPU_EINVAL;
    if (!c->model->has_state) return fail(c, OPMGPU_EINVAL, "no reservoir state on the device");
    if (fipnum) for (int i = 0; i < c->model->nc; ++i) if (fipnum[i] < 0 || fipnum[i] > nregions) return fail(c, OPMGPU_EINVAL, "fipnum outside [0, nregions]");
    return guarded(c, [&]() { c->model->fluid_in_place(fipnum, nregions, fip_cells, values); return int(OPMGPU_OK); });
}
int opmgpu_set_threshold_pressures(opmgpu_ctx* c, const double* thpres)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->set_threshold_pressures(thpres); return int(OPMGPU_OK); });
}
int opmgpu_set_pvcdo(opmgpu_ctx* c, const double* pvcdo)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->set_pvcdo(pvcdo); return int(OPMGPU_OK); });
}
int opmgpu_compute_max_dp(opmgpu_ctx* c, const int32_t* eqlnum, int nregions, int n_face_conn, double* dp_conn, double* max_dp)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    if (!eqlnum || !max_dp || nregions < 1) return fail(c, OPMGPU_EINVAL, "computeMaxDp: eqlnum and max_dp must be given, nregions >= 1");
    if (n_face_conn < 0 || n_face_conn > c->model->nconn) return fail(c, OPMGPU_EINVAL, "computeMaxDp: n_face_conn outside [0, nconn]");
    if (!c->model->has_state) return fail(c, OPMGPU_EINVAL, "no reservoir state on the device");
    for (int i = 0; i < c->model->nc; ++i) if (eqlnum[i] < 1 || eqlnum[i] > nregions) return fail(c, OPMGPU_EINVAL, "computeMaxDp: eqlnum outside [1, nregions]");
    return guarded(c, [&]() { c->model->compute_max_dp(eqlnum, nregions, n_face_conn, dp_conn, max_dp); return int(OPMGPU_OK); });
}
int opmgpu_set_swatinit_scaling(opmgpu_ctx* c, const double* sw, const double* pcow, double* sw_out)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    if (!sw || !pcow) return fail(c, OPMGPU_EINVAL, "setSwatInitScaling: sw and pcow must be given");
    return guarded(c, [&]() { c->model->set_swatinit_scaling(sw, pcow, sw_out); return int(OPMGPU_OK); });
}
int opmgpu_get_pcw(opmgpu_ctx* c, double* pcw)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    if (!pcw) return fail(c, OPMGPU_EINVAL, "get_pcw: pcw must be given");
    return guarded(c, [&]() { c->model->get_pcw(pcw); return int(OPMGPU_OK); });
}
int opmgpu_cap_press(opmgpu_ctx* c, const double* sat, double* pc)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    if (!pc) return fail(c, OPMGPU_EINVAL, "capPress: pc must be given");
    if (!sat && !c->model->has_state) return fail(c, OPMGPU_EINVAL, "capPress: no saturations given and no reservoir state on the device");
    return guarded(c, [&]() { c->model->cap_press(sat, pc); return int(OPMGPU_OK); });
}
int opmgpu_get_simulator_data(opmgpu_ctx* c, double* out)
{
    if (!c || !c->model || !out || !c->model->has_state) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->simulator_data(out); return int(OPMGPU_OK); });
}

int opmgpu_region_state_sums(opmgpu_ctx* c, const int32_t* region, int nregions, double* sums)
{
    if (!c || !c->model || !sums || nregions < 1) return OPMGPU_EINVAL;
    if (!c->model->has_state) return fail(c, OPMGPU_EINVAL, "no reservoir state on the device");
    return guarded(c, [&]() { c->model->region_state_sums(region, nregions, sums); return int(OPMGPU_OK); });
}
int opmgpu_voidage_coefficients(opmgpu_ctx* c, int n, const double* p, const double* rs, const double* rv, const int32_t* pvt_region, double* coeff)
{
    if (!c || !c->model || n < 0 || (n > 0 && (!p || !rs || !rv || !coeff))) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->voidage_coefficients(n, p, rs, rv, pvt_region, coeff); return int(OPMGPU_OK); });
}

int opmgpu_relative_change(opmgpu_ctx* c, double* value)
{
    if (!c || !c->model || !value) return OPMGPU_EINVAL;
    if (!c->model->has_saved) return fail(c, OPMGPU_EINVAL, "no saved state (opmgpu_save_state; a well re-plan discards it)");
    return guarded(c, [&]() { *value = c->model->relative_change(); return OPMGPU_OK; });
}

int opmgpu_set_sat_oil_max(opmgpu_ctx* c, const double* so_max)
{
    if (!c || !c->model || !so_max) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->set_sat_oil_max(so_max); return OPMGPU_OK; });
}
int opmgpu_update_sat_oil_max(opmgpu_ctx* c)
{
    if (!c || !c->model || !c->model->has_state) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->update_sat_oil_max(); return OPMGPU_OK; });
}
int opmgpu_get_sat_oil_max(opmgpu_ctx* c, double* so_max)
{
    if (!c || !c->model || !so_max) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->get_sat_oil_max(so_max); return OPMGPU_OK; });
}

// DRSDT / DRVDT (the rule is stated in opmgpu.h).  The limits change what the next assembly evaluates: a matrix loaded or factored before
// the call is that of the old ones.
int opmgpu_set_dissolution_limits(opmgpu_ctx* c, double drsdt, int drsdt_free_only, double drvdt)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->set_dissolution_limits(drsdt, drsdt_free_only, drvdt); c->matrix_loaded = false; return int(OPMGPU_OK); });
}
int opmgpu_begin_dissolution_step(opmgpu_ctx* c, double dt)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->begin_dissolution_step(dt); c->matrix_loaded = false; return int(OPMGPU_OK); });
}
int opmgpu_get_dissolution_caps(opmgpu_ctx* c, double* rs_cap, double* rv_cap)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->get_dissolution_caps(rs_cap, rv_cap); return int(OPMGPU_OK); });
}
int opmgpu_set_dissolution_caps(opmgpu_ctx* c, const double* rs_cap, const double* rv_cap)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->set_dissolution_caps(rs_cap, rv_cap); c->matrix_loaded = false; return int(OPMGPU_OK); });
}

// Analytic aquifers (the rule is stated in opmgpu.h).  A new set, a begun step and a changed state change what the next assembly adds: a
// matrix loaded or factored before the call is that of the old terms.
int opmgpu_set_aquifers(opmgpu_ctx* c, const opmgpu_aquifers* aquifers)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->set_aquifers(aquifers); c->matrix_loaded = false; return int(OPMGPU_OK); });
}
int opmgpu_aquifer_begin_step(opmgpu_ctx* c, double dt)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->aquifer_begin_step(dt); c->matrix_loaded = false; return int(OPMGPU_OK); });
}
int opmgpu_aquifer_commit_step(opmgpu_ctx* c)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->aquifer_commit_step(); c->matrix_loaded = false; return int(OPMGPU_OK); });
}
int opmgpu_aquifer_state_get(opmgpu_ctx* c, double* W_e, double* W_s, double* t, double* p_a)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->aquifer_state_get(W_e, W_s, t, p_a); return int(OPMGPU_OK); });
}
int opmgpu_aquifer_state_set(opmgpu_ctx* c, const double* W_e, const double* W_s, const double* t)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->aquifer_state_set(W_e, W_s, t); c->matrix_loaded = false; return int(OPMGPU_OK); });
}
int opmgpu_aquifer_connections_get(opmgpu_ctx* c, double* out)
{
    if (!c || !c->model || !out) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->aquifer_connections_get(out); return int(OPMGPU_OK); });
}

// Rock regions and irreversible compaction (the rule is stated in opmgpu.h).  Regions and history change what the next assembly evaluates:
// a matrix loaded or factored before the call is that of the old ones.
int opmgpu_set_rock_regions(opmgpu_ctx* c, const opmgpu_rock_regions* regions)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->set_rock_regions(regions); c->matrix_loaded = false; return int(OPMGPU_OK); });
}
int opmgpu_update_rock_history(opmgpu_ctx* c)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->update_rock_history(); c->matrix_loaded = false; return int(OPMGPU_OK); });
}
int opmgpu_get_rock_history(opmgpu_ctx* c, double* p_min)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    if (!p_min) return fail(c, OPMGPU_EINVAL, "opmgpu_get_rock_history: p_min is NULL");
    return guarded(c, [&]() { c->model->get_rock_history(p_min); return int(OPMGPU_OK); });
}
int opmgpu_set_rock_history(opmgpu_ctx* c, const double* p_min)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->set_rock_history(p_min); c->matrix_loaded = false; return int(OPMGPU_OK); });
}
int opmgpu_get_rock_multipliers(opmgpu_ctx* c, double* pv_mult, double* trans_mult)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->get_rock_multipliers(pv_mult, trans_mult); return int(OPMGPU_OK); });
}

int opmgpu_update_hysteresis(opmgpu_ctx* c)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return c->model->update_hysteresis(); });
}
int opmgpu_set_hysteresis(opmgpu_ctx* c, const double* mdc_ow, const double* mdc_go)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return c->model->set_hysteresis(mdc_ow, mdc_go); });
}
int opmgpu_get_hysteresis(opmgpu_ctx* c, double* mdc_ow, double* mdc_go, double* d_ow, double* d_go)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return c->model->get_hysteresis(mdc_ow, mdc_go, d_ow, d_go); });
}
int opmgpu_set_hysteresis_model(opmgpu_ctx* c, int model, double killough_a)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    // the next assembly evaluates the new scanning curves; a matrix loaded or factored before the call is that of the old ones
    return guarded(c, [&]() { const int st = c->model->set_hysteresis_model(model, killough_a); c->matrix_loaded = false; return st; });
}
int opmgpu_get_hysteresis_scanning(opmgpu_ctx* c, double* sncrt_ow, double* m_ow, double* r_ow, double* sncrt_go, double* m_go, double* r_go)
{
    if (!c || !c->model) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return c->model->get_hysteresis_scanning(sncrt_ow, m_ow, r_ow, sncrt_go, m_go, r_go); });
}

int opmgpu_stabilize_update(opmgpu_ctx* c, int relax_type, double omega)
{
    if (!c || !c->model || (relax_type != OPMGPU_RELAX_DAMPEN && relax_type != OPMGPU_RELAX_SOR)) return OPMGPU_EINVAL;
    if (!c->model->has_dx) return fail(c, OPMGPU_EINVAL, "no resident Newton increment");
    return guarded(c, [&]() {
        c->model->stabilize_update(relax_type, omega);
        return OPMGPU_OK;
    });
}

int opmgpu_load_bsr(opmgpu_ctx* c, int nb, const int32_t* rowptr, const int32_t* col, const double* val9, int single_precision)
{
    if (!c || nb <= 0 || !rowptr || !col || !val9) return OPMGPU_EINVAL;
    if (c->model) return fail(c, OPMGPU_EINVAL, "opmgpu_load_bsr needs a solver-only context (opmgpu_create_solver)");
    return guarded(c, [&]() {
        const int st = c->ls->set_pattern(nb, rowptr, col, c->prm.ilu_ordering);
        if (st != OPMGPU_OK) return fail(c, st, "invalid BSR pattern");
        c->ls->load_host_bsr(val9);
        by_precision(single_precision != 0, [&](auto tag) { c->ls->prepare<decltype(tag)>(true); });
        c->cur_single = single_precision ? 1 : 0;
        c->matrix_loaded = true; c->factored = false; c->ls->ref_transformed = false;
        return int(OPMGPU_OK);
    });
}

int opmgpu_solve_bsr(opmgpu_ctx* c, int nb, const int32_t* rowptr, const int32_t* col, const double* val9, const double* rhs3,
                     int single_precision, double* x3, int* iters, double* reduction)
{
    if (!c || !rhs3 || !x3) return OPMGPU_EINVAL;
    const int st0 = opmgpu_load_bsr(c, nb, rowptr, col, val9, single_precision);
    if (st0 != OPMGPU_OK) return st0;
    return guarded(c, [&]() { return by_precision(single_precision != 0, [&](auto tag) {
        using S = decltype(tag);
        LinSolver& ls = *c->ls;
        SolveResult res; int st;
        {
            Timed t(c, PH_SOLVE);
            ls.vec_from_host<S>(rhs3, VEC_BLOCK_INTERLEAVED, ls.work<S>().b.p);
            st = solved(c, ls.solve<S>(c->prm, false, res, c->err));
        }
        if (iters) *iters = res.iterations;
        if (reduction) *reduction = res.reduction;
        if (st == OPMGPU_OK || st == OPMGPU_ELINSOLVE) ls.vec_to_host<S>(ls.work<S>().x.p, VEC_BLOCK_INTERLEAVED, x3);
        return st;
    }); });
}

// make sure the matrix exists in the precision the kernel-level entry points will use
static int ensure_prepared(opmgpu_ctx* c)
{
    if (!c->matrix_loaded) return fail(c, OPMGPU_EINVAL, "no matrix loaded");
    if (c->cur_single < 0) { c->ls->prepare<double>(true); c->cur_single = 0; }
    return OPMGPU_OK;
}

int opmgpu_spmv(opmgpu_ctx* c, const double* x3, double* y3)
{
    if (!c || !x3 || !y3) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        const int st = ensure_prepared(c); if (st) return st;
        LinSolver& ls = *c->ls;
        by_precision(c->cur_single != 0, [&](auto tag) { using S = decltype(tag); auto& w = ls.work<S>(); ls.vec_from_host<S>(x3, VEC_BLOCK_INTERLEAVED, w.p.p); ls.spmv<S>(w.p.p, w.v.p); ls.vec_to_host<S>(w.v.p, VEC_BLOCK_INTERLEAVED, y3); });
        return int(OPMGPU_OK);
    });
}

int opmgpu_ilu0_factor(opmgpu_ctx* c)
{
    if (!c) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        const int st = ensure_prepared(c); if (st) return st;
        const int fill = fill_level_of(c->prm);
        if (fill < 0) return fail(c, OPMGPU_EINVAL, kFillLevelRange);
        c->ls->fill_level = fill;
        const int s2 = by_precision(c->cur_single != 0, [&](auto tag) { return c->ls->factor<decltype(tag)>(); });
        c->factored = (s2 == OPMGPU_OK);
        return s2 == OPMGPU_OK ? int(OPMGPU_OK) : fail(c, s2, "singular diagonal block in ILU0");
    });
}

int opmgpu_ilu0_apply(opmgpu_ctx* c, const double* d3, double* v3)
{
    if (!c || !d3 || !v3) return OPMGPU_EINVAL;
    if (!c->factored) return fail(c, OPMGPU_EINVAL, "call opmgpu_ilu0_factor first");
    return guarded(c, [&]() {
        LinSolver& ls = *c->ls;
        by_precision(c->cur_single != 0, [&](auto tag) { using S = decltype(tag); auto& w = ls.work<S>(); ls.vec_from_host<S>(d3, VEC_BLOCK_INTERLEAVED, w.p.p); ls.ilu_apply<S>(w.p.p, w.y.p, c->prm.ilu_relaxation, nullptr); ls.vec_to_host<S>(w.y.p, VEC_BLOCK_INTERLEAVED, v3); });
        return int(OPMGPU_OK);
    });
}

int opmgpu_point_ilu_apply(opmgpu_ctx* c, const double* d3, double* v3, double relax)
{
    if (!c || !d3 || !v3) return OPMGPU_EINVAL;
    if (!c->ls || !c->ls->pilu.built || c->ls->pilu.stale) return fail(c, OPMGPU_EINVAL, "solve once with cpr_reference_transform = 2 first");
    return guarded(c, [&]() {
        LinSolver& ls = *c->ls;
        auto& w = ls.work<double>();
        ls.vec_from_host<double>(d3, VEC_BLOCK_INTERLEAVED, w.p.p);
        ls.point_ilu_apply(w.p.p, w.y.p, relax);
        ls.vec_to_host<double>(w.y.p, VEC_BLOCK_INTERLEAVED, v3);
        return int(OPMGPU_OK);
    });
}

int opmgpu_ilu0_get(opmgpu_ctx* c, double* val9)
{
    if (!c || !val9) return OPMGPU_EINVAL;
    if (!c->factored) return fail(c, OPMGPU_EINVAL, "call opmgpu_ilu0_factor first");
    if (c->ls->fill_level > 0) return fail(c, OPMGPU_EINVAL, "opmgpu_ilu0_get returns the ILU0 factors on the matrix's pattern: not with cpr_ilu_n / ilu_fillin_level > 0");
    return guarded(c, [&]() { by_precision(c->cur_single != 0, [&](auto tag) { c->ls->get_lu_bsr<decltype(tag)>(val9); }); return OPMGPU_OK; });
}

int opmgpu_get_ordering(opmgpu_ctx* c, int32_t* position, int32_t* level, int32_t* nlevels)
{
    if (!c || !c->ls->has_pattern()) return OPMGPU_EINVAL;
    const Plan& P = c->ls->plan;
    for (int i = 0; i < P.nb; ++i) { if (position) position[i] = P.pos[i]; if (level) level[i] = P.level[P.pos[i]]; }
    if (nlevels) *nlevels = P.nlevels;
    return OPMGPU_OK;
}

int opmgpu_get_cpr_weights(opmgpu_ctx* c, double* w)
{
    if (!c || !w || !c->ls->has_pattern()) return OPMGPU_EINVAL;
    return guarded(c, [&]() { return by_precision(c->cur_single == 1, [&](auto tag) {
        const auto& cprw = c->ls->work<decltype(tag)>().cprw;
        if (!cprw.p) return fail(c, OPMGPU_EINVAL, "no CPR solve yet");
        c->ls->vec_to_host<decltype(tag)>(cprw.p, VEC_EQUATION_MAJOR, w);
        return int(OPMGPU_OK);
    }); });
}

int opmgpu_get_residual(opmgpu_ctx* c, double* r)
{
    if (!c || !c->model || !r) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->model->get_residual(r); return OPMGPU_OK; });
}
int opmgpu_get_jacobian_nnzb(opmgpu_ctx* c, int32_t* nnzb)
{
    if (!c || !nnzb || !c->ls->has_pattern()) return OPMGPU_EINVAL;
    *nnzb = c->ls->plan.nnzb;
    return OPMGPU_OK;
}
int opmgpu_get_jacobian_bsr(opmgpu_ctx* c, int32_t* rowptr, int32_t* col, double* val9)
{
    if (!c || !c->ls->has_pattern()) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        const Plan& P = c->ls->plan;
        if (rowptr) std::memcpy(rowptr, P.rowptr.data(), sizeof(int32_t) * (P.nb + 1));
        if (col) std::memcpy(col, P.col.data(), sizeof(int32_t) * P.nnzb);
        if (val9) { c->ls->widen_matrix(); c->ls->get_matrix_bsr(c->ls->matrix_d(), val9); }
        return OPMGPU_OK;
    });
}

int opmgpu_get_jacobian_float_copy(opmgpu_ctx* c, double* val9)
{
    if (!c || !val9 || !c->ls->has_pattern()) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        if (c->ls->matrix_is_float || !c->ls->float_copy_valid)
            return fail(c, OPMGPU_EINVAL, "opmgpu_get_jacobian_float_copy: the context holds no float copy of a double Jacobian (the solve makes it then)");
        c->ls->get_float_copy_bsr(val9);
        return int(OPMGPU_OK);
    });
}

int opmgpu_time_kernel(opmgpu_ctx* c, int kernel, int reps, double* ms_per_launch)
{
    if (!c || reps < 1 || !ms_per_launch) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        if (kernel == OPMGPU_K_ASSEMBLE || kernel == OPMGPU_K_PROPS) {
            if (!c->model || !c->model->has_state) return fail(c, OPMGPU_EINVAL, "no model / state");
            *ms_per_launch = c->model->time_assemble(reps, kernel == OPMGPU_K_PROPS);
            c->factored = false; c->cur_single = -1; c->matrix_loaded = true; c->ls->ref_transformed = false;
            return int(OPMGPU_OK);
        }
        const int st = ensure_prepared(c); if (st) return st;
        by_precision(c->cur_single != 0, [&](auto tag) { c->ls->ensure_work<decltype(tag)>(); });
        if ((kernel == OPMGPU_K_ILU_APPLY) && !c->factored) return fail(c, OPMGPU_EINVAL, "call opmgpu_ilu0_factor first");
        *ms_per_launch = c->ls->time_kernel(kernel, reps, c->cur_single);
        return int(OPMGPU_OK);
    });
}

int opmgpu_kernel_timing(opmgpu_ctx* c, int enable)
{
    if (!c) return OPMGPU_EINVAL;
    return guarded(c, [&]() { c->ls->kt.reset(); c->ls->kt.on = enable != 0; return OPMGPU_OK; });
}
int opmgpu_kernel_timing_get(opmgpu_ctx* c, double* total_ms, int64_t* launches)
{
    if (!c || !total_ms) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        KernelTimers& kt = c->ls->kt;
        kt.collect();
        for (int i = 0; i < KT_COUNT; ++i) { total_ms[i] = kt.total_ms[i]; if (launches) launches[i] = kt.count[i]; }
        return OPMGPU_OK;
    });
}

int opmgpu_last_timings(opmgpu_ctx* c, double* assemble_ms, double* solve_ms, double* update_ms)
{
    if (!c) return OPMGPU_EINVAL;
    for (int ph = 0; ph < 3; ++ph) {
        if (!c->ev_pending[ph]) continue;
        float ms = 0.f;
        if (hipEventSynchronize(c->evp[ph][1]) == hipSuccess && hipEventElapsedTime(&ms, c->evp[ph][0], c->evp[ph][1]) == hipSuccess) c->t_phase[ph] = ms;
        c->ev_pending[ph] = false;
    }
    if (assemble_ms) *assemble_ms = c->t_phase[PH_ASSEMBLE];
    if (solve_ms) *solve_ms = c->t_phase[PH_SOLVE];
    if (update_ms) *update_ms = c->t_phase[PH_UPDATE];
    return OPMGPU_OK;
}

int opmgpu_comm_unique_id(uint8_t* id)
{
    if (!id) return OPMGPU_EINVAL;
    try { return RcclComm::unique_id(id); } catch (...) { return OPMGPU_ECOMM; }
}

static int comm_init_common(opmgpu_ctx* c, int rank, int nranks, const uint8_t* id, const opmgpu_transport* transport, int32_t n_owned, int n_neigh,
                            const int32_t* neigh_rank, const int32_t* send_ptr, const int32_t* send_cells, const int32_t* recv_ptr, const int32_t* recv_cells)
{
    if (!c || !c->model || (!id && !transport) || nranks < 1 || rank < 0 || rank >= nranks || n_owned <= 0 || n_owned > c->model->nc || n_neigh < 0) return OPMGPU_EINVAL;
    if (n_neigh > 0 && (!neigh_rank || !send_ptr || !send_cells || !recv_ptr || !recv_cells)) return OPMGPU_EINVAL;
    return guarded(c, [&]() {
        // the decomposed code sums a perforated row's well terms from one workgroup per well: refused before anything is attached
        if (c->model->shared_well_rows() > 0)
            return fail(c, OPMGPU_EINVAL, "multi-GPU: a cell is perforated by several wells; a decomposed run (a communicator is attached) does not support that");
        // a group's wells may sit on several ranks and the re-share is rank-local: refused here too, so that the context stays single-domain
        if (c->model->well_group_count() > 0)
            return fail(c, OPMGPU_EINVAL, "multi-GPU: controlled well groups are set; group control in a decomposed run (a communicator is attached) is not supported");
        // ghost cells' step-start rs / rv are not exchanged: the caps of a decomposed run are out of scope, so the context stays single-domain
        if (c->model->has_dissolution_limits())
            return fail(c, OPMGPU_EINVAL, "multi-GPU: dissolution limits (DRSDT / DRVDT) are set; a decomposed run (a communicator is attached) does not support them");
        // an aquifer's connections may sit on several ranks and its sums are rank-local: refused, so the context stays single-domain
        if (c->model->has_aquifers())
            return fail(c, OPMGPU_EINVAL, "multi-GPU: aquifers are set; a decomposed run (a communicator is attached) does not support them");
        std::unique_ptr<RcclComm> cm(new RcclComm());
        static const int32_t zero2[2] = { 0, 0 };
        const int st = cm->init(rank, nranks, id, transport, n_owned, c->model->nc, n_neigh, neigh_rank, n_neigh ? send_ptr : zero2, send_cells,
                                n_neigh ? recv_ptr : zero2, recv_cells);
        if (st != OPMGPU_OK) return fail(c, st, transport ? "invalid transport / neighbour lists" : "RCCL communicator initialisation failed");
        cm->rebuild(c->model->plan(), c->stream);
        c->ls->cpr_hier_mode = env_int("OPMGPU_CPR_GLOBAL_AMG", 0) == 1 ? 1 : 0;
        if (c->ls->cpr_hier_mode == 1 && env_flag("OPMGPU_AMG_GS", false)) {
            // the distributed cycle smooths by damped Jacobi only (opmgpu_comm_set_pressure_hierarchy refuses the pair): keep mode 0
            std::fprintf(stderr, "[opmgpu] OPMGPU_CPR_GLOBAL_AMG=1 ignored: OPMGPU_AMG_GS is set (level-0 Gauss-Seidel); the pressure hierarchy stays rank-local\n");
            c->ls->cpr_hier_mode = 0;
        }
        c->comm = std::move(cm);
        c->model->attach_comm(c->comm.get(), n_owned);
        c->matrix_loaded = false;
        return int(OPMGPU_OK);
    });
}

int opmgpu_comm_init(opmgpu_ctx* c, int rank, int nranks, const uint8_t* id, int32_t n_owned, int n_neigh, const int32_t* neigh_rank,
                     const int32_t* send_ptr, const int32_t* send_cells, const int32_t* recv_ptr, const int32_t* recv_cells)
{
    if (!id) return OPMGPU_EINVAL;
    return comm_init_common(c, rank, nranks, id, nullptr, n_owned, n_neigh, neigh_rank, send_ptr, send_cells, recv_ptr, recv_cells);
}

int opmgpu_comm_init_transport(opmgpu_ctx* c, int rank, int nranks, const opmgpu_transport* transport, int32_t n_owned, int n_neigh,
                               const int32_t* neigh_rank, const int32_t* send_ptr, const int32_t* send_cells, const int32_t* recv_ptr, const int32_t* recv_cells)
{
    if (!transport) return OPMGPU_EINVAL;
    return comm_init_common(c, rank, nranks, nullptr, transport, n_owned, n_neigh, neigh_rank, send_ptr, send_cells, recv_ptr, recv_cells);
}

int opmgpu_comm_set_coarse_blocks(opmgpu_ctx* c, int m, const int32_t* block_of_owned_cell)
{
    if (!c || !c->comm) return OPMGPU_EINVAL;
    const int st = c->comm->set_coarse_blocks(m, block_of_owned_cell);
    if (st != OPMGPU_OK) return fail(c, st, "opmgpu_comm_set_coarse_blocks: 0 <= block < m <= 8 for every owned cell");
    c->ls->cs_for = nullptr;           // the subdomain map is rebuilt (collectively) at the next CPR solve
    return OPMGPU_OK;
}

int opmgpu_comm_set_pressure_hierarchy(opmgpu_ctx* c, int mode)
{
    if (!c || !c->comm || !c->ls) return OPMGPU_EINVAL;
    if (mode != 0 && mode != 1) return fail(c, OPMGPU_EINVAL, "opmgpu_comm_set_pressure_hierarchy: mode 0 (rank-local) or 1 (distributed)");
    const char* gs = std::getenv("OPMGPU_AMG_GS");
    if (mode == 1 && gs && std::atoi(gs) != 0) return fail(c, OPMGPU_EINVAL, "opmgpu_comm_set_pressure_hierarchy: the distributed hierarchy smooths by damped Jacobi (OPMGPU_AMG_GS is set)");
    if (c->ls->cpr_hier_mode != mode) c->ls->drop_hierarchies();           // rebuilt (collectively) at the next CPR solve
    c->ls->cpr_hier_mode = mode;
    return OPMGPU_OK;
}

int opmgpu_plan_ordering(int nb, const int32_t* rowptr, const int32_t* col, int ordering, int32_t* position, int32_t* level, int32_t* nlevels)
{
    Plan P;
    const int st = build_plan(nb, rowptr, col, ordering, P);
    if (st != OPMGPU_OK) return st;
    for (int i = 0; i < nb; ++i) { if (position) position[i] = P.pos[i]; if (level) level[i] = P.level[P.pos[i]]; }
    if (nlevels) *nlevels = P.nlevels;
    return OPMGPU_OK;
}

} // extern "C"
