// solve.inl -- the driver of one linear solve and the schedule of its ILU0 factorisation; part of linsolver.hip.

// The model's call at the end of an assembly (linsolver.hpp, factor_early_on): the conditions under which the solve would factorise on the side
// stream anyway, on a matrix nobody changes any more (the host well model adds its blocks later) and with the plain ILU0
void LinSolver::factor_ahead(const opmgpu_params& prm, bool host_wells, const std::function<void()>& matrix_final)
{
    ahead = AHEAD_NONE;
    if (!(factor_early_on && factor_overlap && prm.use_cpr && !prm.cpr_reference_transform && emulate_ranks <= 1 && !host_wells && prm.cpr_ilu_n == 0 && fill_level == 0)) return;
    wb_relax = cpr_stage2_relaxation(prm);
    matrix_final();
    if (matrix_is_float) { ensure_work<float>(); factor_async<float>(); ahead = AHEAD_FLOAT; }
    else if (prm.preconditioner_single) { mixed_prepare(true); factor_async<float>(); ahead = AHEAD_FLOAT; }      // mixed precision: the float copy, then its factors
    else { ensure_work<double>(); factor_async<double>(); ahead = AHEAD_DOUBLE; }
}

template <class S> int LinSolver::solve(const opmgpu_params& params, bool matrix_changed, SolveResult& res, std::string& err)
{
    auto refuse = [&](const char* msg) { err = msg; return int(OPMGPU_EINVAL); };
    // the solvers below read ONE relaxation field: under CPR it holds the second stage's (cpr_stage2_relaxation)
    opmgpu_params prm = params;
    if (prm.use_cpr) {
        if (prm.cpr_ilu_n > 0 && prm.cpr_reference_transform == 2) return refuse("cpr_ilu_n > 0 with cpr_reference_transform = 2: the point ILU of the scalar system is an ILU0");
        if (!(prm.cpr_relax > 0.0) || !(prm.cpr_solver_tol > 0.0) || prm.cpr_max_ell_iter < 0) return refuse("cpr_relax / cpr_solver_tol must be positive, cpr_max_ell_iter >= 0");
        if (!(prm.cpr_stage2_relax > 0.0)) return refuse("cpr_stage2_relax must be positive");
        prm.ilu_relaxation = cpr_stage2_relaxation(prm);
        // the elliptic part (elliptic.inl): cpr_max_ell_iter = 0 is this library's one-V-cycle stage, which needs the AMG
        if (prm.cpr_max_ell_iter == 0 && !prm.cpr_use_amg) return refuse("cpr_max_ell_iter = 0 (one application, no inner Krylov method) needs cpr_use_amg = 1");
        ell.inner = prm.cpr_max_ell_iter > 0; ell.use_amg = prm.cpr_use_amg != 0; ell.bicgstab = prm.cpr_use_bicgstab != 0;
        ell.tol = prm.cpr_solver_tol; ell.maxit = prm.cpr_max_ell_iter; ell.relax = prm.cpr_relax;
    }
    wb_relax = prm.ilu_relaxation;
    const int fill = fill_level_of(prm);
    if (fill < 0) return refuse(kFillLevelRange);
    if (fill != fill_level) { join_factor(); ahead = AHEAD_NONE; fill_level = fill; }        // (an early factorisation of the other kind is void)
    if (prm.use_cpr) correction_policy_choose();
    // mixed precision (preconditioner_single): a double solve with its preconditioner in the float work set; not with the in-place transform
    const bool mixed = prm.preconditioner_single && sizeof(S) == 8 && !(prm.use_cpr && prm.cpr_reference_transform) && emulate_ranks <= 1;
    now.mixed = mixed;
    prepare<S>(matrix_changed);
    if (mixed) mixed_prepare(matrix_changed);
    // the reference's CPR formulation (whole-system L transform, 200-bar pressure row, ||L r|| stopping) as an option; once per matrix
    if (prm.use_cpr && prm.cpr_reference_transform) cpr_reference_transform<S>();
    else { now.border_weights = nullptr; now.border_colscale = 1.0; }
    // cpr_reference_transform = 2: the reference's own second stage, a point ILU0 of the transformed system as a scalar equation-major matrix
    now.point_stage2 = prm.use_cpr && prm.cpr_reference_transform == 2;
    if (now.point_stage2) {
        if (sizeof(S) != 8) return refuse("cpr_reference_transform = 2 (point ILU0 of the scalar system) is double only, like the reference's CPR plug-in");
        if (comm || emulate_ranks > 1) return refuse("cpr_reference_transform = 2 is a single-GPU comparison mode");
        if (pilu.stale) { point_ilu_factor(); pilu.stale = false; }
    }
    // The block factorisation.  Under CPR it runs on its side stream, started next to the pressure stage's set-up (cpr_prepare, inside the
    // solver: behind the level 0 -> 1 Galerkin sums); not in the emulated-decomposition diagnostics, whose cut copy of the matrix is built
    // lazily by whichever of the two asks first
    const bool early = ahead == (mixed || std::is_same<S, float>::value ? AHEAD_FLOAT : AHEAD_DOUBLE) && matrix_changed && !prm.cpr_reference_transform;      // factor_ahead() started it behind the assembly
    ahead = AHEAD_NONE;
    if (now.point_stage2) { /* the point ILU0 above is the second stage: no block factorisation */ }
    else if (early) { /* running on the factor stream already; the first ILU0 sweep joins it */ }
    else if (factor_overlap && prm.use_cpr && emulate_ranks <= 1) now.factor_deferred = true;
    else if (mixed) (void)factor<float>(false);
    else (void)factor<S>(false);      // status read below: the solver's own final synchronisation covers it
    auto krylov = [&] { return prm.newton_use_gmres ? gmres<S>(prm) : bicgstab<S>(prm); };
    res = krylov();
    if (prm.use_cpr) correction_policy_report(res.iterations, res.status == OPMGPU_OK);
    if (res.status != OPMGPU_OK && prm.use_cpr && corr_policy.active && corr_policy.cur > 0 && factor_status() == OPMGPU_OK) {
        // the solve ran with a scaled coarse-grid correction: once more with the plain Galerkin correction (factor 1.0, the safe end of the policy's
        // ladder) before anything is reported -- a failed linear solve costs the caller a chopped time step.  The rest of the step stays on it;
        // the failure counts against the factor at once and bans it and every larger one for a while (LinSolver::CorrectionPolicy)
        corr_policy.fail_at_current(res.iterations);
        if (mixed) work<float>().amg->pdamp0 = work<float>().amg->pdamp = corr_policy.arm[0];
        else work<S>().amg->pdamp0 = work<S>().amg->pdamp = corr_policy.arm[0];
        res = krylov();
        correction_policy_report(res.iterations, res.status == OPMGPU_OK);
    }
    if (res.status != OPMGPU_OK && prm.use_cpr && !refreshed && factor_status() == OPMGPU_OK) {
        // the solve ran on lagged coarse operators of the pressure hierarchy (cpr_prepare): once more on fresh ones
        force_refresh = true; lag_block = 8;
        res = krylov();
    }
    if (!now.point_stage2 && factor_status() != OPMGPU_OK) { err = "singular diagonal block in ILU0"; return OPMGPU_ESINGULAR; }
    if (res.status == OPMGPU_ELINSOLVE) err = "Convergence failure for linear solver.";
    if (res.status == OPMGPU_EBREAKDOWN) err = breakdown_note.empty() ? std::string("breakdown in the Krylov method") : breakdown_note;
    return res.status;
}
