// krylov.inl -- the Krylov methods around the preconditioner (included by linsolver.hip): BiCGStab and restarted GMRES with their
// kernels and the device-resident control block every kernel of an iteration checks.

// copy the status fields to the host-mapped block (one thread; only when the solve stops / at the final check)
__device__ __forceinline__ void publish(const SolveCtl* ctl, SolveCtl* hst)
{
    hst->norm0_2 = ctl->norm0_2; hst->norm2 = ctl->norm2; hst->flag = ctl->flag; hst->iters = ctl->iters; hst->decided = ctl->decided;
    __threadfence_system();
    hst->done = ctl->done;
}

// ---- BiCGStab (Dune::BiCGSTABSolver::apply) ------------------------------------------------
// iteration j = 1, 2, ...:
//   k_update_p (j)  : [test ||r||^2 of iteration j-1]  rho_new = <rt,r>; beta; p = r + beta (p - omega v)
//   ILU, k_spmv<1>  : y = M^-1 p ; v = A y ; partials h = <rt,v>
//   k_update_xr1(j) : alpha = rho_new / h ; x += alpha y ; r -= alpha v ; partials ||r||^2
//   ILU, k_spmv<2>  : y = M^-1 r ; t = A y ; partials <t,r>, <t,t>
//   k_update_xr2(j) : [test ||r||^2 of the first half step]  omega ; x += omega y ; r -= omega t ; partials ||r||^2, <rt,r>
// Every workgroup derives the scalars from the partial arrays itself; workgroup 0 records them.
// Restricted residuals of the subdomain coarse space carried along the BiCGStab recurrences (LinSolver::cs_recur): C(x)[q] = sum over
// the rows of coarse unknown q of (CPR weights . x) is linear in x, so with the GLOBAL C(v), C(t) of the two products of an iteration
//   C(r) -= alpha C(v) ; C(r) -= omega C(t) ; C(p) = C(r) + beta (C(p) - omega C(v))
// hold exactly what restricting r and p would give.  Workgroup 0 of the vector kernels advances them (ns <= 64 <= kBlock).
struct CsRec { double* Cp; double* Cr; const double* Cv; const double* Ct; const double* C0; int ns; };

template <class S>
__global__ __launch_bounds__(kBlock) void k_update_p(long n, int j, double eps, SolveCtl* __restrict__ ctl, SolveCtl* __restrict__ hst, const double* __restrict__ p_n2,
                                                     const double* __restrict__ p_rho, int np, const S* __restrict__ r,
                                                     const S* __restrict__ v, S* __restrict__ p, CsRec cs)
{
    __shared__ double sm[12];
    if (ctl->done) return;
    const double* const arr[2] = { p_n2, p_rho };
    double s[2];
    reduce_partials<2>(arr, np, s, sm);
    const double norm2 = s[0], rho_new = s[1];
    const bool first = (j == 1);
    if (first) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->norm0_2 = norm2; ctl->norm2 = norm2; ctl->rho[1] = rho_new; }
        if (!(norm2 == norm2)) { if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->flag = 2; ctl->decided = j; ctl->done = 1; publish(ctl, hst); } return; }
        if (norm2 < 1e-60) { if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->iters = 0; ctl->decided = j; ctl->done = 1; publish(ctl, hst); } return; }
        if (blockIdx.x == 0 && int(threadIdx.x) < cs.ns) { const double c = cs.C0[threadIdx.x]; cs.Cr[threadIdx.x] = c; cs.Cp[threadIdx.x] = c; }
        for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) p[i] = r[i];
        return;
    }
    // convergence test after the second half of iteration j-1:  norm < reduction * norm0  ||  norm < 1e-30
    if (norm2 < ctl->thresh2 || norm2 < 1e-60) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->norm2 = norm2; ctl->iters = j - 1; ctl->decided = j; ctl->done = 1; publish(ctl, hst); }
        return;
    }
    const double rho_old = ctl->rho[(j - 1) & 1], omega = ctl->omega, alpha = ctl->alpha;
    if (fabs(rho_old) <= eps || fabs(omega) <= eps || !(rho_old == rho_old) || !(omega == omega) || !(norm2 == norm2)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->norm2 = norm2; ctl->flag = 2; ctl->iters = j - 1; ctl->decided = j; ctl->done = 1; publish(ctl, hst); }
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->rho[j & 1] = rho_new; ctl->norm2 = norm2; }
    const double beta_d = (rho_new / rho_old) * (alpha / omega);
    const S beta = S(beta_d), om = S(omega);
    if (blockIdx.x == 0 && int(threadIdx.x) < cs.ns) cs.Cp[threadIdx.x] = cs.Cr[threadIdx.x] + beta_d * (cs.Cp[threadIdx.x] - omega * cs.Cv[threadIdx.x]);
    constexpr int L = 16 / sizeof(S);              // 16-byte lanes (n is a multiple of 192)
    struct alignas(16) Pack { S v[L]; };
    const long nv = n / L;
    for (long q = blockIdx.x * long(kBlock) + threadIdx.x; q < nv; q += long(gridDim.x) * kBlock) {
        Pack pp = reinterpret_cast<Pack*>(p)[q];
        const Pack vv = reinterpret_cast<const Pack*>(v)[q], rr = reinterpret_cast<const Pack*>(r)[q];
#pragma unroll
        for (int u = 0; u < L; ++u) pp.v[u] = (pp.v[u] - om * vv.v[u]) * beta + rr.v[u];
        reinterpret_cast<Pack*>(p)[q] = pp;
    }
    for (long i = nv * L + blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) p[i] = (p[i] - om * v[i]) * beta + r[i];
}

template <class S>
__global__ __launch_bounds__(kBlock) void k_update_xr1(long n, int j, double eps, SolveCtl* __restrict__ ctl, SolveCtl* __restrict__ hst, const double* __restrict__ p_h, int np,
                                                       const S* __restrict__ y, const S* __restrict__ q, S* __restrict__ x, S* __restrict__ r,
                                                       double* __restrict__ p_n1, CsRec cs)
{
    __shared__ double sm[12];
    if (ctl->done) return;
    const double* const arr[1] = { p_h };
    double s[1];
    reduce_partials<1>(arr, np, s, sm);
    const double h = s[0];
    if (fabs(h) < eps || !(h == h)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->flag = 1; ctl->iters = j; ctl->decided = j; ctl->done = 1; publish(ctl, hst); }
        return;
    }
    const double alpha = ctl->rho[j & 1] / h;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->alpha = alpha;
    if (blockIdx.x == 0 && int(threadIdx.x) < cs.ns) cs.Cr[threadIdx.x] -= alpha * cs.Cv[threadIdx.x];
    const S a = S(alpha);
    double acc[1] = { 0.0 };
    constexpr int L = 16 / sizeof(S);
    struct alignas(16) Pack { S v[L]; };
    const long nv = n / L;
    for (long k = blockIdx.x * long(kBlock) + threadIdx.x; k < nv; k += long(gridDim.x) * kBlock) {
        Pack xx = reinterpret_cast<Pack*>(x)[k], rr = reinterpret_cast<Pack*>(r)[k];
        const Pack yy = reinterpret_cast<const Pack*>(y)[k], qq = reinterpret_cast<const Pack*>(q)[k];
#pragma unroll
        for (int u = 0; u < L; ++u) { xx.v[u] += a * yy.v[u]; rr.v[u] = rr.v[u] - a * qq.v[u]; acc[0] += double(rr.v[u]) * double(rr.v[u]); }
        reinterpret_cast<Pack*>(x)[k] = xx; reinterpret_cast<Pack*>(r)[k] = rr;
    }
    for (long i = nv * L + blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) {
        x[i] += a * y[i];
        const S rn = r[i] - a * q[i];
        r[i] = rn;
        acc[0] += double(rn) * double(rn);
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) p_n1[blockIdx.x] = acc[0];
}

template <class S>
__global__ __launch_bounds__(kBlock) void k_update_xr2(long n, int j, SolveCtl* __restrict__ ctl, SolveCtl* __restrict__ hst, const double* __restrict__ p_n1,
                                                       const double* __restrict__ p_tr, const double* __restrict__ p_tt, int np_v, int np_s,
                                                       const S* __restrict__ y, const S* __restrict__ q, const S* __restrict__ rt,
                                                       S* __restrict__ x, S* __restrict__ r, double* __restrict__ p_n2, double* __restrict__ p_rho, CsRec cs)
{
    __shared__ double sm[12];
    if (ctl->done) return;
    double s1[1], s2[2];
    { const double* const arr[1] = { p_n1 }; reduce_partials<1>(arr, np_v, s1, sm); }
    if (s1[0] < ctl->thresh2) {          // converged after the first half step of iteration j: x is final
        if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->norm2 = s1[0]; ctl->iters = j; ctl->decided = j; ctl->done = 1; publish(ctl, hst); }
        return;
    }
    { const double* const arr[2] = { p_tr, p_tt }; reduce_partials<2>(arr, np_s, s2, sm); }
    const double omega = s2[0] / s2[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->omega = omega;
    if (blockIdx.x == 0 && int(threadIdx.x) < cs.ns) cs.Cr[threadIdx.x] -= omega * cs.Ct[threadIdx.x];
    const S a = S(omega);
    double acc[2] = { 0.0, 0.0 };
    constexpr int L = 16 / sizeof(S);
    struct alignas(16) Pack { S v[L]; };
    const long nv = n / L;
    for (long k = blockIdx.x * long(kBlock) + threadIdx.x; k < nv; k += long(gridDim.x) * kBlock) {
        Pack xx = reinterpret_cast<Pack*>(x)[k], rr = reinterpret_cast<Pack*>(r)[k];
        const Pack yy = reinterpret_cast<const Pack*>(y)[k], qq = reinterpret_cast<const Pack*>(q)[k], tt = reinterpret_cast<const Pack*>(rt)[k];
#pragma unroll
        for (int u = 0; u < L; ++u) {
            xx.v[u] += a * yy.v[u]; rr.v[u] = rr.v[u] - a * qq.v[u];
            acc[0] += double(rr.v[u]) * double(rr.v[u]); acc[1] += double(tt.v[u]) * double(rr.v[u]);
        }
        reinterpret_cast<Pack*>(x)[k] = xx; reinterpret_cast<Pack*>(r)[k] = rr;
    }
    for (long i = nv * L + blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) {
        x[i] += a * y[i];
        const S rn = r[i] - a * q[i];
        r[i] = rn;
        acc[0] += double(rn) * double(rn);
        acc[1] += double(rt[i]) * double(rn);
    }
    block_sum<2>(acc, sm);
    if (threadIdx.x == 0) { p_n2[blockIdx.x] = acc[0]; p_rho[blockIdx.x] = acc[1]; }
}

// convergence test after the last enqueued iteration (what k_update_p(j+1) would have done)
// tick (optional): a host-mapped word the host spins on instead of synchronising the stream -- written last, after a system fence
__global__ __launch_bounds__(kBlock) void k_final_check(int j, SolveCtl* __restrict__ ctl, SolveCtl* __restrict__ hst, const double* __restrict__ p_n2, int np,
                                                        int* __restrict__ tick_ptr = nullptr, int tick = 0)
{
    __shared__ double sm[12];
    if (ctl->done) { if (threadIdx.x == 0) { publish(ctl, hst); if (tick_ptr) { __threadfence_system(); *(volatile int*)tick_ptr = tick; } } return; }
    const double* const arr[1] = { p_n2 };
    double s[1];
    reduce_partials<1>(arr, np, s, sm);
    if (threadIdx.x == 0) {
        ctl->norm2 = s[0];
        ctl->iters = j;
        if (s[0] < ctl->thresh2 || s[0] < 1e-60) ctl->done = 1;
        publish(ctl, hst);
        if (tick_ptr) { __threadfence_system(); *(volatile int*)tick_ptr = tick; }
    }
}
// one workgroup.  zbuf (optional): nz doubles cleared in the same launch -- GMRES' Hessenberg block, instead of a fill of its own
__global__ __launch_bounds__(kBlock) void k_ctl_init(SolveCtl* ctl, SolveCtl* hst, double red, double* __restrict__ zbuf = nullptr, int nz = 0)
{
    for (int i = threadIdx.x; i < nz; i += kBlock) zbuf[i] = 0.0;
    if (threadIdx.x != 0) return;
    hst->done = 0; hst->flag = 0; hst->iters = 0; hst->decided = 0; hst->norm2 = 0.0; hst->norm0_2 = 0.0;
    ctl->rho[0] = 1.0; ctl->rho[1] = 1.0; ctl->alpha = 1.0; ctl->omega = 1.0;
    ctl->norm0_2 = 0.0; ctl->norm2 = 0.0; ctl->thresh2 = 0.0; ctl->done = 0; ctl->flag = 0; ctl->iters = 0; ctl->decided = 0;
    (void)red;
}
// thresh2 = (reduction * ||r0||)^2 needs ||r0||^2: one workgroup, right after the initial dot
__global__ __launch_bounds__(kBlock) void k_ctl_thresh(SolveCtl* __restrict__ ctl, double red, const double* __restrict__ p_n2, int np)
{
    __shared__ double sm[12];
    const double* const arr[1] = { p_n2 };
    double s[1];
    reduce_partials<1>(arr, np, s, sm);
    if (threadIdx.x == 0) { ctl->norm0_2 = s[0]; ctl->norm2 = s[0]; ctl->thresh2 = red * red * s[0]; }
}
// multi-GPU bridge: collapse partial arrays to their sums (fixed order) so they can be all-reduced
template <int NV>
__global__ __launch_bounds__(kBlock) void k_sum_partials(const double* __restrict__ a0, const double* __restrict__ a1, int np, double* __restrict__ out)
{
    __shared__ double sm[12];
    const double* const arr[2] = { a0, a1 ? a1 : a0 };
    double s[2];
    reduce_partials<2>(arr, np, s, sm);
    if (threadIdx.x == 0) { out[0] = s[0]; if (NV == 2) out[1] = s[1]; }
}

// this rank's block sums of (CPR weights . d): parts[u * gridDim.x + workgroup] for its coarse unknowns u < m (blk: block of a row,
// -1 = not owned; without blocks the owner mask decides and m = 1)
template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_wdot(int nb, int nbp, const S* __restrict__ d, const S* __restrict__ w, const int8_t* __restrict__ owned,
                                                    const int8_t* __restrict__ blk, int m, double* __restrict__ parts, const SolveCtl* __restrict__ ctl)
{
    __shared__ double sm[32];
    if (ctl && ctl->done) return;
    double acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < nb; i += long(gridDim.x) * kBlock) {
        const int b = blk ? int(blk[i]) : ((!owned || owned[i]) ? 0 : -1);
        if (b < 0) continue;
        const S bs = w[i] * d[i] + w[nbp + i] * d[nbp + i] + w[2 * long(nbp) + i] * d[2 * long(nbp) + i];      // as k_cpr_sum_eqs forms it
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] += (u == b) ? double(bs) : 0.0;
    }
    block_sum<8>(acc, sm);
    if (threadIdx.x == 0) for (int u = 0; u < m; ++u) parts[long(u) * gridDim.x + blockIdx.x] = acc[u];
}
// bridge with the coarse-space sums: out[0..NV) as k_sum_partials, out[NV + q] = this rank's sum for coarse unknown q (its own slots
// mine*m .. mine*m + m - 1), zero for the others' -- the all-reduce that follows then delivers every rank's
template <int NV>
__global__ __launch_bounds__(kBlock) void k_bridge_cs(const double* __restrict__ a0, const double* __restrict__ a1, int np, const double* __restrict__ cparts, int ncp,
                                                      int ns, int m, int mine, double* __restrict__ out)
{
    __shared__ double sm[12];
    __shared__ double tot[8];
    const double* const arr[2] = { a0, a1 ? a1 : a0 };
    double s[2];
    reduce_partials<2>(arr, np, s, sm);
    if (threadIdx.x == 0) { out[0] = s[0]; if (NV == 2) out[1] = s[1]; }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int b = 0; b < m; ++b) {
        double v = 0.0;
        for (int i = threadIdx.x; i < ncp; i += kBlock) v += cparts[long(b) * ncp + i];
        const double sw = wave_sum(v);
        __syncthreads();
        if (lane == 0) sm[wv] = sw;
        __syncthreads();
        if (threadIdx.x == 0) tot[b] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    }
    __syncthreads();
    if (int(threadIdx.x) < ns) { const int b = int(threadIdx.x) - mine * m; out[NV + threadIdx.x] = (b >= 0 && b < m) ? tot[b] : 0.0; }
}

template <class S> SolveResult LinSolver::bicgstab(const opmgpu_params& prm)
{
    SolverWork<S>& w = work<S>();
    SolveResult res;
    wb_active = false;             // (the wells' Woodbury correction of stage 2 runs under GMRES only: the closed-form rows below assume the plain ILU0)
    const long n = long(3) * plan.nbp;
    const int gv = std::min(grid_for(n), kMaxPart);            // vector kernels (also the number of their partials)
    const int gs = std::min(grid8_for(plan.nb), kMaxPart);     // reducing SpMV launches (multiple of 8: XCD-aware chunking)
    const double eps = sizeof(S) == 8 ? 1e-80 : 0.0;           // dune: real_type EPSILON = 1e-80 (0 in float)
    const int maxit = prm.linear_solver_maxiter;
    const int8_t* mask = comm ? comm->owner_mask() : nullptr;
    // closed form of (A M^-1 p) on the level-0 rows -- valid when M is the ILU0 of exactly this matrix and none of the row's
    // neighbours is a ghost whose entry of M^-1 p is overwritten by the halo exchange (multi-GPU: light_ok masks those rows out)
    const bool cpr = prm.use_cpr != 0;                   // multi-GPU: rank-local (additive Schwarz) AMG + block-Jacobi ILU0
    lag_allowed = prm.linear_solver_reduction >= 1e-4;
    const bool mx = now.mixed && sizeof(S) == 8;
    if (cpr) { if (mx) cpr_prepare_mixed(); else cpr_prepare<S>(); }
    if (now.factor_deferred) { now.factor_deferred = false; if (mx) factor_async<float>(); else factor_async<S>(); }
    if (cpr) { if (mx) { if (!wf.amg->npost0_user) wf.amg->npost0 = 2; } else if (!w.amg->npost0_user) w.amg->npost0 = 2; }   // post-sweeps on level 0: 2 under BiCGStab, 1 under GMRES (see gmres)
    solution_mirror = nullptr; mirror_written = false;          // (the mirror is GMRES': this solver's caller copies x)
    cancel_p_now = false;
    if (cpr) { if (mx) wf.amg->lane_restrict = lean_conditions(); else w.amg->lane_restrict = lean_conditions(); }      // the V-cycle's restriction: shared with gmres()
    // (with cpr_relax != 1 the pressure part of M^-1 p is scaled, which the closed form does not cover)
    // (mixed precision: the float ILU0 is not the ILU0 of exactly the double matrix -- the closed form would be off by float rounding)
    const bool closed = closed_form_level0 && emulate_ranks <= 1 && !(cpr && ell.relax != 1.0) && !mx && !(cpr && now.point_stage2) && fill_level == 0;      // (ell.relax = cpr_relax; under CPR prm.ilu_relaxation holds cpr_relax * cpr_stage2_relax: solve())
    const int8_t* lightmask = nullptr;
    const bool overlap = comm && halo_overlap;
    if (comm && (closed || overlap)) {
        if (light_ok_for != comm || light_ok.n != size_t(plan.nbp)) {
            light_ok.alloc(plan.nbp); light_ok.zero(stream);
            hipLaunchKernelGGL(k_light_mask, dim3(grid_for(plan.nb)), dim3(kBlock), 0, stream, plan.nb, dp.slice_ptr.p, dp.col.p, dp.rowlen.p, comm->owner_mask(), light_ok.p);
            light_ok_for = comm;
        }
        if (closed) lightmask = light_ok.p;
    }
    if (overlap && !halo_stream) {
        OPMGPU_HIP(hipStreamCreateWithFlags(&halo_stream, hipStreamNonBlocking));
        for (auto& e : ev_halo) OPMGPU_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const S* pin_p = closed ? w.p.p : nullptr; const S* pin_r = closed ? w.r.p : nullptr;
    const S* zin_p = cpr ? w.z.p : pin_p; const S* zin_r = cpr ? w.z.p : pin_r;     // second-stage input of the last M^-1
    const int n0 = plan.level_ptr[1];
    // v = A y with the halo exchange of y behind the rows that do not need it; returns the number of partials written
    auto spmv_halo = [&](auto which, S* yv, S* out, const S* w1, double* q0, double* q1, const S* pin, const S* zin) -> int {
        constexpr int ND = decltype(which)::value;
        auto launch = [&](int phase) {       // phase 2 (the cut-adjacent rows) lays its partials behind phase 1's
            const int off = phase == 2 ? gs : 0;
            if (phase != 2) lowrank_reduce<S>(yv, (const SolveCtl*)ctl.p);       // wells live on one rank: their perforated cells are owned rows
            hipLaunchKernelGGL((k_spmv<S, ND>), dim3(phase == 2 ? kBndPart : gs), dim3(kBlock), 0, stream, xcd_mode(), plan.nb, plan.nbp, dp.slice_ptr.p, dp.col.p, matrix<S>(),
                               yv, out, w1, mask, (const SolveCtl*)ctl.p, q0 + off, q1 ? q1 + off : (double*)nullptr, pin, zin, n0, S(prm.ilu_relaxation), lowrank, lightmask, phase,
                               phase ? (const int8_t*)light_ok.p : (const int8_t*)nullptr);
        };
        if (overlap) { halo_overlapped(*this, yv, launch); return gs + kBndPart; }
        if (comm) halo(comm, yv, stream);
        launch(0);
        return gs;
    };
    double* P_h = partials.p, *P_n1 = P_h + npart, *P_tr = P_n1 + npart, *P_tt = P_tr + npart, *P_n2 = P_tt + npart, *P_rho = P_n2 + npart;
    double* red = P_rho + npart;                               // 8 all-reduced scalars (multi-GPU)
    // (multi-GPU) collapse partial arrays of np entries into red[slot..] and all-reduce them; consumers then read 1 entry
    // defer > 0: no all-reduce now, the NEXT bridge (whose slots follow this one's) reduces `defer` more values in the same call
    int deferred = 0;
    // coarse-space restriction by recurrence (see CsRec): active for the real multi-rank coarse space only
    // The recurrences run in double next to vectors of precision S: every x -= a y of the vectors leaves a rounding error of eps_S |r_k| in
    // the REAL restricted residual that the recurrence does not see, so once ||r|| has dropped by about sqrt(eps_S) the carried value is
    // noise and the correction it drives stalls the iteration (seen: float solve asked for 1e-10).  The host reads ||r||^2 after every
    // CPR iteration anyway (wait_tick): below cs_floor the applications go back to restricting and all-reducing themselves.
    const bool cs_rec = cpr && comm && cs_recur && !cpr_speculate && coarse_nsub >= 1 && coarse_nsub <= 64;
    const double cs_floor = sizeof(S) == 4 ? 1e-3 : 1e-11;
    bool cs_live = cs_rec;
    const int ns = cs_rec ? coarse_nsub : 0;
    // position of all-reduce slot s in `red`: the coarse-space vectors follow slot 0 (initial C(r)), slot 1 (C(v)) and slot 4 (C(t))
    auto pos = [&](int slot) { return slot + (slot >= 1 ? ns : 0) + (slot >= 2 ? ns : 0) + (slot >= 5 ? ns : 0); };
    CsRec csr = { nullptr, nullptr, nullptr, nullptr, nullptr, 0 };
    double* cs_wparts = nullptr; int cs_gp = 0;
    if (cs_rec) {
        if (cs_state.n < size_t(2) * ns) cs_state.alloc(size_t(2) * ns);
        csr.Cp = cs_state.p; csr.Cr = cs_state.p + ns; csr.ns = ns;
        csr.C0 = red + pos(0) + 1; csr.Cv = red + pos(1) + 1; csr.Ct = red + pos(4) + 1;
        cs_wparts = cs_buf.p + size_t(2) * ns * ns + ns;       // the scratch of cpr_apply's fused restriction: free between applications
        cs_gp = std::min(grid_for(plan.nb), kMaxPart);
    }
    // cs_vec (cs_rec only): the vector whose restriction is appended behind the scalars of this bridge
    auto bridge = [&](double*& a0, double*& a1, int& np, int slot, bool defer = false, const S* cs_vec = nullptr) {
        if (!comm) return;
        double* out = red + pos(slot);
        const int nv = a1 ? 2 : 1;
        int extra = 0;
        if (cs_live && cs_vec) {
            hipLaunchKernelGGL((k_cs_wdot<S>), dim3(cs_gp), dim3(kBlock), 0, stream, plan.nb, plan.nbp, cs_vec, (const S*)w.cprw.p, cs_m > 1 ? (const int8_t*)nullptr : mask,
                               cs_m > 1 ? (const int8_t*)cs_blk.p : (const int8_t*)nullptr, cs_m, cs_wparts, (const SolveCtl*)nullptr);
            if (a1) hipLaunchKernelGGL((k_bridge_cs<2>), dim3(1), dim3(kBlock), 0, stream, a0, a1, np, (const double*)cs_wparts, cs_gp, ns, cs_m, comm->my_rank(), out);
            else hipLaunchKernelGGL((k_bridge_cs<1>), dim3(1), dim3(kBlock), 0, stream, a0, (const double*)nullptr, np, (const double*)cs_wparts, cs_gp, ns, cs_m, comm->my_rank(), out);
            extra = ns;
        } else if (a1) hipLaunchKernelGGL((k_sum_partials<2>), dim3(1), dim3(kBlock), 0, stream, a0, a1, np, out);
        else hipLaunchKernelGGL((k_sum_partials<1>), dim3(1), dim3(kBlock), 0, stream, a0, (const double*)nullptr, np, out);
        if (defer) deferred += nv;
        else { comm->allreduce_sum(out - deferred, nv + deferred + extra, stream); deferred = 0; }
        a0 = out; if (a1) a1 = out + 1; np = 1;
    };
    // x = 0, r = rt = b, p = v = 0
    w.x.zero(stream);
    OPMGPU_HIP(hipMemcpyAsync(w.r.p, w.b.p, n * sizeof(S), hipMemcpyDeviceToDevice, stream));
    OPMGPU_HIP(hipMemcpyAsync(w.rt.p, w.b.p, n * sizeof(S), hipMemcpyDeviceToDevice, stream));
    SolveCtl* d_ctl = ctl.p;
    hipLaunchKernelGGL(k_ctl_init, dim3(1), dim3(1), 0, stream, d_ctl, h_ctl_dev, prm.linear_solver_reduction);
    hipLaunchKernelGGL((k_dot<S>), dim3(gv), dim3(kBlock), 0, stream, n, w.r.p, w.r.p, P_n2);
    double* a_n2 = P_n2; double* a_rho = P_n2; double* none = nullptr; int np_n2 = gv;
    bridge(a_n2, none, np_n2, 0, false, w.r.p); a_rho = a_n2;
    hipLaunchKernelGGL(k_ctl_thresh, dim3(1), dim3(kBlock), 0, stream, d_ctl, prm.linear_solver_reduction, (const double*)a_n2, np_n2);
    int j = 1, last = 0, target = 0;
    bool stop = false, checked = false;      // checked: the last enqueued iteration has been tested and the status block is current
    for (; j <= maxit && !stop; ++j) {
        checked = false;
        hipEvent_t kt_a = kt.begin();
        const CsRec csr_off = { nullptr, nullptr, nullptr, nullptr, nullptr, 0 };
        const CsRec csr_it = cs_live ? csr : csr_off;
        hipLaunchKernelGGL((k_update_p<S>), dim3(gv), dim3(kBlock), 0, stream, n, j, eps, d_ctl, h_ctl_dev, (const double*)a_n2, (const double*)a_rho, np_n2,
                           w.r.p, w.v.p, w.p.p, csr_it);
        kt.end(KT_VECTOR, kt_a);
        precond_apply<S>(w.p.p, w.y.p, prm.ilu_relaxation, d_ctl, cpr, csr_it.Cp);
        kt_a = kt.begin();
        const int np_spmv1 = spmv_halo(std::integral_constant<int, 1>(), w.y.p, w.v.p, w.rt.p, P_h, (double*)nullptr, pin_p, zin_p);
        kt.end(KT_SPMV1, kt_a);
        double* a_h = P_h; int np_h = np_spmv1; none = nullptr;
        bridge(a_h, none, np_h, 1, false, w.v.p);
        kt_a = kt.begin();
        hipLaunchKernelGGL((k_update_xr1<S>), dim3(gv), dim3(kBlock), 0, stream, n, j, eps, d_ctl, h_ctl_dev, (const double*)a_h, np_h, w.y.p, w.v.p,
                           w.x.p, w.r.p, P_n1, csr_it);
        kt.end(KT_VECTOR, kt_a);
        double* a_n1 = P_n1; int np_n1 = gv; none = nullptr;
        bridge(a_n1, none, np_n1, 2, true);      // ||r||^2 of the half step is consumed by k_update_xr2: reduced together with <t,r>, <t,t> (slots 2..4)
        precond_apply<S>(w.r.p, w.y.p, prm.ilu_relaxation, d_ctl, cpr, csr_it.Cr);
        kt_a = kt.begin();
        const int np_spmv2 = spmv_halo(std::integral_constant<int, 2>(), w.y.p, w.t.p, w.r.p, P_tr, P_tt, pin_r, zin_r);
        kt.end(KT_SPMV2, kt_a);
        double* a_tr = P_tr; double* a_tt = P_tt; int np_t = np_spmv2;
        bridge(a_tr, a_tt, np_t, 3, false, w.t.p);
        kt_a = kt.begin();
        hipLaunchKernelGGL((k_update_xr2<S>), dim3(gv), dim3(kBlock), 0, stream, n, j, d_ctl, h_ctl_dev, (const double*)a_n1, (const double*)a_tr,
                           (const double*)a_tt, np_n1, np_t, w.y.p, w.t.p, w.rt.p, w.x.p, w.r.p, P_n2, P_rho, csr_it);
        kt.end(KT_VECTOR, kt_a);
        a_n2 = P_n2; a_rho = P_rho; np_n2 = gv;
        bridge(a_n2, a_rho, np_n2, 5);
        last = j;
        if (cpr && !cpr_speculate) {
            // CPR iterations are long (~0.6 ms of kernels) and few (~5): a speculative extra iteration of ~50 no-op
            // launches costs more than one host round trip, so test convergence at the END of the iteration and wait.
            const int tick = ++tick_seq;
            hipLaunchKernelGGL(k_final_check, dim3(1), dim3(kBlock), 0, stream, j, d_ctl, h_ctl_dev, (const double*)a_n2, np_n2, poll_status ? h_tick_dev : (int*)nullptr, tick);
            wait_tick(tick);
            if (h_ctl->done) stop = true;
            if (cs_live && !(h_ctl->norm2 > cs_floor * cs_floor * h_ctl->norm0_2)) cs_live = false;      // the same decision on every rank: the norms are collective
            checked = true;
            continue;
        }
        OPMGPU_HIP(hipEventRecord(ev[j & 1], stream));
        if (j >= 2 && target == 0) {       // iteration j-1 is complete once its event has fired; iteration j is already queued
            OPMGPU_HIP(hipEventSynchronize(ev[(j - 1) & 1]));
            if (h_ctl->done) {
                // single GPU: stop now.  Multi GPU: every rank must enqueue the SAME number of iterations (their
                // collectives pair up); `decided` is identical on all ranks, when a rank notices it is not.
                if (!comm) stop = true;
                else target = std::min(maxit, h_ctl->decided + 1);
            }
        }
        if (target != 0 && j >= target) stop = true;
    }
    if (!checked) {
        hipLaunchKernelGGL(k_final_check, dim3(1), dim3(kBlock), 0, stream, last, d_ctl, h_ctl_dev, (const double*)a_n2, np_n2);
        OPMGPU_HIP(hipStreamSynchronize(stream));
    }
    if (comm) comm->check_async();          // a collective that failed asynchronously must not pass as a converged solve
    const double norm0 = std::sqrt(h_ctl->norm0_2), norm = std::sqrt(h_ctl->norm2);
    res.converged = h_ctl->done && h_ctl->flag == 0;
    res.iterations = h_ctl->done ? h_ctl->iters : maxit;
    res.reduction = norm0 > 0 ? norm / norm0 : 0.0;
    if (h_ctl->flag != 0 || !(norm0 == norm0)) {
        res.status = OPMGPU_EBREAKDOWN;
        char buf[160];
        std::snprintf(buf, sizeof buf, "breakdown in BiCGSTAB (%s; ||r0|| = %.3e)", !(norm0 == norm0) ? "non-finite initial defect" : (h_ctl->flag == 1 ? "|h| < eps" : "|rho| or |omega| <= eps"), norm0);
        breakdown_note = buf;
    }
    else if (!res.converged && !prm.ignore_convergence_failure) res.status = OPMGPU_ELINSOLVE;      // ISTLSolver.hpp:358-368
    last_its = res.iterations;
    if (refreshed) its_ref = res.iterations;
    else if (coarse_lag == 1 && last_its > its_ref + std::max(1, its_ref / 4)) lag_block = 8;     // see cpr_prepare
    return res;
}

// ---- restarted GMRES (Dune::RestartedGMResSolver::apply, reached from ISTLSolver.hpp:257-264 with newton_use_gmres) ----
// LEFT-preconditioned: the residual it measures is M^-1 (b - A x).  Arnoldi with modified Gram-Schmidt: every projection is a
// k_dot launch whose partials the following k_gm_axpy re-reduces (no reduction launches, deterministic); the Hessenberg
// column, the Givens rotations and the convergence test live on the device (k_gm_givens, one thread), the host only reads the
// mapped status block once per iteration like the CPR path does.
struct GmState { double* H; double* s; double* cs; double* sn; double* y; double* gam; };      // H[(m+1) x m] row-major, all double
// gam[m+1]: the closed form of the product on the level-0 rows (k_spmv, GM): (A v_i)_row = gam[i] base_row with
//   gam[0] = 1 / beta,   gam[i+1] = (gam[i] - sum_{k<=i} h_ki gam[k]) / h_{i+1,i}      (h: the UNROTATED Hessenberg column i)

template <class S>
__global__ __launch_bounds__(kBlock) void k_gm_axpy(long n, int slot, const double* __restrict__ parts, int np, double* __restrict__ H,
                                                    const S* __restrict__ vk, S* __restrict__ w, const SolveCtl* __restrict__ ctl)
{
    __shared__ double sm[12];
    if (ctl->done) return;
    const double* const arr[1] = { parts };
    double s[1];
    reduce_partials<1>(arr, np, s, sm);
    if (blockIdx.x == 0 && threadIdx.x == 0) H[slot] = s[0];
    const S h = S(s[0]);
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) w[i] -= h * vk[i];
}
// One modified-Gram-Schmidt step fused with the next one's projection: w -= h vk with h = sum(parts_in) (recorded in H[slot]), and in the
// same pass the partials of <vnext, w> for the updated w (vnext == nullptr: of <w, w>, the norm that ends the column).  The same
// arithmetic as k_gm_axpy followed by k_dot / k_dot_owned (the partial sums run over 16-byte lanes, a fixed order: deterministic); one pass
// over w instead of two and half the launches.
template <class S>
__global__ __launch_bounds__(kBlock) void k_gm_axpy_dot(long n, int nbp, const int8_t* __restrict__ mask, int slot, const double* __restrict__ parts_in, int np,
                                                        double* __restrict__ H, const S* __restrict__ vk, S* __restrict__ w, const S* __restrict__ vnext,
                                                        double* __restrict__ parts_out, const SolveCtl* __restrict__ ctl)
{
    __shared__ double sm[12];
    if (ctl->done) return;
    const double* const arr[1] = { parts_in };
    double s[1];
    reduce_partials<1>(arr, np, s, sm);
    if (blockIdx.x == 0 && threadIdx.x == 0) H[slot] = s[0];
    const S h = S(s[0]);
    double acc[1] = { 0.0 };
    if (!mask) {
        // 16-byte lanes: three read streams and one write stream of 12 MB each want more bytes in flight per thread than one scalar
        constexpr int L = 16 / sizeof(S);
        struct alignas(16) Pack { S v[L]; };
        const long nv = n / L;
        const Pack* __restrict__ vk4 = reinterpret_cast<const Pack*>(vk);
        const Pack* __restrict__ vn4 = reinterpret_cast<const Pack*>(vnext);
        Pack* __restrict__ w4 = reinterpret_cast<Pack*>(w);
        for (long q = blockIdx.x * long(kBlock) + threadIdx.x; q < nv; q += long(gridDim.x) * kBlock) {
            Pack a = w4[q];
            const Pack b = vk4[q];
            Pack c = a;
            if (vnext) c = vn4[q];
#pragma unroll
            for (int u = 0; u < L; ++u) { a.v[u] = a.v[u] - h * b.v[u]; acc[0] += double(vnext ? c.v[u] : a.v[u]) * double(a.v[u]); }
            w4[q] = a;
        }
        for (long i = nv * L + blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) {      // (n is a multiple of 192: empty)
            const S wn = w[i] - h * vk[i];
            w[i] = wn;
            acc[0] += double(vnext ? vnext[i] : wn) * double(wn);
        }
    } else
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) {
        const S wn = w[i] - h * vk[i];
        w[i] = wn;
        if (mask[i % nbp]) acc[0] += double(vnext ? vnext[i] : wn) * double(wn);
    }
    __syncthreads();
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) parts_out[blockIdx.x] = acc[0];
}
// ---- decomposed runs: classical Gram-Schmidt.  Modified Gram-Schmidt (dune's, above) projects on v_0 .. v_i one after the other and
// needs an all-reduce per projection -- i + 2 sequential ones in column i, ~13 us each over RCCL.  Here all projections of a column are
// taken from the SAME w (one kernel, one all-reduce of i + 1 scalars), then subtracted together, then the norm of what is left (a second
// all-reduce): 2 per column.  A different rounding path than the reference's -- used only where the preconditioner is decomposed anyway;
// one GPU keeps dune's order (parity with the oracle's restatement).  The columns of a CPR solve are few (~4), so the weaker
// orthogonality of the classical form does not show (OPMGPU_GMRES_CGS=0: modified Gram-Schmidt also when decomposed).
template <class S>
__global__ __launch_bounds__(kBlock) void k_gm_multidot(long n, int nbp, const int8_t* __restrict__ mask, int cnt, const S* __restrict__ kry, const S* __restrict__ w,
                                                        double* __restrict__ parts, const SolveCtl* __restrict__ ctl)
{
    __shared__ double sm[32];
    if (ctl->done) return;
    // slot cnt: the owned part of ||w||^2 -- with the projections h_k of an orthonormal basis, ||w - sum h_k v_k||^2 = ||w||^2 - sum h_k^2
    // (Pythagoras), so the column's norm needs no second all-reduce (k_gm_cgs_update decides whether the difference is trustworthy)
    for (int k0 = 0; k0 < cnt + 1; k0 += 8) {
        double acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        const int nk = cnt + 1 - k0 < 8 ? cnt + 1 - k0 : 8;
        for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) {
            if (mask && !mask[i % nbp]) continue;
            const double wi = double(w[i]);
#pragma unroll
            for (int u = 0; u < 8; ++u) if (u < nk) acc[u] += wi * ((k0 + u < cnt) ? double(kry[long(k0 + u) * n + i]) : wi);
        }
        block_sum<8>(acc, sm);
        if (threadIdx.x == 0) for (int u = 0; u < nk; ++u) parts[long(k0 + u) * gridDim.x + blockIdx.x] = acc[u];
        __syncthreads();
    }
}
__global__ __launch_bounds__(kBlock) void k_sum_partials_multi(const double* __restrict__ parts, int np, double* __restrict__ out, const SolveCtl* __restrict__ ctl)
{
    __shared__ double sm[12];
    if (ctl->done) return;
    const double* const arr[1] = { parts + long(blockIdx.x) * np };
    double s[1];
    reduce_partials<1>(arr, np, s, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}
// w -= sum_k h_k v_k with the all-reduced h; column i of H; partial sums of the owned part of ||w||^2
template <class S>
__global__ __launch_bounds__(kBlock) void k_gm_cgs_update(long n, int nbp, const int8_t* __restrict__ mask, int cnt, int m, int col, const double* __restrict__ h,
                                                          double* __restrict__ H, const S* __restrict__ kry, S* __restrict__ w, double* __restrict__ parts_out,
                                                          const SolveCtl* __restrict__ ctl, double* __restrict__ pyth = nullptr)
{
    __shared__ double sm[8];
    __shared__ S hs[64];
    if (ctl->done) return;
    for (int k = threadIdx.x; k < cnt; k += kBlock) { hs[k] = S(h[k]); if (blockIdx.x == 0) H[k * m + col] = h[k]; }
    if (pyth && blockIdx.x == 0 && threadIdx.x == 0) {
        // ||w_new||^2 = ||w||^2 - sum h_k^2 from the all-reduced numbers (h[cnt] = ||w||^2).  The difference loses relative accuracy as
        // w falls into the span of the basis -- eps ||w||^2 / rest, i.e. ~1 % at rest = 1e-5 ||w||^2 with float vectors -- which is the
        // column that ends the solve: its entry only feeds the residual estimate |s_{i+1}|, a 1 % error there moves no stopping decision.
        // (A lucky breakdown, rest <= 0 by rounding, is clamped: the estimate becomes ~0 and the solve stops.)
        double s2 = 0.0;
        for (int k = 0; k < cnt; ++k) s2 += h[k] * h[k];
        const double rest = h[cnt] - s2;
        pyth[0] = rest > 1e-28 * h[cnt] ? rest : 1e-28 * h[cnt];
    }
    __syncthreads();
    double acc[1] = { 0.0 };
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) {
        S v = w[i];
        for (int k = 0; k < cnt; ++k) v -= hs[k] * kry[long(k) * n + i];
        w[i] = v;
        if (!mask || mask[i % nbp]) acc[0] += double(v) * double(v);
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) parts_out[blockIdx.x] = acc[0];
}
// vout = w / ||w|| with ||w||^2 in parts; slot >= 0: H[slot] = ||w|| (breakdown flag if ~0); slot < 0: the restart normalisation,
// s[0] = ||w|| and, at the very first one (first != 0), the convergence threshold
template <class S>
__global__ __launch_bounds__(kBlock) void k_gm_normalize(long n, int slot, int first, double red, const double* __restrict__ parts, int np,
                                                         double* __restrict__ H, double* __restrict__ s0, const S* __restrict__ w, S* __restrict__ vout,
                                                         SolveCtl* __restrict__ ctl, SolveCtl* __restrict__ hst, double* __restrict__ gam0 = nullptr)
{
    __shared__ double sm[12];
    if (ctl->done) return;
    const double* const arr[1] = { parts };
    double s[1];
    reduce_partials<1>(arr, np, s, sm);
    const double nrm = sqrt(s[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (slot >= 0) H[slot] = nrm; else { s0[0] = nrm; ctl->norm2 = s[0]; if (gam0) gam0[0] = 1.0 / nrm; }       // (nrm ~ 0: the solve ends below, no product reads it)
        if (first) { ctl->norm0_2 = s[0]; ctl->norm2 = s[0]; ctl->thresh2 = red * red * s[0]; }
    }
    if (!(nrm == nrm) || nrm < 1e-80) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (first && nrm == nrm) { ctl->iters = 0; ctl->done = 1; }            // zero right-hand side: converged at once
            else { ctl->flag = 2; ctl->done = 1; }                                   // breakdown in GMRes - |w| == 0
            publish(ctl, hst);
        }
        return;
    }
    const S inv = S(1.0 / nrm);
    constexpr int L = 16 / sizeof(S);
    struct alignas(16) Pack { S v[L]; };
    const long nv = n / L;
    for (long q = blockIdx.x * long(kBlock) + threadIdx.x; q < nv; q += long(gridDim.x) * kBlock) {
        Pack a = reinterpret_cast<const Pack*>(w)[q];
#pragma unroll
        for (int u = 0; u < L; ++u) a.v[u] *= inv;
        reinterpret_cast<Pack*>(vout)[q] = a;
    }
    for (long i = nv * L + blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) vout[i] = w[i] * inv;
}
// column i of the Hessenberg matrix: previous rotations, new rotation (dune generatePlaneRotation / applyPlaneRotation), |s[i+1]|
__global__ void k_gm_givens(int i, int m, int j, GmState g, SolveCtl* __restrict__ ctl, SolveCtl* __restrict__ hst, int* __restrict__ tick_ptr = nullptr, int tick = 0)
{
    if (ctl->done) { publish(ctl, hst); if (tick_ptr) { __threadfence_system(); *(volatile int*)tick_ptr = tick; } return; }
    double* H = g.H;
    if (g.gam) {   // the next column's factor on the level-0 rows, from this column's entries BEFORE the old rotations are applied to them
        double a = g.gam[i];
        for (int k = 0; k <= i; ++k) a -= H[k * m + i] * g.gam[k];
        g.gam[i + 1] = a / H[(i + 1) * m + i];
    }
    auto rot = [](double& dx, double& dy, double c, double sN) { const double t = c * dx + sN * dy; dy = -sN * dx + c * dy; dx = t; };
    for (int k = 0; k < i; ++k) rot(H[k * m + i], H[(k + 1) * m + i], g.cs[k], g.sn[k]);
    const double dx = H[i * m + i], dy = H[(i + 1) * m + i];
    const double ndx = fabs(dx), ndy = fabs(dy);
    double c, sN;
    if (ndy < 1e-15) { c = 1.0; sN = 0.0; }
    else if (ndx < 1e-15) { c = 0.0; sN = 1.0; }
    else if (ndy > ndx) { const double t = ndx / ndy; c = 1.0 / sqrt(1.0 + t * t); sN = c; c *= t; sN *= dx / ndx; sN *= dy / ndy; }
    else { const double t = ndy / ndx; c = 1.0 / sqrt(1.0 + t * t); sN = c * (dy / dx); }
    g.cs[i] = c; g.sn[i] = sN;
    rot(H[i * m + i], H[(i + 1) * m + i], c, sN);
    rot(g.s[i], g.s[i + 1], c, sN);
    const double nrm = fabs(g.s[i + 1]);
    ctl->norm2 = nrm * nrm;
    ctl->iters = j;
    if (nrm * nrm < ctl->thresh2) { ctl->done = 1; ctl->decided = j; }
    publish(ctl, hst);
    if (tick_ptr) { __threadfence_system(); *(volatile int*)tick_ptr = tick; }      // the host spins on this word instead of synchronising the stream (wait_tick)
}
// y = R^-1 s (back-substitution over the first cnt columns)
__global__ void k_gm_solve_y(int cnt, int m, GmState g)
{
    for (int a = cnt - 1; a >= 0; --a) {
        double rhs = g.s[a];
        for (int b = a + 1; b < cnt; ++b) rhs -= g.H[a * m + b] * g.y[b];
        g.y[a] = rhs / g.H[a * m + a];
    }
}
// FIRST: the first cycle of a solve from x0 = 0 -- x is not loaded (and was not cleared), the sum is added to the literal 0: the same
// operations in the same order as on a cleared x.  x2 (optional): every entry is stored there as well (LinSolver::solution_mirror)
template <class S, bool FIRST = false>
__global__ __launch_bounds__(kBlock) void k_gm_update_x(long n, int cnt, const double* __restrict__ y, const S* __restrict__ kry, S* __restrict__ x,
                                                        S* __restrict__ x2 = nullptr)
{
    constexpr int L = 16 / sizeof(S);              // 16-byte lanes (n is a multiple of 192)
    struct alignas(16) Pack { S v[L]; };
    const long nv = n / L;
    Pack* __restrict__ x4 = reinterpret_cast<Pack*>(x);
    Pack* __restrict__ m4 = reinterpret_cast<Pack*>(x2);
    for (long q = blockIdx.x * long(kBlock) + threadIdx.x; q < nv; q += long(gridDim.x) * kBlock) {
        Pack acc;
#pragma unroll
        for (int u = 0; u < L; ++u) acc.v[u] = 0;
        for (int a = cnt - 1; a >= 0; --a) {                                            // the order of dune's update(): a = i-1 .. 0
            const Pack k4 = reinterpret_cast<const Pack*>(kry + long(a) * n)[q];
            const S ya = S(y[a]);
#pragma unroll
            for (int u = 0; u < L; ++u) acc.v[u] += ya * k4.v[u];
        }
        Pack xv;
        if (FIRST) {
#pragma unroll
            for (int u = 0; u < L; ++u) xv.v[u] = 0;
        } else xv = x4[q];
#pragma unroll
        for (int u = 0; u < L; ++u) xv.v[u] += acc.v[u];
        x4[q] = xv;
        if (x2) m4[q] = xv;
    }
    for (long i = nv * L + blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) {
        S acc = 0;
        for (int a = cnt - 1; a >= 0; --a) acc += S(y[a]) * kry[long(a) * n + i];
        const S xn = (FIRST ? S(0) : x[i]) + acc;
        x[i] = xn;
        if (x2) x2[i] = xn;
    }
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_gm_defect(long n, const S* __restrict__ b, const S* __restrict__ ax, S* __restrict__ out)
{
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) out[i] = b[i] - ax[i];
}
__global__ void k_gm_reset_s(int m, GmState g) { for (int i = 1; i < m + 1; ++i) g.s[i] = 0.0; }
// opmgpu_params.gmres_verify_residual: left-preconditioned GMRES stops on || M^-1 (b - A x) ||; before the solve is reported as converged
// the TRUE defect r = b - A x is formed (the vector a restart would start from anyway) together with the owned parts of ||r||^2 and ||b||^2
template <class S>
__global__ __launch_bounds__(kBlock) void k_gm_defect_norms(long n, int nbp, const int8_t* __restrict__ mask, const S* __restrict__ b, const S* __restrict__ ax,
                                                            S* __restrict__ out, double* __restrict__ parts_r, double* __restrict__ parts_b)
{
    __shared__ double sm[8];
    double acc[2] = { 0.0, 0.0 };
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) {
        const S bi = b[i], r = bi - ax[i];
        out[i] = r;
        if (!mask || mask[i % nbp]) { acc[0] += double(r) * double(r); acc[1] += double(bi) * double(bi); }
    }
    block_sum<2>(acc, sm);
    if (threadIdx.x == 0) { parts_r[blockIdx.x] = acc[0]; parts_b[blockIdx.x] = acc[1]; }
}
// verdict of the check: ||r|| <= reduction ||b|| keeps `done`; otherwise the iteration goes on from r with the threshold on the
// preconditioned residual lowered by the factor the true residual missed its target by (and a safety factor of 2).  vr[0] = ||r||^2 / ||b||^2.
__global__ __launch_bounds__(kBlock) void k_gm_verify(const double* __restrict__ parts_r, const double* __restrict__ parts_b, int np, double red, double* __restrict__ vr,
                                                      SolveCtl* __restrict__ ctl, SolveCtl* __restrict__ hst, int* __restrict__ tick_ptr, int tick)
{
    __shared__ double sm[12];
    const double* const arr[2] = { parts_r, parts_b };
    double s[2];
    reduce_partials<2>(arr, np, s, sm);
    if (threadIdx.x == 0) {
        const double ratio2 = s[1] > 0.0 ? s[0] / s[1] : 0.0;
        vr[0] = ratio2;
        if (ratio2 == ratio2 && ratio2 > red * red) {
            ctl->done = 0;
            ctl->thresh2 = ctl->norm2 * (red * red / ratio2) * 0.25;
        } else if (ratio2 == ratio2) ctl->norm2 = ratio2 * ctl->norm0_2;      // the reported reduction is then the TRUE one (what BiCGStab's means)
        publish(ctl, hst);
        if (tick_ptr) { __threadfence_system(); *(volatile int*)tick_ptr = tick; }
    }
}

template <class S> SolveResult LinSolver::gmres(const opmgpu_params& prm)
{
    SolveResult res;
    // multi-GPU: the basis vector is halo-exchanged before every product (ghost rows of the product are zero, like in bicgstab), the
    // projections are owner-masked dot products whose partial arrays are collapsed and all-reduced before the axpy reads them: one small
    // all-reduce per projection + one for the norm with dune's modified Gram-Schmidt (j + 2 in iteration j of a cycle), two per iteration with
    // the classical form that decomposed runs use by default (k_gm_multidot; a CPR solve takes ~4 iterations).  Every rank sees
    // the same Hessenberg matrix, so the Givens / convergence decisions and the final combination are identical everywhere, and the
    // ghost entries of x are the owners' entries bit for bit (they are the same combination of exchanged basis vectors).
    const int8_t* mask = comm ? comm->owner_mask() : nullptr;
    SolverWork<S>& w = work<S>();
    const long n = long(3) * plan.nbp;
    const int gv = std::min(grid_for(n), kMaxPart);
    const int m = std::max(1, int(prm.linear_solver_restart));
    const int maxit = prm.linear_solver_maxiter;
    const bool cpr = prm.use_cpr != 0;
    // the GMRES option keeps the pressure hierarchy fresh for every matrix (it is the reference's robustness fallback; the lag policy of the
    // BiCGStab path, cpr_prepare, was measured under it without a gain on the 5-spot deck)
    lag_allowed = false;
    const bool mx = now.mixed && sizeof(S) == 8;
    if (cpr) { if (mx) cpr_prepare_mixed(); else cpr_prepare<S>(); }
    if (now.factor_deferred) { now.factor_deferred = false; if (mx) factor_async<float>(); else factor_async<S>(); }
    // one post-smoothing sweep on level 0 instead of two: measured over nine decks with wells +1..+5 % under GMRES (the same iteration
    // counts within 0.1, a cheaper cycle), -7..0 % under BiCGStab on the well-free decks (profiles/r02_amg_sweep_gmres.log)
    if (cpr) { if (mx) { if (!wf.amg->npost0_user) wf.amg->npost0 = 1; } else if (!w.amg->npost0_user) w.amg->npost0 = 1; }
    w.kry.alloc(size_t(m + 1) * n);
    // newton_use_gmres = 2: flexible (right-preconditioned) GMRES -- z_i = M^-1 v_i is KEPT, w = A z_i is orthogonalised, x += sum y_i z_i.
    // Not the reference's solver: Dune's RestartedGMResSolver (value 1) applies M from the left, which costs one application more per
    // solve (M^-1 b before the first column; a CPR solve has ~4 columns) and stops on the PRECONDITIONED residual; this form stops on the
    // true residual, the criterion of the reference's default BiCGStab.  One more basis of m vectors in memory.
    const bool flex = prm.newton_use_gmres == 2;
    wb_active = true;
    // gmres_verify_residual: the flexible form measures the true residual itself
    const bool verify = prm.gmres_verify_residual != 0 && !flex;
    bool verified = false;
    int verify_rounds = 0;
    static const bool cgs_on = env_flag("OPMGPU_GMRES_CGS", true);
    const bool cgs = comm != nullptr && cgs_on && m <= 63;          // one GPU keeps dune's modified Gram-Schmidt
    if (cgs) cgs_parts.alloc(size_t(m + 2) * gv + size_t(m + 2));
    // Decomposed, classical Gram-Schmidt: the halo of the vector a column ends with travels WITH the all-reduce of its projections (one
    // fused operation, CommBase::allreduce_sum_halo_*): w = M^-1 A v_i gets its ghost entries from the owners, the update w -= sum h_k v_k
    // and the normalisation run over ghost rows too (the basis vectors' ghost entries are the owners' values by induction), so v_{i+1} needs
    // no exchange of its own before the next product -- one latency per column less, and one at the start (the first vector's halo rides on
    // the all-reduce of its norm).  A/B: OPMGPU_GMRES_FUSE_HALO=0
    static const bool fuse_env = env_flag("OPMGPU_GMRES_FUSE_HALO", true);
    const bool fuse_halo = comm != nullptr && cgs && fuse_env && !flex;
    // The column's norm by Pythagoras (one all-reduce per column) -- for the loose reductions of Newton solves only (>= 1e-4, a handful of
    // columns): the identity needs an orthonormal basis, and classical Gram-Schmidt loses orthogonality as the columns add up -- at a
    // 1e-10 reduction (~20 columns) the decomposed runs left the single-domain Newton path with it (tests/test_gpu_dist_shm.py, cpr_gmres),
    // with the explicit norm (a second all-reduce) they do not.  OPMGPU_GMRES_PYTH=0: always the explicit norm.
    static const bool cgs_pyth_env = env_flag("OPMGPU_GMRES_PYTH", true);
    const bool cgs_pyth = cgs_pyth_env && prm.linear_solver_reduction >= 1e-4;
    if (flex) w.kryz.alloc(size_t(m) * n);
    // The lean start and end of a solve (linsolver.hpp, lean_solve): no clear of x, gmbuf cleared by k_ctl_init, no k_gm_reset_s behind
    // that clear, the solution stored to the caller's mirror as well.  Not with the flexible form or the verified residual, which keep
    // the launches they were validated with.
    const bool lean = lean_conditions() && !flex && !verify;
    // (double only, like the closed form of the product: float and mixed solves keep the plain sequence, whose rounding the verified
    // residual's float cases are compared against; cpr_apply adds the plan's and the factors' conditions)
    cancel_p_now = cpr && cpr_cancel_p && plain_setup() && !flex && !verify && sizeof(S) == 8 && !mx;
    S* mirror = nullptr;
    if constexpr (sizeof(S) == 8) { if (lean) mirror = solution_mirror; }
    solution_mirror = nullptr; mirror_written = false;
    if (cpr) { if (mx) wf.amg->lane_restrict = lean; else w.amg->lane_restrict = lean; }
    gmbuf.alloc(size_t(m + 1) * m + (m + 1) + 3 * m + 8 + (m + 1));
    if (!lean) gmbuf.zero(stream);
    GmState g; g.H = gmbuf.p; g.s = g.H + size_t(m + 1) * m; g.cs = g.s + (m + 1); g.sn = g.cs + m; g.y = g.sn + m; g.gam = nullptr;
    // Closed form of the product on the level-0 rows (k_spmv, GM): on the conditions of bicgstab()'s `closed`, and
    //   double only       -- in float the recurrence of gamma drifts from the explicit product by more than the Arnoldi estimate tolerates
    //                        (the true preconditioned residual 3x the estimate at a reduction of 4e-7);
    //   not flexible      -- its product multiplies z_i = M^-1 v_i and its basis is built from A z_i, not M^-1 A v_i;
    //   not verified      -- the check takes `done` back and may continue a cycle from a threshold the recurrence was not carried for; kept
    //                        on the explicit product it was validated with;
    //   one GPU           -- the halo exchange overwrites ghost entries of v_i (bicgstab masks those rows, GMRES' classical Gram-Schmidt path is
    //                        a different recurrence);
    //   relaxation 1      -- with w != 1 (A M^-1 d)_i = d_i - (1 - w) z_i needs the second stage's input, which a basis vector does not have;
    //   no Woodbury       -- the wells' correction behind the ILU0 changes M^-1 d on the perforated rows, which their neighbours' rows of A read: A M^-1
    //                        is then no longer the identity on the level-0 rows next to a perforation;
    //   no row transform  -- cpr_reference_transform is the comparison mode against the reference's formulation (L A x = L b, optionally its point
    //                        ILU0): it keeps the explicit product, the closed form was not validated on the transformed system.
    // The perforated level-0 rows keep the full product (gm_light).
    const bool gm_closed = closed_form_level0 && emulate_ranks <= 1 && !(cpr && ell.relax != 1.0) && !mx && !(cpr && now.point_stage2) && fill_level == 0      // bicgstab()'s `closed`
                           && sizeof(S) == 8 && !flex && !verify && !comm && prm.ilu_relaxation == 1.0 && !(well_woodbury && wb_active) && prm.cpr_reference_transform == 0;
    const int8_t* gm_mask = nullptr;
    if (gm_closed) {
        g.gam = g.y + m + 8;
        if (lowrank.perf_of_row) {
            if (gm_light_for != lowrank.perf_of_row || gm_light_plan != plan_id || gm_light.n != size_t(plan.nbp)) {
                gm_light.alloc(plan.nbp);
                hipLaunchKernelGGL(k_unperforated_mask, dim3(grid_for(plan.nbp)), dim3(kBlock), 0, stream, plan.nbp, lowrank.perf_of_row, gm_light.p);
                gm_light_for = lowrank.perf_of_row; gm_light_plan = plan_id;
            }
            gm_mask = gm_light.p;
        }
    }
    const S* gm_base = w.b.p;          // the vector the cycle started from: b, after a restart the true defect
    double* parts = partials.p;
    double* parts2 = partials.p + npart;                             // second partial array: producer and consumer of a fused step differ
    double* red1 = partials.p + size_t(6) * npart;                   // the all-reduced scalar of a projection (multi-GPU)
    SolveCtl* d_ctl = ctl.p;
    // <a, b> into a partial array the consumer kernels re-reduce: np entries on one GPU, one all-reduced entry otherwise
    const double* dot_arr = parts; int dot_np = gv;
    // (multi-GPU) a partial array collapsed and all-reduced into red1 -- with halo_of's halo exchange in the same operation
    auto allreduce_dot = [&](const double* arr, S* halo_of = nullptr) {
        hipLaunchKernelGGL((k_sum_partials<1>), dim3(1), dim3(kBlock), 0, stream, arr, (const double*)nullptr, gv, red1);
        if (halo_of) allreduce_halo(comm, red1, 1, halo_of, stream); else comm->allreduce_sum(red1, 1, stream);
        dot_arr = red1; dot_np = 1;
    };
    auto dot = [&](const S* a_, const S* b_) {
        if (!comm) { hipLaunchKernelGGL((k_dot<S>), dim3(gv), dim3(kBlock), 0, stream, n, a_, b_, parts); dot_arr = parts; dot_np = gv; return; }
        hipLaunchKernelGGL((k_dot_owned<S>), dim3(gv), dim3(kBlock), 0, stream, n, plan.nbp, mask, a_, b_, parts);
        allreduce_dot(parts);
    };
    auto product = [&](S* vin, S* out, const SolveCtl* c, bool exchange = true) {          // out = A vin (vin's ghost entries refreshed first unless they are current)
        if (comm && exchange) halo(comm, vin, stream);
        lowrank_reduce<S>(vin, c);
        hipLaunchKernelGGL((k_spmv<S, 0>), dim3(std::min(grid8_for(plan.nb), 4 * kMaxPart)), dim3(kBlock), 0, stream, xcd_mode(), plan.nb, plan.nbp,
                           dp.slice_ptr.p, dp.col.p, matrix<S>(), (const S*)vin, out, (const S*)nullptr, mask, c,
                           (double*)nullptr, (double*)nullptr, (const S*)nullptr, (const S*)nullptr, 0, S(0), lowrank, (const int8_t*)nullptr);
    };
    // A v_i inside a cycle: the level-0 rows from gam[i] and the cycle's base vector
    auto product_basis = [&](int i, S* out, const SolveCtl* c, bool exchange) {
        if (!gm_closed) { product(w.kry.p + size_t(i) * n, out, c, exchange); return; }
        S* vin = w.kry.p + size_t(i) * n;
        lowrank_reduce<S>(vin, c);
        hipLaunchKernelGGL((k_spmv<S, 0, 1>), dim3(std::min(grid8_for(plan.nb), 4 * kMaxPart)), dim3(kBlock), 0, stream, xcd_mode(), plan.nb, plan.nbp,
                           dp.slice_ptr.p, dp.col.p, matrix<S>(), (const S*)vin, out, (const S*)nullptr, mask, c,
                           (double*)nullptr, (double*)nullptr, gm_base, (const S*)nullptr, int(plan.level_ptr[1]), S(0), lowrank, gm_mask, 0, (const int8_t*)nullptr,
                           (const double*)(g.gam + i));
    };
    auto V = [&](int k) { return w.kry.p + size_t(k) * n; };
    auto precond = [&](const S* d, S* out) { precond_apply<S>(d, out, prm.ilu_relaxation, d_ctl, cpr); };
    auto Z = [&](int k) { return w.kryz.p + size_t(k) * n; };
    auto normalize_start = [&](S* src, int first) {          // v0 = src / ||src||, s[0] = ||src||  (src = M^-1 defect, flexible: the defect)
        if (fuse_halo) {        // ||src||^2 over the owned rows and src's halo in one operation: v0 then carries the owners' ghost values
            hipLaunchKernelGGL((k_dot_owned<S>), dim3(gv), dim3(kBlock), 0, stream, n, plan.nbp, mask, (const S*)src, (const S*)src, parts);
            allreduce_dot(parts, src);
        } else
        dot(src, src);
        hipLaunchKernelGGL((k_gm_normalize<S>), dim3(gv), dim3(kBlock), 0, stream, n, -1, first, prm.linear_solver_reduction, dot_arr, dot_np,
                           g.H, g.s, src, V(0), d_ctl, h_ctl_dev, g.gam);
        // s[1..m] = 0 for the new cycle (k_gm_normalize wrote s[0]).  Lean, first cycle: k_ctl_init has just cleared all of gmbuf, s included
        if (!(lean && first)) hipLaunchKernelGGL(k_gm_reset_s, dim3(1), dim3(1), 0, stream, m, g);
    };
    // x0 = 0: defect = b.  Lean: x is not cleared, the first cycle's combination writes it (k_gm_update_x<S, true>); the exits that
    // leave without a combination clear it below
    bool x_written = !lean;
    if (!lean) {
        w.x.zero(stream);
        hipLaunchKernelGGL(k_ctl_init, dim3(1), dim3(1), 0, stream, d_ctl, h_ctl_dev, prm.linear_solver_reduction);
    } else
        hipLaunchKernelGGL(k_ctl_init, dim3(1), dim3(kBlock), 0, stream, d_ctl, h_ctl_dev, prm.linear_solver_reduction, gmbuf.p, int(gmbuf.n));
    if (flex) normalize_start(w.b.p, 1);
    else { precond(w.b.p, w.t.p); normalize_start(w.t.p, 1); }
    // no synchronisation here: the first iteration is enqueued behind the set-up (factorisation, hierarchy, first application); a zero
    // defect sets `done` on the device, the iteration's kernels then return at once and its status check reports 0 iterations
    int j = 1;
    bool stop = false;
    // the next iteration's product is enqueued BEFORE the host waits for this iteration's verdict (v_{i+1} is complete once k_gm_normalize
    // ran; if the verdict is "converged" the product's kernels see `done` and return): the device starts on it while the host is still
    // reading the status word and enqueueing the rest.  Measured +0.4 % (inside the run-to-run noise), and every solve ends with one such
    // launch that returns at once, which drags the profiler's per-kernel average of the SpMV away from its real duration: off by default
    // (OPMGPU_GMRES_SPECULATE=1 switches it on)
    static const bool speculate = env_flag("OPMGPU_GMRES_SPECULATE", false);
    while (j <= maxit && !stop) {
        int i = 0, cycle_misses = 0;
        bool product_enqueued = false;
        for (; i < m && j <= maxit && !stop; ++i, ++j) {
            hipEvent_t kt_a;
            if (flex) {
                precond(V(i), Z(i));                                   // z_i = M^-1 v_i
                kt_a = kt.begin();
                product(Z(i), w.t.p, (const SolveCtl*)d_ctl);          // w = A z_i
                kt.end(KT_SPMV1, kt_a);
            } else {
                if (!product_enqueued) {
                    kt_a = kt.begin();
                    product_basis(i, w.v.p, (const SolveCtl*)d_ctl, !fuse_halo);
                    kt.end(KT_SPMV1, kt_a);
                }
                product_enqueued = false;
                precond(w.v.p, w.t.p);                                 // w = M^-1 A v_i
            }
            kt_a = kt.begin();
            if (cgs) {
                // decomposed (cgs implies comm): classical Gram-Schmidt, two all-reduces per column (k_gm_multidot)
                const int cnt = i + 1;
                hipLaunchKernelGGL((k_gm_multidot<S>), dim3(gv), dim3(kBlock), 0, stream, n, plan.nbp, mask, cnt, (const S*)w.kry.p, (const S*)w.t.p, cgs_parts.p, (const SolveCtl*)d_ctl);
                double* hsum = cgs_parts.p + size_t(m + 2) * gv;              // cnt projections + ||w||^2, all-reduced together
                hipLaunchKernelGGL(k_sum_partials_multi, dim3(cnt + 1), dim3(kBlock), 0, stream, (const double*)cgs_parts.p, gv, hsum, (const SolveCtl*)d_ctl);
                if (fuse_halo) allreduce_halo(comm, hsum, cnt + 1, w.t.p, stream); else comm->allreduce_sum(hsum, cnt + 1, stream);
                double* pyth = cgs_pyth ? g.y + m + 2 : (double*)nullptr;    // norm^2 of what is left, by Pythagoras
                hipLaunchKernelGGL((k_gm_cgs_update<S>), dim3(gv), dim3(kBlock), 0, stream, n, plan.nbp, mask, cnt, m, i, (const double*)hsum, g.H,
                                   (const S*)w.kry.p, w.t.p, parts, (const SolveCtl*)d_ctl, pyth);
                if (cgs_pyth) { dot_arr = pyth; dot_np = 1; }          // one all-reduce per column: the norm of what is left comes from Pythagoras
                else allreduce_dot(parts);
            } else {
            // modified Gram-Schmidt, each step's update fused with the next step's projection (k_gm_axpy_dot)
            dot((const S*)V(0), (const S*)w.t.p);
            for (int k = 0; k <= i; ++k) {
                double* out = (dot_arr == parts) ? parts2 : parts;
                hipLaunchKernelGGL((k_gm_axpy_dot<S>), dim3(gv), dim3(kBlock), 0, stream, n, plan.nbp, mask, k * m + i, dot_arr, dot_np, g.H, (const S*)V(k), w.t.p,
                                   k < i ? (const S*)V(k + 1) : (const S*)nullptr, out, (const SolveCtl*)d_ctl);
                if (!comm) { dot_arr = out; dot_np = gv; } else allreduce_dot(out);
            }
            }
            hipLaunchKernelGGL((k_gm_normalize<S>), dim3(gv), dim3(kBlock), 0, stream, n, (i + 1) * m + i, 0, 0.0, dot_arr, dot_np, g.H, g.s,
                               (const S*)w.t.p, V(i + 1), d_ctl, h_ctl_dev);
            const int tick = ++tick_seq;
            hipLaunchKernelGGL(k_gm_givens, dim3(1), dim3(1), 0, stream, i, m, j, g, d_ctl, h_ctl_dev, poll_status ? h_tick_dev : (int*)nullptr, tick);
            kt.end(KT_VECTOR, kt_a);
            if (speculate && !flex && i + 1 < m && j + 1 <= maxit) {
                kt_a = kt.begin();
                product_basis(i + 1, w.v.p, (const SolveCtl*)d_ctl, !fuse_halo);
                kt.end(KT_SPMV1, kt_a);
                product_enqueued = true;
            }
            wait_tick(tick);
            if (h_ctl->done) stop = true;
            if (stop && verify && h_ctl->flag == 0 && h_ctl->iters > 0) {
                // gmres_verify_residual: the preconditioned residual met the threshold -- does the true one?  The candidate x + V y of the
                // i + 1 completed columns goes into a scratch vector (x itself is only updated when the cycle ends), one product, one pass
                // for || b - A xt ||^2 and || b ||^2.  If it misses the target, `done` is taken back, the threshold on the preconditioned
                // residual is lowered in proportion, and the SAME cycle goes on with its next column: the Krylov space is kept.
                const int cnt = i + 1;
                hipLaunchKernelGGL(k_gm_solve_y, dim3(1), dim3(1), 0, stream, cnt, m, g);
                OPMGPU_HIP(hipMemcpyAsync(w.y.p, w.x.p, size_t(n) * sizeof(S), hipMemcpyDeviceToDevice, stream));
                hipLaunchKernelGGL((k_gm_update_x<S>), dim3(gv), dim3(kBlock), 0, stream, n, cnt, (const double*)g.y, (const S*)w.kry.p, w.y.p);
                product(w.y.p, w.p.p, (const SolveCtl*)nullptr);
                hipLaunchKernelGGL((k_gm_defect_norms<S>), dim3(gv), dim3(kBlock), 0, stream, n, plan.nbp, mask, (const S*)w.b.p, (const S*)w.p.p, w.r.p, parts, parts2);
                const double* pr = parts; const double* pb = parts2; int np_v = gv;
                if (comm) {
                    hipLaunchKernelGGL((k_sum_partials<2>), dim3(1), dim3(kBlock), 0, stream, (const double*)parts, (const double*)parts2, gv, red1);
                    comm->allreduce_sum(red1, 2, stream);
                    pr = red1; pb = red1 + 1; np_v = 1;
                }
                const int vtick = ++tick_seq;
                hipLaunchKernelGGL(k_gm_verify, dim3(1), dim3(kBlock), 0, stream, pr, pb, np_v, prm.linear_solver_reduction, g.y + m, d_ctl, h_ctl_dev,
                                   poll_status ? h_tick_dev : (int*)nullptr, vtick);
                wait_tick(vtick);
                verified = true;
                if (!h_ctl->done) {
                    stop = false; ++verify_rounds;
                    product_enqueued = false;          // (OPMGPU_GMRES_SPECULATE: the next column's product was enqueued while `done` was up and returned at once)
                    // a second miss in the same cycle (the first already with float vectors, whose Arnoldi estimate keeps falling while
                    // b - A x does not: measured on the 1 M-cell deck, in-cycle continuation never reached 1e-5 there): the recurrence's
                    // estimate has drifted from the real defect -- end the cycle here and restart from the true defect, which the restart
                    // path forms from the updated x (iterative refinement)
                    if (++cycle_misses >= (sizeof(S) == 4 ? 1 : 2)) { ++i; ++j; break; }      // (float vectors: refine at the first miss)
                }
            }
        }
        if (h_ctl->flag != 0) break;                                   // breakdown: dune throws, no update
        if (h_ctl->done && h_ctl->iters == 0) break;                   // zero defect: x = 0 is the solution, no column was built
        // x += sum_a y_a v_a with R y = s   (i columns were completed)
        hipLaunchKernelGGL(k_gm_solve_y, dim3(1), dim3(1), 0, stream, i, m, g);
        if (!x_written) hipLaunchKernelGGL((k_gm_update_x<S, true>), dim3(gv), dim3(kBlock), 0, stream, n, i, (const double*)g.y, (const S*)w.kry.p, w.x.p, mirror);
        else hipLaunchKernelGGL((k_gm_update_x<S>), dim3(gv), dim3(kBlock), 0, stream, n, i, (const double*)g.y, flex ? (const S*)w.kryz.p : (const S*)w.kry.p, w.x.p, mirror);
        x_written = true;
        if (!stop && j <= maxit) {                                     // restart from the true defect
            product(w.x.p, w.v.p, (const SolveCtl*)nullptr);
            hipLaunchKernelGGL((k_gm_defect<S>), dim3(gv), dim3(kBlock), 0, stream, n, (const S*)w.b.p, (const S*)w.v.p, w.r.p);
            gm_base = w.r.p;
            if (flex) normalize_start(w.r.p, 0);
            else { precond(w.r.p, w.t.p); normalize_start(w.t.p, 0); }
        }
    }
    // lean: no combination ran (zero defect, a breakdown in the first cycle, no iteration allowed) -- x = 0, as the clear would have left it;
    // the mirror is then not written and the caller copies x as before
    if (!x_written) w.x.zero(stream);
    else mirror_written = mirror != nullptr;
    // the status block is current (the last iteration's tick was waited for); what is still in flight (the combination of the basis
    // vectors into x) is ordered before everything the caller enqueues next on this stream.  Without polling: synchronise.
    if (!poll_status || !stop) OPMGPU_HIP(hipStreamSynchronize(stream));
    if (comm) comm->check_async();
    const double norm0 = std::sqrt(h_ctl->norm0_2), norm = std::sqrt(h_ctl->norm2);
    res.converged = h_ctl->done && h_ctl->flag == 0;
    res.iterations = (h_ctl->done && h_ctl->flag == 0) ? h_ctl->iters : j - 1;
    res.reduction = norm0 > 0 ? norm / norm0 : 0.0;
    (void)verified;
    last_verify_rounds = verify_rounds;
    if (h_ctl->flag != 0 || !(norm0 == norm0)) {
        res.status = OPMGPU_EBREAKDOWN;
        char buf[160];
        std::snprintf(buf, sizeof buf, "breakdown in GMRes (%s; column %d, ||M^-1 r0|| = %.3e)", !(norm0 == norm0) ? "non-finite initial defect" : (h_ctl->flag == 2 ? "|w| == 0" : "non-finite Hessenberg entry"), j, norm0);
        breakdown_note = buf;
    }
    else if (!res.converged && !prm.ignore_convergence_failure) res.status = OPMGPU_ELINSOLVE;
    last_its = res.iterations;              // the back-off of the lag policy, as at the end of bicgstab (see cpr_prepare)
    if (refreshed) its_ref = res.iterations;
    else if (coarse_lag == 1 && last_its > its_ref + std::max(1, its_ref / 4)) lag_block = 8;
    return res;
}
