// coarse_space.inl -- global (subdomain) coarse space of the CPR pressure stage (included by linsolver.hip): the k_cs_* kernels,
// LinSolver::coarse_setup / coarse_domains / coarse_begin.  Applied by cpr_apply (cpr.inl); its restriction carried along the BiCGStab
// recurrences by krylov.inl.

// ---- global coarse space of the CPR pressure stage (multi-GPU / emulated ranks): one unknown per subdomain ----
// The AMG is subdomain-local, so nothing in it couples the subdomains: pressure error that is smooth across several of them is
// only reduced at the cuts and the iteration count grows with the number of ranks (measured with OPMGPU_EMULATE_RANKS: 4.3 -> 8.0
// iterations at 8 slabs).  Classical remedy (Nicolaides coarse space): before the local V-cycle the residual is corrected by the
// Galerkin problem on the span of the subdomains' indicator vectors, A_c = P^T A_p P (n_sub x n_sub, inverted on every rank),
//   e = A_c^-1 P^T r ;  r' = r - A_p P e ;  x_p = P e + Vcycle(r') .
// P e is constant per subdomain, so its ghost entries are known without a halo exchange; the only communication is the sum of the
// n_sub restricted residuals (one small all-reduce per application) and of the rows of A_c (once per matrix).
__global__ __launch_bounds__(kBlock) void k_cs_sub_emulated(int nb, int nbp, int nranks, const int32_t* __restrict__ nat, int32_t* __restrict__ sub)
{
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nbp) return;
    sub[row] = row < nb ? int32_t(long(nat[row]) * nranks / nb) : 0;
}
// partial sums per workgroup: out[block][k] for k < ns2 (fixed order inside the block: thread 0 adds the per-thread tables of its
// block serially -- small tables, rows of one block belong to one or two subdomains).  Deterministic.
template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_matrix(int nb, int nbp, int ns, const int32_t* __restrict__ slice_ptr, const int32_t* __restrict__ col,
                                                      const int16_t* __restrict__ rowlen, const int32_t* __restrict__ sub, const int8_t* __restrict__ owned,
                                                      const S* __restrict__ w, const S* __restrict__ A, double* __restrict__ cA)
{
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nb || (owned && !owned[row])) return;
    const int base = slice_ptr[row >> 6], lane = row & 63, a = sub[row];
    const double w0 = double(w[row]), w1 = double(w[nbp + row]), w2 = double(w[2 * long(nbp) + row]);
    int bcur = -1; double acc = 0.0;
    for (int k = 0, len = rowlen[row]; k < len; ++k) {
        const long e = long(base + k) * 64 + lane;
        const S* bl = A + (e >> 6) * 576 + (e & 63);
        const double v = w0 * double(bl[0]) + w1 * double(bl[192]) + w2 * double(bl[384]);
        const int b = sub[col[e]];
        if (b != bcur) { if (bcur >= 0) atomicAdd(&cA[a * ns + bcur], acc); bcur = b; acc = 0.0; }
        acc += v;
    }
    if (bcur >= 0) atomicAdd(&cA[a * ns + bcur], acc);
}
__global__ void k_cs_invert(int ns, const double* __restrict__ cA, double* __restrict__ inv)
{
    // Gauss-Jordan with partial pivoting, one thread (ns <= 64)
    extern __shared__ double m[];          // [ns][2 ns]
    const int n2 = 2 * ns;
    for (int i = 0; i < ns; ++i) for (int j = 0; j < n2; ++j) m[i * n2 + j] = j < ns ? cA[i * ns + j] : (j - ns == i ? 1.0 : 0.0);
    for (int p = 0; p < ns; ++p) {
        int piv = p;
        for (int i = p + 1; i < ns; ++i) if (fabs(m[i * n2 + p]) > fabs(m[piv * n2 + p])) piv = i;
        if (m[piv * n2 + p] == 0.0) { for (int i = 0; i < ns * ns; ++i) inv[i] = 0.0; return; }     // singular: no correction
        if (piv != p) for (int j = 0; j < n2; ++j) { const double t = m[p * n2 + j]; m[p * n2 + j] = m[piv * n2 + j]; m[piv * n2 + j] = t; }
        const double d = 1.0 / m[p * n2 + p];
        for (int j = 0; j < n2; ++j) m[p * n2 + j] *= d;
        for (int i = 0; i < ns; ++i) if (i != p) { const double f = m[i * n2 + p]; for (int j = 0; j < n2; ++j) m[i * n2 + j] -= f * m[p * n2 + j]; }
    }
    for (int i = 0; i < ns; ++i) for (int j = 0; j < ns; ++j) inv[i * ns + j] = m[i * n2 + ns + j];
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_restrict(int nb, const int32_t* __restrict__ sub, const int8_t* __restrict__ owned, const S* __restrict__ r,
                                                        double* __restrict__ cr, const SolveCtl* __restrict__ ctl)
{
    if (ctl && ctl->done) return;
    const int row = blockIdx.x * kBlock + threadIdx.x;
    const bool act = row < nb && (!owned || owned[row]);
    const int a = act ? sub[row] : -1;
    const double v = act ? double(r[row]) : 0.0;
    // wave-uniform subdomain (the usual case): one atomic per wave, fixed lane order inside it
    const int a0 = __shfl(a, 0, 64);
    if (__all(a == a0)) { const double s_ = wave_sum(v); if ((threadIdx.x & 63) == 0 && a0 >= 0) atomicAdd(&cr[a0], s_); }
    else if (act) atomicAdd(&cr[a], v);
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_correct(int nb, int nbp, int ns, const int32_t* __restrict__ slice_ptr, const int32_t* __restrict__ col,
                                                       const int16_t* __restrict__ rowlen, const int32_t* __restrict__ sub, const S* __restrict__ w,
                                                       const S* __restrict__ A, const double* __restrict__ inv, const double* __restrict__ cr, S omega,
                                                       const S* __restrict__ dinv, S* __restrict__ b, S* __restrict__ x0, S* __restrict__ xc,
                                                       const SolveCtl* __restrict__ ctl)
{
    __shared__ double e[64];
    if (ctl && ctl->done) return;
    if (threadIdx.x < ns) { double s_ = 0.0; for (int k = 0; k < ns; ++k) s_ += inv[threadIdx.x * ns + k] * cr[k]; e[threadIdx.x] = s_; }
    __syncthreads();
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nb) return;
    const int base = slice_ptr[row >> 6], lane = row & 63;
    const double w0 = double(w[row]), w1 = double(w[nbp + row]), w2 = double(w[2 * long(nbp) + row]);
    double acc = 0.0;
    for (int k = 0, len = rowlen[row]; k < len; ++k) {
        const long en = long(base + k) * 64 + lane;
        const S* bl = A + (en >> 6) * 576 + (en & 63);
        acc += (w0 * double(bl[0]) + w1 * double(bl[192]) + w2 * double(bl[384])) * e[sub[col[en]]];
    }
    const S rn = S(double(b[row]) - acc);
    b[row] = rn; x0[row] = omega * dinv[row] * rn; xc[row] = S(e[sub[row]]);
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_add(int nb, const S* __restrict__ x, const S* __restrict__ xc, S* __restrict__ out, const SolveCtl* __restrict__ ctl)
{
    if (ctl && ctl->done) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nb) out[i] = x[i] + xc[i];
}

// real multi-GPU (one subdomain per process): deterministic versions -- per-workgroup partials, re-reduced in a fixed order
template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_rsum(int nb, const int8_t* __restrict__ owned, const S* __restrict__ r, double* __restrict__ parts,
                                                    const SolveCtl* __restrict__ ctl)
{
    __shared__ double sm[4];
    if (ctl && ctl->done) return;
    double acc[1] = { 0.0 };
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < nb; i += long(gridDim.x) * kBlock) if (!owned || owned[i]) acc[0] += double(r[i]);
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) parts[blockIdx.x] = acc[0];
}
__global__ __launch_bounds__(kBlock) void k_cs_place(int np, const double* __restrict__ parts, int ns, int mine, double* __restrict__ cr,
                                                     const SolveCtl* __restrict__ ctl)
{
    __shared__ double sm[12];
    if (ctl && ctl->done) return;
    const double* const arr[1] = { parts };
    double s_[1];
    reduce_partials<1>(arr, np, s_, sm);
    if (threadIdx.x < ns) cr[threadIdx.x] = threadIdx.x == mine ? s_[0] : 0.0;
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_rowparts(int nb, int nbp, LinSolver::CsSlots sl, const int32_t* __restrict__ slice_ptr, const int32_t* __restrict__ col,
                                                        const int16_t* __restrict__ rowlen, const int32_t* __restrict__ sub, const int8_t* __restrict__ owned,
                                                        const S* __restrict__ w, const S* __restrict__ A, double* __restrict__ parts, S* __restrict__ T)
{
    // T[q][row] = sum_j A_p(row, j) [subdomain(j) == slot q]: what the per-application correction needs of the matrix
    __shared__ double sm[32];
    double acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (long row = blockIdx.x * long(kBlock) + threadIdx.x; row < nb; row += long(gridDim.x) * kBlock) {
        if (owned && !owned[row]) { for (int q = 0; q < sl.n; ++q) T[long(q) * nbp + row] = S(0); continue; }
        double mine[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        const int base = slice_ptr[row >> 6], lane = row & 63;
        const double w0 = double(w[row]), w1 = double(w[nbp + row]), w2 = double(w[2 * long(nbp) + row]);
        for (int k = 0, len = rowlen[row]; k < len; ++k) {
            const long e = long(base + k) * 64 + lane;
            const S* bl = A + (e >> 6) * 576 + (e & 63);
            const double v = w0 * double(bl[0]) + w1 * double(bl[192]) + w2 * double(bl[384]);
            const int s_ = sl.slot_of_sub[sub[col[e]]];
#pragma unroll
            for (int q = 0; q < 8; ++q) mine[q] += (q == s_) ? v : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) { acc[q] += mine[q]; if (q < sl.n) T[long(q) * nbp + row] = S(mine[q]); }
    }
    block_sum<8>(acc, sm);
    if (threadIdx.x == 0) for (int q = 0; q < 8; ++q) parts[long(q) * gridDim.x + blockIdx.x] = acc[q];
}
__global__ __launch_bounds__(kBlock) void k_cs_place_row(int np, const double* __restrict__ parts, LinSolver::CsSlots sl, int ns, int mine, double* __restrict__ cA)
{
    __shared__ double sm[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int q = 0; q < sl.n; ++q) {
        double v = 0.0;
        for (int i = threadIdx.x; i < np; i += kBlock) v += parts[long(q) * np + i];
        const double s_ = wave_sum(v);
        __syncthreads();
        if (lane == 0) sm[wv] = s_;
        __syncthreads();
        if (threadIdx.x == 0) cA[mine * ns + sl.sub_of_slot[q]] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    }
}

// ---- several coarse unknowns per rank (cs_m index-range blocks of the owned cells; own blocks occupy the slots 0 .. m-1) ----
// A_c(rank*m + b, sub_of_slot[q]) = sum over the owned rows of block b of T[q][row]; one slot per blockIdx.y, partials per workgroup
template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_block_rows(int nb, int nbp, const int8_t* __restrict__ blk, const S* __restrict__ T, double* __restrict__ parts)
{
    __shared__ double sm[32];
    const int q = blockIdx.y;
    double acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (long row = blockIdx.x * long(kBlock) + threadIdx.x; row < nb; row += long(gridDim.x) * kBlock) {
        const int b = blk[row];
        if (b < 0) continue;
        const double v = double(T[long(q) * nbp + row]);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] += (u == b) ? v : 0.0;
    }
    block_sum<8>(acc, sm);
    if (threadIdx.x == 0) for (int u = 0; u < 8; ++u) parts[(long(q) * 8 + u) * gridDim.x + blockIdx.x] = acc[u];
}
__global__ __launch_bounds__(kBlock) void k_cs_place_blocks(int np, const double* __restrict__ parts, LinSolver::CsSlots sl, int ns, int m, int mine, double* __restrict__ cA)
{
    __shared__ double sm[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int q = 0; q < sl.n; ++q)
        for (int b = 0; b < m; ++b) {
            double v = 0.0;
            for (int i = threadIdx.x; i < np; i += kBlock) v += parts[(long(q) * 8 + b) * np + i];
            const double s_ = wave_sum(v);
            __syncthreads();
            if (lane == 0) sm[wv] = s_;
            __syncthreads();
            if (threadIdx.x == 0) cA[(mine * m + b) * ns + sl.sub_of_slot[q]] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
        }
}
// restricted residual of the own blocks: cr[rank*m + b] = sum over the rows of block b (zeros elsewhere: the all-reduce gathers)
template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_rsum_blocks(int nb, const int8_t* __restrict__ blk, const S* __restrict__ r, double* __restrict__ parts,
                                                           const SolveCtl* __restrict__ ctl)
{
    __shared__ double sm[32];
    if (ctl && ctl->done) return;
    double acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < nb; i += long(gridDim.x) * kBlock) {
        const int b = blk[i];
        if (b < 0) continue;
        const double v = double(r[i]);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] += (u == b) ? v : 0.0;
    }
    block_sum<8>(acc, sm);
    if (threadIdx.x == 0) for (int u = 0; u < 8; ++u) parts[long(u) * gridDim.x + blockIdx.x] = acc[u];
}
__global__ __launch_bounds__(kBlock) void k_cs_place_cr(int np, const double* __restrict__ parts, int ns, int m, int mine, double* __restrict__ cr,
                                                        const SolveCtl* __restrict__ ctl)
{
    __shared__ double sm[4];
    __shared__ double tot[8];
    if (ctl && ctl->done) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int b = 0; b < m; ++b) {
        double v = 0.0;
        for (int i = threadIdx.x; i < np; i += kBlock) v += parts[long(b) * np + i];
        const double s_ = wave_sum(v);
        __syncthreads();
        if (lane == 0) sm[wv] = s_;
        __syncthreads();
        if (threadIdx.x == 0) tot[b] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    }
    __syncthreads();
    if (threadIdx.x < ns) { const int b = threadIdx.x - mine * m; cr[threadIdx.x] = (b >= 0 && b < m) ? tot[b] : 0.0; }
}
// wells with blocks: the pair (perforation i, perforations of block b) adds w_i . P_i . sum_{j in b} Q_j[:, pressure] to T[b][row_i]
// (own blocks are the slots 0 .. m-1); A_c then takes it from T like every other entry.  One workgroup per well, fixed order.
template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_wells_blocks(LowRankOp lr, int nbp, int m, const int8_t* __restrict__ blk, const S* __restrict__ w, S* __restrict__ T)
{
    __shared__ double sm[28];
    __shared__ double q7s[8][7];
    const int wl = blockIdx.x;
    for (int b = 0; b < m; ++b) {
        double q7[7] = { 0, 0, 0, 0, 0, 0, 0 };
        for (int j = lr.connpos[wl] + threadIdx.x; j < lr.connpos[wl + 1]; j += kBlock)
            if (blk[lr.perf_row[j]] == b) for (int k = 0; k < 7; ++k) q7[k] += lr.Q[21 * long(j) + 3 * k];
        __syncthreads();
        block_sum<7>(q7, sm);
        if (threadIdx.x == 0) for (int k = 0; k < 7; ++k) q7s[b][k] = q7[k];
    }
    __syncthreads();
    for (int i = lr.connpos[wl] + threadIdx.x; i < lr.connpos[wl + 1]; i += kBlock) {
        const int row = lr.perf_row[i];
        const double wa[3] = { double(w[row]), double(w[nbp + row]), double(w[2 * long(nbp) + row]) };
        for (int b = 0; b < m; ++b) {
            double t = 0.0;
            for (int a = 0; a < 3; ++a) { double pa = 0.0; for (int k = 0; k < 7; ++k) pa += lr.P[21 * long(i) + 7 * a + k] * q7s[b][k]; t += wa[a] * pa; }
            T[long(b) * nbp + row] = S(double(T[long(b) * nbp + row]) + t);
        }
    }
}

// wells (rank-7 operator per well, all perforations on this rank): their part of P^T (A_p + wells) P and of the row sums.  Without it
// a rate-controlled well's diagonal terms are counted although the Schur complement cancels them for a constant pressure shift.
// One workgroup per well, fixed reduction order; k_cs_wells_sum then adds the per-well totals to A_c(mine, mine) in well order.
template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_wells(LowRankOp lr, int nbp, const S* __restrict__ w, S* __restrict__ T0, double* __restrict__ well_tot)
{
    __shared__ double sm[28];
    __shared__ double q7s[7];
    const int wl = blockIdx.x;
    double q7[7] = { 0, 0, 0, 0, 0, 0, 0 };
    for (int j = lr.connpos[wl] + threadIdx.x; j < lr.connpos[wl + 1]; j += kBlock)
        for (int k = 0; k < 7; ++k) q7[k] += lr.Q[21 * long(j) + 3 * k];              // pressure column of Q_j
    block_sum<7>(q7, sm);
    if (threadIdx.x == 0) for (int k = 0; k < 7; ++k) q7s[k] = q7[k];
    __syncthreads();
    double tot[1] = { 0.0 };
    for (int i = lr.connpos[wl] + threadIdx.x; i < lr.connpos[wl + 1]; i += kBlock) {
        const int row = lr.perf_row[i];
        const double wa[3] = { double(w[row]), double(w[nbp + row]), double(w[2 * long(nbp) + row]) };
        double t = 0.0;
        for (int a = 0; a < 3; ++a) { double pa = 0.0; for (int k = 0; k < 7; ++k) pa += lr.P[21 * long(i) + 7 * a + k] * q7s[k]; t += wa[a] * pa; }
        T0[row] = S(double(T0[row]) + t);
        tot[0] += t;
    }
    __syncthreads();
    block_sum<1>(tot, sm);
    if (threadIdx.x == 0) well_tot[wl] = tot[0];
}
__global__ void k_cs_wells_sum(int nw, const double* __restrict__ well_tot, int mine, int ns, double* __restrict__ cA)
{
    double s_ = 0.0;
    for (int wl = 0; wl < nw; ++wl) s_ += well_tot[wl];
    cA[mine * ns + mine] += s_;
}

template <class S>
__global__ __launch_bounds__(kBlock) void k_cs_correct_fast(int nb, int nbp, int ns, LinSolver::CsSlots sl, const int32_t* __restrict__ sub, const S* __restrict__ T,
                                                            const double* __restrict__ inv, const double* __restrict__ cr, S omega, const S* __restrict__ dinv,
                                                            S* __restrict__ b, S* __restrict__ x0, S* __restrict__ xc, const SolveCtl* __restrict__ ctl)
{
    __shared__ double e[64];
    if (ctl && ctl->done) return;
    if (threadIdx.x < ns) { double s_ = 0.0; for (int k = 0; k < ns; ++k) s_ += inv[threadIdx.x * ns + k] * cr[k]; e[threadIdx.x] = s_; }
    __syncthreads();
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nb) return;
    double acc = 0.0;
    for (int q = 0; q < sl.n; ++q) acc += e[sl.sub_of_slot[q]] * double(T[long(q) * nbp + row]);
    const S rn = S(double(b[row]) - acc);
    b[row] = rn; x0[row] = omega * dinv[row] * rn; xc[row] = S(e[sub[row]]);
}

template <class S> void LinSolver::coarse_setup(bool rowparts_done)
{
    SolverWork<S>& w = work<S>();
    const int ns = coarse_nsub;
    const bool emulated = !comm && emulate_ranks > 1;
    const int mine = comm ? comm->my_rank() : 0;
    double* cA = cs_buf.p; double* inv = cA + ns * ns;
    if (!emulated && cs_m > 1) {
        // several coarse unknowns per rank: T is complete (fused row pass or k_cs_rowparts below), the rows of A_c are block sums of it
        double* rparts = cs_buf.p + size_t(2) * ns * ns + ns;
        if (!rowparts_done) {
            const int gp0 = std::min(grid_for(plan.nb), kMaxPart);
            hipLaunchKernelGGL((k_cs_rowparts<S>), dim3(gp0), dim3(kBlock), 0, stream, plan.nb, plan.nbp, cs_slots, dp.slice_ptr.p, dp.col.p, dp.rowlen.p, cs_sub.p,
                               comm ? comm->owner_mask() : (const int8_t*)nullptr, (const S*)w.cprw.p, matrix<S>(), rparts, w.csT.p);
        }
        if (lowrank.nw > 0)
            hipLaunchKernelGGL((k_cs_wells_blocks<S>), dim3(lowrank.nw), dim3(kBlock), 0, stream, lowrank, plan.nbp, cs_m, (const int8_t*)cs_blk.p, (const S*)w.cprw.p, w.csT.p);
        const int gp = std::min(grid_for(plan.nb), 128);           // 64 partial arrays (slot x block) of gp entries in the scratch
        hipLaunchKernelGGL((k_cs_block_rows<S>), dim3(gp, cs_slots.n), dim3(kBlock), 0, stream, plan.nb, plan.nbp, (const int8_t*)cs_blk.p, (const S*)w.csT.p, rparts);
        hipLaunchKernelGGL(k_cs_place_blocks, dim3(1), dim3(kBlock), 0, stream, gp, (const double*)rparts, cs_slots, ns, cs_m, mine, cA);
        if (comm) comm->allreduce_sum(cA, ns * ns, stream);
    } else if (!emulated) {
        const int gp = rowparts_done ? std::min(grid_for(plan.nbp), kCsRowParts) : std::min(grid_for(plan.nb), kMaxPart);
        double* rparts = cs_buf.p + size_t(2) * ns * ns + ns;      // 8 slots x gp partials
        if (!rowparts_done)
            hipLaunchKernelGGL((k_cs_rowparts<S>), dim3(gp), dim3(kBlock), 0, stream, plan.nb, plan.nbp, cs_slots, dp.slice_ptr.p, dp.col.p, dp.rowlen.p, cs_sub.p,
                               comm ? comm->owner_mask() : (const int8_t*)nullptr, (const S*)w.cprw.p, matrix<S>(), rparts, w.csT.p);
        hipLaunchKernelGGL(k_cs_place_row, dim3(1), dim3(kBlock), 0, stream, gp, (const double*)rparts, cs_slots, ns, mine, cA);
        if (lowrank.nw > 0) {
            cs_well_tot.alloc(lowrank.nw);
            hipLaunchKernelGGL((k_cs_wells<S>), dim3(lowrank.nw), dim3(kBlock), 0, stream, lowrank, plan.nbp, (const S*)w.cprw.p, w.csT.p, cs_well_tot.p);
            hipLaunchKernelGGL(k_cs_wells_sum, dim3(1), dim3(1), 0, stream, lowrank.nw, (const double*)cs_well_tot.p, mine, ns, cA);
        }
        if (comm) comm->allreduce_sum(cA, ns * ns, stream);
    } else {
        hipLaunchKernelGGL((k_cs_matrix<S>), dim3(grid_for(plan.nb)), dim3(kBlock), 0, stream, plan.nb, plan.nbp, ns, dp.slice_ptr.p, dp.col.p, dp.rowlen.p, cs_sub.p,
                           (const int8_t*)nullptr, (const S*)w.cprw.p, matrix<S>(), cA);
    }
    hipLaunchKernelGGL(k_cs_invert, dim3(1), dim3(1), size_t(2) * ns * ns * sizeof(double), stream, ns, (const double*)cA, inv);
}
// subdomain map, slots and buffers of the coarse space (before the fused row pass writes into them)
// Subdomains of the coarse space (real ranks or one GPU): m coarse unknowns per rank -- index-range blocks of its owned cells; a single
// GPU keeps the one global constant -- the largest m <= requested that every rank can hold (own blocks + the neighbours' blocks seen
// in ghost rows <= 8 slots, n_ranks * m <= 64), agreed collectively.  Cached per communicator / plan.  COLLECTIVE when stale.
void LinSolver::coarse_domains()
{
    const void* key = comm ? static_cast<const void*>(comm) : static_cast<const void*>(this);
    if (cs_sub.p && cs_sub.n == size_t(plan.nbp) && cs_for == key && cs_blk.p) return;
    const int mine = comm ? comm->my_rank() : 0;
    std::vector<int32_t> sub;
    std::vector<int8_t> blk;
    // with wells ONE unknown per rank: measured with real ranks, blocks and the wells' rank-7 operator do not mix (2 ranks: 35 -> 77
    // iterations over six Newton iterations, 4 ranks: 43 -> 96), while one unknown per rank still pays there (4 ranks: 67 -> 43)
    // ... unless the CALLER supplies the blocks (opmgpu_comm_set_coarse_blocks: sub-slabs along the cut direction keep vertical wells whole)
    int m = (comm && comm->user_coarse_blocks() > 0) ? comm->user_coarse_blocks() : (comm && !run_has_wells) ? std::max(1, std::min(cs_blocks_req, 8)) : 1;
    while (m > 1 && comm->num_ranks() * m > 64) m /= 2;
    for (;; m /= 2) {
        if (comm) comm->coarse_blocks_of_rows(plan, m, stream, sub, blk); else { sub.assign(plan.nbp, 0); blk.assign(plan.nbp, int8_t(0)); }
        cs_slots.n = 0;
        for (int i = 0; i < 64; ++i) cs_slots.slot_of_sub[i] = 0;
        bool overflow = false;
        auto add = [&](int sd) {
            for (int q = 0; q < cs_slots.n; ++q) if (cs_slots.sub_of_slot[q] == sd) return;
            if (cs_slots.n < 8 && sd >= 0 && sd < 64) { cs_slots.slot_of_sub[sd] = int8_t(cs_slots.n); cs_slots.sub_of_slot[cs_slots.n++] = sd; }
            else overflow = true;
        };
        for (int b = 0; b < m; ++b) add(mine * m + b);             // own blocks: slots 0 .. m-1
        for (int32_t sd : sub) add(sd);
        double flag = overflow ? 1.0 : 0.0;
        if (comm) {
            DevArray<double> f; f.alloc(1);
            OPMGPU_HIP(hipMemcpyAsync(f.p, &flag, sizeof(double), hipMemcpyHostToDevice, stream));
            comm->allreduce_max(f.p, 1, stream);
            OPMGPU_HIP(hipMemcpyAsync(&flag, f.p, sizeof(double), hipMemcpyDeviceToHost, stream));
            OPMGPU_HIP(hipStreamSynchronize(stream));
        }
        if (flag == 0.0) break;
        if (m == 1) throw HipError(OPMGPU_EINVAL, "coarse space: more than 7 neighbour ranks or more than 64 ranks (set OPMGPU_COARSE=0)");
    }
    cs_m = m;
    for (int r = plan.nb; r < plan.nbp; ++r) blk[r] = int8_t(-1);
    cs_sub.alloc(plan.nbp); cs_sub.upload(sub, stream);
    cs_blk.alloc(plan.nbp); cs_blk.upload(blk, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    cs_for = key;
}

// buffers of the coarse space (before the fused row pass writes into them); the emulated subdomain map
template <class S> void LinSolver::coarse_begin()
{
    SolverWork<S>& w = work<S>();
    const int ns = coarse_nsub;
    const bool emulated = !comm && emulate_ranks > 1;
    if (emulated) {
        const void* key = static_cast<const void*>(this);
        if (!cs_sub.p || cs_sub.n != size_t(plan.nbp) || cs_for != key || cs_emulated_ns != ns) {
            cs_sub.alloc(plan.nbp);
            hipLaunchKernelGGL(k_cs_sub_emulated, dim3(grid_for(plan.nbp)), dim3(kBlock), 0, stream, plan.nb, plan.nbp, ns, dp.nat.p, cs_sub.p);
            cs_for = key; cs_emulated_ns = ns; cs_blk.release();
        }
    }
    cs_buf.alloc(size_t(2) * ns * ns + ns + size_t(8) * kCsRowParts);          // scratch: 8 x 8192 partials (also 64 arrays of 128 for the blocks)
    OPMGPU_HIP(hipMemsetAsync(cs_buf.p, 0, (size_t(2) * ns * ns + ns) * sizeof(double), stream));
    w.cxc.alloc(plan.nbp);
    if (!emulated) w.csT.alloc(size_t(cs_slots.n) * plan.nbp);
}
