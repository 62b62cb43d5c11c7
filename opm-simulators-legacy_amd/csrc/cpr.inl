// cpr.inl -- the CPR preconditioner (included by linsolver.hip, behind coarse_space.inl and the stage-2 / elliptic parts): the k_cpr_*
// kernels, the reference's formulation as an option (cpr_reference_transform), cpr_prepare with the policies of the pressure
// hierarchy (lagged coarse operators, scaling of the coarse-grid corrections) and the two-stage application cpr_apply.

// ---- CPR (NewtonIterationBlackoilCPR.cpp:79-185) ----
// formEllipticSystem (NewtonIterationUtilities.cpp:197-287): the pressure equation of a cell is the sum of those (matbal-scaled)
// phase equations whose pressure derivative is strong on the diagonal -- |J_ii| / (column sum of |J_ji|, j != i) > 0.01 --
// with the reference's fix-up for a weak oil equation (:233-252): if no equation is strong the oil equation alone is used.
// Equations here are ordered water, oil, gas (the reference swaps oil first: "a concession to MRST").  Weights are 0 / 1.
template <class S>
__device__ inline void cpr_row_weights(int lane, int base, int len, int nl, const int32_t* __restrict__ tpos, const S* __restrict__ A, int mode, S w[3])
{
    if (mode == 1) {
        // quasi-IMPES: w = first row of A_ii^-1, i.e. the combination of the cell's equations that eliminates its own saturation /
        // composition unknowns from the diagonal block (w . A_ii = [1 0 0]); not what the reference does (experiment knob)
        const long e = long(base + nl) * 64 + lane;
        const S* b = A + (e >> 6) * 576 + (e & 63);
        double m[9];
        for (int q = 0; q < 9; ++q) m[q] = double(b[q * 64]);
        const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
        const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
        const double id = (det != 0.0 && det == det) ? 1.0 / det : 0.0;
        double w0 = c0 * id, w1 = (m[2] * m[7] - m[1] * m[8]) * id, w2 = (m[1] * m[5] - m[2] * m[4]) * id;
        if (id == 0.0) { w0 = 1.0; w1 = 1.0; w2 = 1.0; }
        w[0] = S(w0); w[1] = S(w1); w[2] = S(w2);
        return;
    }
    double sod[3] = { 0.0, 0.0, 0.0 }, dj[3] = { 0.0, 0.0, 0.0 };
    for (int k = 0; k < len; ++k) {
        const long e = long(base + k) * 64 + lane;
        if (k == nl) {
            const S* b = A + (e >> 6) * 576 + (e & 63);
            dj[0] = fabs(double(b[0])); dj[1] = fabs(double(b[192])); dj[2] = fabs(double(b[384]));
        } else {
            const int t = tpos[e];
            if (t < 0) continue;
            const S* b = A + long(t >> 6) * 576 + (t & 63);
            sod[0] += fabs(double(b[0])); sod[1] += fabs(double(b[192])); sod[2] += fabs(double(b[384]));
        }
    }
    const bool sw = dj[0] / sod[0] > 0.01, sg = dj[2] / sod[2] > 0.01;       // NaN (0/0) compares false like the reference's Eigen cast
    bool so = dj[1] / sod[1] > 0.01;
    if (!so && !sw && !sg) so = true;
    w[0] = sw ? S(1) : S(0); w[1] = so ? S(1) : S(0); w[2] = sg ? S(1) : S(0);
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_cpr_weights(int nb, int nbp, const int32_t* __restrict__ slice_ptr, const int16_t* __restrict__ rowlen,
                                                        const int16_t* __restrict__ nlower, const int32_t* __restrict__ tpos, const S* __restrict__ A,
                                                        S* __restrict__ w, int mode)
{
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nb) return;
    S ww[3];
    cpr_row_weights<S>(row & 63, slice_ptr[row >> 6], rowlen[row], nlower[row], tpos, A, mode, ww);
    w[row] = ww[0]; w[nbp + row] = ww[1]; w[2 * long(nbp) + row] = ww[2];
}
// the same for a list of rows: the assembly kernel wrote the weights of every row from the reservoir equations, the device well model then
// changed the diagonal blocks of its perforated cells -- their weights are redone from the final matrix (off-diagonal blocks, and with
// them every other row's column sums, are untouched by the wells)
template <class S>
__global__ __launch_bounds__(kBlock) void k_cpr_weights_rows(int nrows, const int32_t* __restrict__ rows, int nbp, const int32_t* __restrict__ slice_ptr,
                                                             const int16_t* __restrict__ rowlen, const int16_t* __restrict__ nlower, const int32_t* __restrict__ tpos,
                                                             const S* __restrict__ A, S* __restrict__ w, int mode)
{
    // one wavefront per row, one lane per entry (rows are <= 64 wide here or fall back to the serial walk): the serial form is a chain of
    // ~14 dependent round trips (transposed position -> block), 17 us for 500 rows in one workgroup
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (q >= nrows) return;
    const int row = rows[q];
    const int lane = row & 63, base = slice_ptr[row >> 6], len = rowlen[row], nl = nlower[row];
    if (mode == 1 || len > 64) {
        if (l == 0) { S ww[3]; cpr_row_weights<S>(lane, base, len, nl, tpos, A, mode, ww); w[row] = ww[0]; w[nbp + row] = ww[1]; w[2 * long(nbp) + row] = ww[2]; }
        return;
    }
    double sod[3] = { 0.0, 0.0, 0.0 }, dj[3] = { 0.0, 0.0, 0.0 };
    if (l < len) {
        const long e = long(base + l) * 64 + lane;
        if (l == nl) {
            const S* b = A + (e >> 6) * 576 + (e & 63);
            dj[0] = fabs(double(b[0])); dj[1] = fabs(double(b[192])); dj[2] = fabs(double(b[384]));
        } else {
            const int t = tpos[e];
            if (t >= 0) {
                const S* b = A + long(t >> 6) * 576 + (t & 63);
                sod[0] = fabs(double(b[0])); sod[1] = fabs(double(b[192])); sod[2] = fabs(double(b[384]));
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { sod[a] = wave_sum(sod[a]); dj[a] = wave_sum(dj[a]); }       // fixed lane order: deterministic
    if (l == 0) {
        const bool sw = dj[0] / sod[0] > 0.01, sg = dj[2] / sod[2] > 0.01;       // as cpr_row_weights
        bool so = dj[1] / sod[1] > 0.01;
        if (!so && !sw && !sg) so = true;
        w[row] = sw ? S(1) : S(0); w[nbp + row] = so ? S(1) : S(0); w[2 * long(nbp) + row] = sg ? S(1) : S(0);
    }
}
// A_p(i,j) = sum over the selected equations of A_ij[eq][pressure]; one thread per row (padding slots included: value 0)
template <class S>
__global__ __launch_bounds__(kBlock) void k_extract_pressure(int nb, int nbp, const int32_t* __restrict__ slice_ptr, const S* __restrict__ w,
                                                             const S* __restrict__ A, S* __restrict__ Ap)
{
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nbp) return;
    const int base = slice_ptr[row >> 6], width = slice_ptr[(row >> 6) + 1] - base, lane = row & 63;
    const bool real = row < nb;
    const S w0 = real ? w[row] : S(0), w1 = real ? w[nbp + row] : S(0), w2 = real ? w[2 * long(nbp) + row] : S(0);
    for (int k = 0; k < width; ++k) {
        const long e = long(base + k) * 64 + lane;
        const S* b = A + (e >> 6) * 576 + (e & 63);
        Ap[e] = w0 * b[0] + w1 * b[192] + w2 * b[384];
    }
}
// r_p = the same combination of the three (scaled) phase residuals.  CSM (coarse space of the pressure stage): 0 = none -- the first
// pre-smoothing sweep of the V-cycle from a zero guess is fused here (one launch less); 1 / 2 = the restriction of r_p onto the one
// unknown / the blocks of this rank is fused instead (per-workgroup partials, k_cs_place / k_cs_place_cr reduce them in a fixed order;
// the coarse-space correction then writes the first sweep from the corrected residual)
template <class S, int CSM>
__global__ __launch_bounds__(kBlock) void k_cpr_sum_eqs(int nb, int nbp, const S* __restrict__ d, const S* __restrict__ w, S* __restrict__ bp, S omega,
                                                        const S* __restrict__ dinv, S* __restrict__ x0, const SolveCtl* __restrict__ ctl,
                                                        const int8_t* __restrict__ owned, const int8_t* __restrict__ blk, double* __restrict__ parts,
                                                        S* __restrict__ xw = nullptr, int nw = 0)
{
    __shared__ double sm[32];
    if (ctl && ctl->done) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nw) xw[i] = S(0);              // bordered level 0: the wells' unknowns start from zero (a memset is two more launches)
    S b = S(0);
    if (i < nb) {
        b = w[i] * d[i] + w[nbp + i] * d[nbp + i] + w[2 * long(nbp) + i] * d[2 * long(nbp) + i];
        bp[i] = b;
        if (CSM == 0) x0[i] = omega * dinv[i] * b;
    }
    if (CSM == 1) {
        double acc[1] = { (i < nb && (!owned || owned[i])) ? double(b) : 0.0 };
        block_sum<1>(acc, sm);
        if (threadIdx.x == 0) parts[blockIdx.x] = acc[0];
    }
    if (CSM == 2) {
        const int bl = i < nb ? int(blk[i]) : -1;
        double acc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = (u == bl) ? double(b) : 0.0;
        block_sum<8>(acc, sm);
        if (threadIdx.x == 0) for (int u = 0; u < 8; ++u) parts[long(u) * gridDim.x + blockIdx.x] = acc[u];
    }
}
// Border of the level-0 pressure system (amg.hpp): one unknown per well, its bhp.  With q_a = sum_j cq_s[a][j] (flux equations) the
// well's control equation g(q, bhp) = 0 is the extra ROW: sum_j (sum_a g_a dcq_s[a][j]/dp_j) dp_j + (g_bhp + sum_a g_a sum_j dcq_s[a][j]/dbhp)
// dbhp; the extra COLUMN is what the cells' (matbal-scaled, CPR-weighted) equations see of bhp: -sum_a w_a(row) scale_a dcq_s[a][j]/dbhp.
// Eliminating the unknown again gives the pressure part of the explicit Schur complement the reference forms (minus the wellbore-mixture
// terms) -- without its clique fill.  One workgroup per well; out = [bcol (nperf) | crow (nperf) | dw (nw)].
template <class S>
__global__ __launch_bounds__(kBlock) void k_cpr_border(LowRankOp lr, int nbp, const S* __restrict__ w, S* __restrict__ out, double colscale = 1.0)
{
    __shared__ double sm[4];
    const int k = blockIdx.x;
    const double* g = lr.ctrl_row + 4 * k;
    const double ew = lr.eff[k];            // the column is a cell-row term: weighed by the well's efficiency factor; the row is the well's own equation
    double acc[1] = { 0.0 };
    for (int j = lr.connpos[k] + threadIdx.x; j < lr.connpos[k + 1]; j += kBlock) {
        const double* Fs = lr.Fsave + 21 * long(j);
        const int row = lr.perf_row[j];
        double bc = 0.0, cr = 0.0;
        for (int a = 0; a < 3; ++a) {
            bc -= double(w[long(a) * nbp + row]) * lr.scale[a] * Fs[18 + a];
            cr += g[a] * Fs[3 * a];
            acc[0] += g[a] * Fs[18 + a];
        }
        out[j] = S(colscale * (ew * bc)); out[lr.nperf + j] = S(cr);
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) {
        double d = g[3] + acc[0];
        if (d == 0.0 || !(d == d)) d = 1.0;          // a decoupled (dead) well: identity row
        out[2 * lr.nperf + k] = S(d);
    }
}
// z = d - A [x_p; 0; 0]   (only the pressure column of every block is read: 1/3 of the matrix)
template <class S>
__global__ __launch_bounds__(kBlock) void k_cpr_presidual(int xm, int nb, int nbp, const int32_t* __restrict__ slice_ptr, const int32_t* __restrict__ col,
                                                          const S* __restrict__ val, const S* __restrict__ d, const S* __restrict__ xp,
                                                          S* __restrict__ z, const int8_t* __restrict__ mask, const SolveCtl* __restrict__ ctl,
                                                          int phase = 0, const int8_t* __restrict__ interior = nullptr)
{
    if (ctl && ctl->done) return;
    const int nchunks = (nb + kBlock - 1) / kBlock;
    const int ch = xcd_first(nchunks, xm);
    if (ch >= xcd_end(nchunks, xm)) return;
    const int row = ch * kBlock + threadIdx.x;
    if (row >= nb) return;
    if (phase && (phase == 1) != (interior[row] != 0)) return;          // halo exchange of x_p in flight: see k_spmv
    const int base = slice_ptr[row >> 6], width = slice_ptr[(row >> 6) + 1] - base, lane = row & 63;
    const S* __restrict__ v = val + vidx(base, lane);
    const int32_t* __restrict__ c = col + long(base) * 64 + lane;
    if (mask && !mask[row]) { z[row] = 0; z[nbp + row] = 0; z[2 * long(nbp) + row] = 0; return; }     // ghost rows stay zero (block-Jacobi second stage)
    S z0 = d[row], z1 = d[nbp + row], z2 = d[2 * long(nbp) + row];
    for (int k = 0; k < width; ++k) {
        const S x0 = xp[c[k * 64]];
        const S* __restrict__ b = v + k * 576;
        z0 -= b[0] * x0; z1 -= b[192] * x0; z2 -= b[384] * x0;
    }
    z[row] = z0; z[nbp + row] = z1; z[2 * long(nbp) + row] = z2;
}
// The same on the level-0 rows alone, WITHOUT the row's own diagonal term: s_r = d_r - sum_{k != r} A_rk[:,0] x_p,k, written where z_r is
// (LinSolver::cpr_factor_p: the top level's forward sweep reads it through its L blocks and forms its own rows' part itself; nothing is
// launched for, or written to, the top rows).  Single GPU only: no owner mask, no halo phases.
template <class S>
__global__ __launch_bounds__(kBlock) void k_cpr_presidual_l0(int xm, int n0, int nbp, const int32_t* __restrict__ slice_ptr, const int32_t* __restrict__ col,
                                                             const int16_t* __restrict__ nlower, const S* __restrict__ val, const S* __restrict__ d,
                                                             const S* __restrict__ xp, S* __restrict__ z, const SolveCtl* __restrict__ ctl)
{
    if (ctl && ctl->done) return;
    const int nchunks = (n0 + kBlock - 1) / kBlock;
    const int ch = xcd_first(nchunks, xm);
    if (ch >= xcd_end(nchunks, xm)) return;
    const int row = ch * kBlock + threadIdx.x;
    if (row >= n0) return;
    // (the last slice of the level may hold top rows too: its width is theirs as well, the slots past this row's own entries are padding, value 0)
    const int base = slice_ptr[row >> 6], width = slice_ptr[(row >> 6) + 1] - base, lane = row & 63, nl = nlower[row];
    const S* __restrict__ v = val + vidx(base, lane);
    const int32_t* __restrict__ c = col + long(base) * 64 + lane;
    S z0 = d[row], z1 = d[nbp + row], z2 = d[2 * long(nbp) + row];
    for (int k = 0; k < nl; ++k) {               // (a level-0 row has no lower entries: nl = 0, the diagonal is its first slot)
        const S x0 = xp[c[k * 64]];
        const S* __restrict__ b = v + k * 576;
        z0 -= b[0] * x0; z1 -= b[192] * x0; z2 -= b[384] * x0;
    }
    for (int k = nl + 1; k < width; ++k) {
        const S x0 = xp[c[k * 64]];
        const S* __restrict__ b = v + k * 576;
        z0 -= b[0] * x0; z1 -= b[192] * x0; z2 -= b[384] * x0;
    }
    z[row] = z0; z[nbp + row] = z1; z[2 * long(nbp) + row] = z2;
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_cpr_add_p(int nb, const S* __restrict__ xp, S* __restrict__ v, const SolveCtl* __restrict__ ctl, S c)
{
    // c = cpr_relax: the reference's CPRPreconditioner scales the pressure part by it when it is not 1 (the ILU0 part carries it already)
    if (ctl && ctl->done) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nb) return;
    v[i] += c * xp[i];
}

// level 0 of the decomposed pressure cycle (LinSolver::cpr_l0_halo): the ghost entries of the iterate from the exchanged staging vector;
// the ghost rows are identity rows, so their right-hand side follows (b = x: zero residual, stationary under the Jacobi sweep)
template <class S>
__global__ __launch_bounds__(kBlock) void k_l0_ghosts(int nb, const int8_t* __restrict__ owned, const S* __restrict__ hx, S* __restrict__ x, S* __restrict__ b,
                                                      const SolveCtl* __restrict__ ctl)
{
    if (ctl && ctl->done) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nb && !owned[i]) { const S v = hx[i]; x[i] = v; b[i] = v; }
}

// the whole per-row set-up of the pressure stage in ONE pass over the matrix (per Newton iteration): weights (k_cpr_weights), the
// pressure matrix (k_extract_pressure) and, with CS, the coarse-space row parts (k_cs_rowparts) -- same arithmetic as the three
template <class S, bool CS, bool WR>
__global__ __launch_bounds__(kBlock) void k_cpr_rows(int nb, int nbp, int mode, LinSolver::CsSlots sl, const int32_t* __restrict__ slice_ptr, const int32_t* __restrict__ col,
                                                     const int16_t* __restrict__ rowlen, const int16_t* __restrict__ nlower, const int32_t* __restrict__ tpos,
                                                     const int32_t* __restrict__ sub, const int8_t* __restrict__ owned, const S* __restrict__ A,
                                                     S* __restrict__ w, S* __restrict__ Ap, double* __restrict__ parts, S* __restrict__ T)
{
    __shared__ double sm[32];
    double acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (long row = blockIdx.x * long(kBlock) + threadIdx.x; row < nbp; row += long(gridDim.x) * kBlock) {
        const int base = slice_ptr[row >> 6], width = slice_ptr[(row >> 6) + 1] - base, lane = row & 63;
        if (row >= nb) { for (int k = 0; k < width; ++k) Ap[long(base + k) * 64 + lane] = S(0); continue; }
        const int len = rowlen[row];
        S ww[3];
        if (WR) { ww[0] = w[row]; ww[1] = w[nbp + row]; ww[2] = w[2 * long(nbp) + row]; }       // written by the assembly (k_flux)
        else {
            cpr_row_weights<S>(lane, base, len, nlower[row], tpos, A, mode, ww);
            w[row] = ww[0]; w[nbp + row] = ww[1]; w[2 * long(nbp) + row] = ww[2];
        }
        const bool cs = CS && !(owned && !owned[row]);
        const double w0 = double(ww[0]), w1 = double(ww[1]), w2 = double(ww[2]);
        double mine[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        for (int k = 0; k < width; ++k) {
            const long e = long(base + k) * 64 + lane;
            const S* bl = A + (e >> 6) * 576 + (e & 63);
            const S b0 = bl[0], b1 = bl[192], b2 = bl[384];
            Ap[e] = ww[0] * b0 + ww[1] * b1 + ww[2] * b2;
            if (cs && k < len) {
                const double v = w0 * double(b0) + w1 * double(b1) + w2 * double(b2);
                const int s_ = sl.slot_of_sub[sub[col[e]]];
#pragma unroll
                for (int q = 0; q < 8; ++q) mine[q] += (q == s_) ? v : 0.0;
            }
        }
        if (CS) {
#pragma unroll
            for (int q = 0; q < 8; ++q) { acc[q] += mine[q]; if (q < sl.n) T[long(q) * nbp + row] = S(mine[q]); }
        }
    }
    if (CS) {
        block_sum<8>(acc, sm);
        if (threadIdx.x == 0) for (int q = 0; q < 8; ++q) parts[long(q) * gridDim.x + blockIdx.x] = acc[q];
    }
}

template <class S> void LinSolver::cpr_reweigh_rows(const int32_t* d_rows, int nrows)
{
    if (nrows <= 0 || !weights_from_assembly) return;
    hipLaunchKernelGGL((k_cpr_weights_rows<S>), dim3((nrows + 3) / 4), dim3(kBlock), 0, stream, nrows, d_rows, plan.nbp, dp.slice_ptr.p, dp.rowlen.p, dp.nlower.p,
                       dp.tpos.p, matrix<S>(), work<S>().cprw.p, cpr_weight_mode);
}

// ---- the reference's CPR formulation as an option (opmgpu_params.cpr_reference_transform) ----
// L of a row from its 0/1 dominance weights (formEllipticSystem's l1, l21 / l22, l31 / l33, NewtonIterationUtilities.cpp:218-262, in this
// library's equation order water, oil, gas; the reference swaps oil to the front first, so "the first equation" there is the oil slot):
//   row 0 = pscale * sum of the dominant equations                              (pressure equation; pscale = 200 bar, CPR.cpp:117-121)
//   row 1 = the water equation -- or the oil equation, if oil is weak and water at least as dominant as gas (l21)
//   row 2 = the gas equation   -- or the oil equation, if oil is weak and gas more dominant than water (l31)
// (a weak oil equation with nothing else dominant stays in the sum alone: the weights already say so, no swap)
template <class S>
__device__ __forceinline__ void ref_L(const S* __restrict__ w, int nbp, int row, double pscale, double (&L)[9])
{
    const double w0 = double(w[row]), w1 = double(w[nbp + row]), w2 = double(w[2 * long(nbp) + row]);
    const bool oil_weak = w1 == 0.0;
    const bool l21 = oil_weak && w0 >= w2, l31 = oil_weak && !(w0 >= w2);
    L[0] = pscale * w0; L[1] = pscale * w1; L[2] = pscale * w2;
    L[3] = l21 ? 0.0 : 1.0; L[4] = l21 ? 1.0 : 0.0; L[5] = 0.0;
    L[6] = 0.0; L[7] = l31 ? 1.0 : 0.0; L[8] = l31 ? 0.0 : 1.0;
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_ref_transform_rows(int nb, int nbp, double pscale, const int32_t* __restrict__ slice_ptr, const int16_t* __restrict__ rowlen,
                                                               const S* __restrict__ w, S* __restrict__ A)
{
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nb) return;
    double L[9];
    ref_L<S>(w, nbp, row, pscale, L);
    const int base = slice_ptr[row >> 6], lane = row & 63, len = rowlen[row];
    for (int k = 0; k < len; ++k) {
        S* b = A + long(base + k) * 576 + lane;
        double m[9], o[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) m[q] = double(b[q * 64]);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int v = 0; v < 3; ++v) o[3 * i + v] = L[3 * i] * m[v] + L[3 * i + 1] * m[3 + v] + L[3 * i + 2] * m[6 + v];
#pragma unroll
        for (int q = 0; q < 9; ++q) b[q * 64] = S(o[q]);
    }
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_ref_transform_vec(int nb, int nbp, double pscale, const S* __restrict__ w, S* __restrict__ b)
{
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nb) return;
    double L[9];
    ref_L<S>(w, nbp, row, pscale, L);
    const double r0 = double(b[row]), r1 = double(b[nbp + row]), r2 = double(b[2 * long(nbp) + row]);
    b[row] = S(L[0] * r0 + L[1] * r1 + L[2] * r2); b[nbp + row] = S(L[3] * r0 + L[4] * r1 + L[5] * r2); b[2 * long(nbp) + row] = S(L[6] * r0 + L[7] * r1 + L[8] * r2);
}
// the wells' low-rank part A += P_w Q_w: the rows of P ([nperf][3][7]) belong to the perforated cells' equations
template <class S>
__global__ __launch_bounds__(kBlock) void k_ref_transform_lowrank(LowRankOp lr, int nbp, double pscale, const S* __restrict__ w, double* __restrict__ P)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= lr.nperf) return;
    double L[9];
    ref_L<S>(w, nbp, lr.perf_row[j], pscale, L);
    double* p = P + 21 * long(j);
    double m[21];
    for (int q = 0; q < 21; ++q) m[q] = p[q];
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 7; ++k) p[7 * i + k] = L[3 * i] * m[k] + L[3 * i + 1] * m[7 + k] + L[3 * i + 2] * m[14 + k];
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_unit_weights(int nbp, S* __restrict__ w)
{
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nbp) return;
    w[row] = S(1); w[nbp + row] = S(0); w[2 * long(nbp) + row] = S(0);
}

template <class S> void LinSolver::cpr_reference_transform()
{
    SolverWork<S>& w = work<S>();
    const double pscale = 200.0e5;               // 200 * unit::barsa (NewtonIterationBlackoilCPR.cpp:117)
    const int g = grid_for(plan.nb);
    if (!ref_transformed) {
        w.cprw.alloc(3 * size_t(plan.nbp)); w.cprw_orig.alloc(3 * size_t(plan.nbp));
        if (!weights_from_assembly)
            hipLaunchKernelGGL((k_cpr_weights<S>), dim3(g), dim3(kBlock), 0, stream, plan.nb, plan.nbp, dp.slice_ptr.p, dp.rowlen.p, dp.nlower.p,
                               dp.tpos.p, matrix<S>(), w.cprw.p, cpr_weight_mode);
        OPMGPU_HIP(hipMemcpyAsync(w.cprw_orig.p, w.cprw.p, 3 * size_t(plan.nbp) * sizeof(S), hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL((k_ref_transform_rows<S>), dim3(g), dim3(kBlock), 0, stream, plan.nb, plan.nbp, pscale, dp.slice_ptr.p, dp.rowlen.p, (const S*)w.cprw_orig.p,
                           const_cast<S*>(matrix<S>()));
        if (lowrank.nw > 0 && lowrank.P)
            hipLaunchKernelGGL((k_ref_transform_lowrank<S>), dim3(grid_for(lowrank.nperf)), dim3(kBlock), 0, stream, lowrank, plan.nbp, pscale, (const S*)w.cprw_orig.p,
                               const_cast<double*>(lowrank.P));
        // the pressure equation is row 0 of every transformed block: unit weights for the pressure stage (its extraction, restriction and
        // coarse space); the bordered well column is formed from the ORIGINAL weights and carries the pressure row's scaling
        hipLaunchKernelGGL((k_unit_weights<S>), dim3(grid_for(plan.nbp)), dim3(kBlock), 0, stream, plan.nbp, w.cprw.p);
        weights_from_assembly = true;
        now.border_weights = w.cprw_orig.p; now.border_colscale = pscale;
        ref_transformed = true;
        pre_stale = true;
        pilu.stale = true;
    }
    hipLaunchKernelGGL((k_ref_transform_vec<S>), dim3(g), dim3(kBlock), 0, stream, plan.nb, plan.nbp, pscale, (const S*)w.cprw_orig.p, w.b.p);
}

template <class S> void LinSolver::cpr_prepare()
{
    SolverWork<S>& w = work<S>();
    KtScope kts(kt, KT_CPR_SETUP);
    const long ne = plan.nentries;
    if (!w.amg) w.amg.reset(new AmgHierarchy<S>(stream));
    // OPMGPU_AMG_LAG=k (experiment): refresh the pressure hierarchy's numbers only on every k-th matrix
    if (amg_lag > 1 && w.amg->ready() && w.cprw.p && (++amg_age % amg_lag) != 0) return;
    w.cprw.alloc(3 * size_t(plan.nbp));
    // global coarse space: real ranks, or the emulated ones
    // one subdomain (single GPU) is the global constant: the near-null-space vector of a closed, slightly compressible system
    // (wells with a pressure control anchor the level: measured, the constant then costs more than it gains -- so with one
    // subdomain it is used for well-free systems only; coarse_mode 2 forces it, 0 switches the whole coarse space off)
    const bool emulated = !comm && emulate_ranks > 1;
    if (coarse_mode != 0 && !emulated) coarse_domains();
    const int nsub = comm ? comm->num_ranks() * cs_m : (emulate_ranks > 1 ? emulate_ranks : 1);
    const bool single_ok = coarse_mode == 2 || (coarse_single_ok && lowrank.nw == 0);
    coarse_nsub = coarse_mode != 0 && (nsub >= 2 || single_ok) ? nsub : 0;
    if (coarse_nsub > 64) coarse_nsub = 0;        // table sizes of the kernels
    if (ell.inner) coarse_nsub = 0;               // the inner Krylov method of the elliptic part works on A_p itself (rank-local when decomposed)
    if (dist_hierarchy()) coarse_nsub = 0;        // the distributed hierarchy reaches the whole domain itself
    // Scaling of the coarse-grid corrections: 1.9 in general; the correction into level 0 by 2.2 when ONE subdomain carries the coarse
    // space (one GPU, no wells) -- the global constant is then removed exactly for the whole domain and the hierarchy is global:
    // measured +4 % (100^3), +9 % (200^3), +7 % (300^3) throughput, 0 % on the sigma = 2 deck (2.2 on every level: better at 100^3 /
    // 200^3, -15 % at 300^3).  Not with wells (3.7 -> 4.4 iterations on the 5-spot deck) and not decomposed (emulated 8 ranks: 4.8 ->
    // 5.6; real 4 ranks: unchanged).
    // Everywhere else the best factor depends on the deck (round 3, profiles/r03_sweep_headline.log: the 5-spot deck wants 2.2-2.6 under
    // GMRES -- 4.6 -> 3.6 iterations --, the SPE10-like deck and 200^3 want 1.9): the policy below picks between two settings by the
    // iteration counts they produce.
    corr_policy.active = false;
    if (!w.amg->pdamp_user) {
        const bool global_constant = coarse_nsub == 1 && lowrank.nw == 0;
        if (global_constant || !corr_policy.on || corr_policy.external) {
            if (!w.amg->factors_kept) { w.amg->pdamp0 = global_constant ? 2.2 : 1.9; w.amg->pdamp = 1.9; }       // (only until the hierarchy's first application: see amg.hpp)
        } else { w.amg->pdamp0 = w.amg->pdamp = corr_policy.arm[corr_policy.cur]; corr_policy.active = true; }
    }
    if (w.amg->ready() && !emulated) {
        // the usual case: one pass over the matrix does weights + pressure matrix (+ coarse-space row parts)
        const int gp = std::min(grid_for(plan.nbp), kCsRowParts);
        if (coarse_nsub >= 1) {
            coarse_begin<S>();
            auto kern = weights_from_assembly ? k_cpr_rows<S, true, true> : k_cpr_rows<S, true, false>;
            hipLaunchKernelGGL(kern, dim3(gp), dim3(kBlock), 0, stream, plan.nb, plan.nbp, cpr_weight_mode, cs_slots, dp.slice_ptr.p, dp.col.p, dp.rowlen.p,
                               dp.nlower.p, dp.tpos.p, cs_sub.p, comm ? comm->owner_mask() : (const int8_t*)nullptr, matrix<S>(), w.cprw.p,
                               w.amg->levels[0]->val.p, cs_buf.p + size_t(2) * coarse_nsub * coarse_nsub + coarse_nsub, w.csT.p);
        } else {
            auto kern = weights_from_assembly ? k_cpr_rows<S, false, true> : k_cpr_rows<S, false, false>;
            hipLaunchKernelGGL(kern, dim3(gp), dim3(kBlock), 0, stream, plan.nb, plan.nbp, cpr_weight_mode, cs_slots, dp.slice_ptr.p, dp.col.p, dp.rowlen.p,
                               dp.nlower.p, dp.tpos.p, (const int32_t*)nullptr, (const int8_t*)nullptr, matrix<S>(), w.cprw.p,
                               w.amg->levels[0]->val.p, (double*)nullptr, (S*)nullptr);
        }
        // Coarse operators (levels >= 1 and the coarsest inverse, 0.18 of the 0.27 ms set-up) follow the first TWO matrices of a time
        // step (the first update moves the state most; the second solve is also the reference for the guard below): level 0 (weights,
        // A_p, its Jacobi diagonal) is rebuilt for every matrix, the coarse-grid corrections of the Newton iterations 3.. of a step
        // come from the operators of its second matrix.  Measured on both bench decks: same iteration
        // counts even with operators frozen for 20 iterations, -4..7 % time per Newton iteration.  Two guards:
        //  * only with the global coarse space active (it is rebuilt for every matrix and corrects the pressure level / the subdomain
        //    constants exactly): without it -- one GPU with wells -- the hierarchy alone carries the near-null pressure-level mode,
        //    and a lagged one left 5e-6 relative error in that mode at a 1e-12 residual (tests/test_gpu_dist.py, wells case);
        //  * a lagged solve that needs clearly more iterations than the solve on the fresh operators (a step far from equilibrium:
        //    measured 13 instead of 8 iterations over six Newton iterations of such a deck) switches the lag off for the rest of
        //    this time step and the next 8 (bicgstab's epilogue sets lag_block);
        //  * only for the loose reductions of Newton solves (>= 1e-4): at 1e-11 a lagged hierarchy stagnated on a grid with isolated
        //    cells (several near-null modes; tests/test_gpu_fullsize.py, Norne-like); and a lagged solve that fails is repeated once
        //    on fresh operators before the failure is reported (solve(), solve.inl).
        // OPMGPU_AMG_LAG_COARSE: 0 = refresh for every matrix, 1 = this policy (default), k > 1 = every k-th matrix, no guards.
        bool refresh;
        if (coarse_lag == 0) refresh = true;
        else if (coarse_lag > 1) refresh = (coarse_age++ % coarse_lag) == 0;
        else {
            if (new_step_hint) { if (lag_block > 0) --lag_block; step_matrix = 0; } else ++step_matrix;
            refresh = step_matrix <= 1 || coarse_nsub == 0 || lag_block > 0 || !lag_allowed || force_refresh;
        }
        force_refresh = false;
        new_step_hint = false;
        refreshed = refresh;
        if (w.amg->border_nw() > 0)
            hipLaunchKernelGGL((k_cpr_border<S>), dim3(lowrank.nw), dim3(kBlock), 0, stream, lowrank, plan.nbp, now.border_weights ? (const S*)now.border_weights : (const S*)w.cprw.p, w.amg->levels[0]->val.p + w.amg->levels[0]->nentries, now.border_colscale);
        // The factorisation (HBM-bound, 140 us, on its own stream) is needed by the first ILU0 sweep only, i.e. behind the hierarchy set-up
        // AND the first V-cycle.  It starts when the level 0 -> 1 Galerkin sums are done -- the one bandwidth-heavy kernel of the chain,
        // which it would slow from 60 to 100 us -- and runs next to the small levels' sums and the first cycle (latency-bound launches).
        w.amg->galerkin(refresh && !(ell.inner && !ell.use_amg), [&] { if (now.factor_deferred) { now.factor_deferred = false; factor_async<S>(); } });
        if (ell.inner && !ell.use_amg) elliptic_factor<S>();
        if (coarse_nsub >= 1) coarse_setup<S>(true);
        return;
    }
    if (!weights_from_assembly)
        hipLaunchKernelGGL((k_cpr_weights<S>), dim3(grid_for(plan.nb)), dim3(kBlock), 0, stream, plan.nb, plan.nbp, dp.slice_ptr.p, dp.rowlen.p, dp.nlower.p,
                           dp.tpos.p, ((emulate_what & 2) ? pre_matrix<S>() : matrix<S>()), w.cprw.p, cpr_weight_mode);
    if (!w.amg->ready()) {
        // first matrix with this pattern: pressure values to the host, aggregation hierarchy (structure only) built there
        DevArray<S> tmp; tmp.alloc(ne);
        hipLaunchKernelGGL((k_extract_pressure<S>), dim3(grid_for(plan.nbp)), dim3(kBlock), 0, stream, plan.nb, plan.nbp, dp.slice_ptr.p, (const S*)w.cprw.p, ((emulate_what & 2) ? pre_matrix<S>() : matrix<S>()), tmp.p);
        std::vector<S> h(ne);
        tmp.download(h.data(), ne, stream);
        OPMGPU_HIP(hipStreamSynchronize(stream));
        std::vector<double> hd(h.begin(), h.end());
        // wells: the pressure system gets one bordering unknown per well (OPMGPU_CPR_WELL_BORDER=0: the wells stay invisible to the AMG)
        static const bool border_on = env_flag("OPMGPU_CPR_WELL_BORDER", true);
        AmgBorderSpec bs;
        if (border_on && lowrank.nw > 0 && lowrank.Fsave && lowrank.ctrl_row && emulate_ranks <= 1) {
            bs.nw = lowrank.nw; bs.nperf = lowrank.nperf;
            bs.connpos.resize(bs.nw + 1); bs.perf_row.resize(bs.nperf);
            OPMGPU_HIP(hipMemcpyAsync(bs.connpos.data(), lowrank.connpos, (bs.nw + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
            OPMGPU_HIP(hipMemcpyAsync(bs.perf_row.data(), lowrank.perf_row, bs.nperf * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
            DevArray<S> bt; bt.alloc(2 * size_t(bs.nperf) + bs.nw);
            hipLaunchKernelGGL((k_cpr_border<S>), dim3(lowrank.nw), dim3(kBlock), 0, stream, lowrank, plan.nbp, now.border_weights ? (const S*)now.border_weights : (const S*)w.cprw.p, bt.p, now.border_colscale);
            std::vector<S> hb(bt.n);
            bt.download(hb.data(), bt.n, stream);
            OPMGPU_HIP(hipStreamSynchronize(stream));
            bs.bcol.assign(hb.begin(), hb.begin() + bs.nperf); bs.crow.assign(hb.begin() + bs.nperf, hb.begin() + 2 * bs.nperf); bs.dw.assign(hb.begin() + 2 * bs.nperf, hb.end());
            bs.d_connpos = lowrank.connpos; bs.d_perf_row = lowrank.perf_row; bs.d_perf_of_row = lowrank.perf_of_row; bs.d_perf_well = lowrank.perf_well; bs.d_perf_next = lowrank.perf_next;
        }
        w.amg->dcomm = dist_hierarchy() ? comm : nullptr;
        w.amg->setup(plan, dp.slice_ptr.p, dp.col.p, hd, bs.nw > 0 ? &bs : nullptr);
    }
    hipLaunchKernelGGL((k_extract_pressure<S>), dim3(grid_for(plan.nbp)), dim3(kBlock), 0, stream, plan.nb, plan.nbp, dp.slice_ptr.p, (const S*)w.cprw.p, ((emulate_what & 2) ? pre_matrix<S>() : matrix<S>()),
                       w.amg->levels[0]->val.p);
    if (w.amg->border_nw() > 0)
        hipLaunchKernelGGL((k_cpr_border<S>), dim3(lowrank.nw), dim3(kBlock), 0, stream, lowrank, plan.nbp, now.border_weights ? (const S*)now.border_weights : (const S*)w.cprw.p, w.amg->levels[0]->val.p + w.amg->levels[0]->nentries, now.border_colscale);
    w.amg->galerkin();
    if (ell.inner && !ell.use_amg) elliptic_factor<S>();
    new_step_hint = false; refreshed = true;
    if (coarse_nsub >= 1) { coarse_begin<S>(); coarse_setup<S>(false); }
}

void LinSolver::drop_hierarchies() { wd.amg.reset(); wf.amg.reset(); gm_light_for = nullptr; }      // (the wells changed: so did the perforated rows)

void LinSolver::CorrectionPolicy::fail_at_current(int iterations)
{
    avg[cur] = avg[cur] < 0.0 ? 4.0 * std::max(iterations, 1) : 2.0 * avg[cur];
    for (int k = cur; k < kArms; ++k) banned_until[k] = steps + ban;
    step_its = step_solves = 0; step_failed = false;
    cur = 0;
}

void LinSolver::correction_policy_choose()
{
    CorrectionPolicy& P = corr_policy;
    if (!P.on || P.external || !new_step_hint) return;            // the setting changes at time-step boundaries only
    if (P.step_solves >= 2 || P.step_failed) {      // score the step that has just ended
        const double score = (P.step_failed ? 4.0 : 1.0) * double(P.step_its) / double(std::max(P.step_solves, 1));
        P.avg[P.cur] = P.avg[P.cur] < 0.0 ? score : 0.5 * P.avg[P.cur] + 0.5 * score;
        ++P.steps;
        if (P.step_failed && P.cur > 0) for (int k = P.cur; k < P.kArms; ++k) P.banned_until[k] = P.steps + P.ban;
    }
    P.step_its = P.step_solves = 0; P.step_failed = false;
    // best of what was tried and is allowed: a larger factor has to beat a smaller one by the margin
    int best = -1;
    for (int k = 0; k < P.kArms; ++k)
        if (P.allowed(k) && P.avg[k] >= 0.0 && (best < 0 || P.avg[k] < P.margin * P.avg[best])) best = k;
    if (best < 0) {          // nothing scored yet (or everything scored is banned): the base setting, else the largest allowed below it
        int k = P.kBase; while (k > 0 && !P.allowed(k)) --k;
        P.cur = k;
        return;
    }
    int next = best;
    if (best == P.kBase && P.allowed(P.kBase + 1) && P.avg[P.kBase + 1] < 0.0) next = P.kBase + 1;           // the pair of round 3: the larger factor once
    else if (P.avg[best] > P.trouble_its && best > 0 && P.avg[best - 1] < 0.0) next = best - 1;              // many iterations: one arm down, once
    else if (P.steps % P.period == P.period - 1) {                                                            // periodic second look at a neighbour
        if (best == P.kBase + 1) next = P.kBase;
        else if (P.allowed(best + 1)) next = best + 1;
    }
    P.cur = next;
}
void LinSolver::correction_policy_report(int iterations, bool converged)
{
    CorrectionPolicy& P = corr_policy;
    if (!P.on || !P.active) return;
    P.step_its += iterations; ++P.step_solves;
    if (!converged) P.step_failed = true;
}

// M^-1 d = [x_p;0;0] + ILU0^-1 (d - A [x_p;0;0]),  x_p = Vcycle(sum of the equations of d) -- or the inner Krylov solve of elliptic.inl
template <class S> void LinSolver::cpr_apply(const S* d, S* v, double relax, const SolveCtl* ctl, const double* cr_given)
{
    SolverWork<S>& w = work<S>();
    AmgLevel<S>& L0 = *w.amg->levels[0];
    const int g = grid_for(plan.nb);
    const bool coarse = coarse_nsub >= 1;
    const bool emulated = !comm && emulate_ranks > 1;
    // the sum [x_p; 0; 0] + ILU0^-1 z formed inside the sweeps (linsolver.hpp, cpr_cancel_p): a two-level plan, every relaxation factor 1
    const bool cancel = cancel_p_now && plan.nlevels == 2 && relax == 1.0 && ell.relax == 1.0 && fill_level == 0 && !now.point_stage2;
    // the top level's part of the stage-2 residual through the ILU0 factor (linsolver.hpp, cpr_factor_p).  Everything `cancel` asks, each for
    // a reason of this path's own:
    //   cancel_p_now      -- the level-0 rows' backward sweep starts from d, so z on those rows is the forward sweep's input and nothing else,
    //                        and s can stand where it stood; set by a double GMRES solve that is neither mixed, flexible nor verified, on
    //                        plain_setup(): one GPU and no emulated ranks (the ILU0 is of exactly the matrix the residual multiplies, and
    //                        no owner mask or halo phase reaches the residual), no Woodbury correction
    //   two levels        -- every lower entry of a top row lies on level 0, where the forward sweep is the identity: the row reads s itself
    //   relaxation 1      -- s_r enters the sum unscaled; with w != 1 the sweep's input is w z
    //   fill_level 0, no point stage 2 -- D_r = A_rr on level 0 and L_ir = A_ir A_rr^-1: the factor of the matrix's own pattern
    // Perforated rows need no exception: what the device wells add to A itself lies in the diagonal blocks of their cells, which the ILU0
    // factors and the sweep's diagonal term reads like any other; the rest of the wells is the low-rank operator (LowRankOp, applied inside
    // k_spmv), which neither k_cpr_presidual nor the factor ever saw, with the switch on or off.
    const bool factor_p = cancel && cpr_factor_p;
    const bool fused_rsum = coarse && !emulated && g <= kCsRowParts;       // real coarse space: restriction fused into the kernel below
    hipEvent_t kt_a = kt.begin();
    double* const cs_parts = coarse ? cs_buf.p + size_t(2) * coarse_nsub * coarse_nsub + coarse_nsub : nullptr;   // own scratch (the BiCGStab partial arrays are live across an application)
    S* const xw = L0.nw > 0 ? L0.x.p + L0.n : (S*)nullptr;        // the wells' unknowns start from zero (their right-hand side is zero): k_cpr_sum_eqs clears them
    if (!fused_rsum)
        hipLaunchKernelGGL((k_cpr_sum_eqs<S, 0>), dim3(g), dim3(kBlock), 0, stream, plan.nb, plan.nbp, d, (const S*)w.cprw.p, L0.b.p, S(w.amg->omega0()), (const S*)L0.dinv.p, L0.x.p, ctl,
                           (const int8_t*)nullptr, (const int8_t*)nullptr, (double*)nullptr, xw, L0.nw);
    else if (cs_m > 1)
        hipLaunchKernelGGL((k_cpr_sum_eqs<S, 2>), dim3(g), dim3(kBlock), 0, stream, plan.nb, plan.nbp, d, (const S*)w.cprw.p, L0.b.p, S(w.amg->omega0()), (const S*)L0.dinv.p, L0.x.p, ctl,
                           (const int8_t*)nullptr, (const int8_t*)cs_blk.p, cs_parts, xw, L0.nw);
    else
        hipLaunchKernelGGL((k_cpr_sum_eqs<S, 1>), dim3(g), dim3(kBlock), 0, stream, plan.nb, plan.nbp, d, (const S*)w.cprw.p, L0.b.p, S(w.amg->omega0()), (const S*)L0.dinv.p, L0.x.p, ctl,
                           comm ? comm->owner_mask() : (const int8_t*)nullptr, (const int8_t*)nullptr, cs_parts, xw, L0.nw);
    w.amg->factors_kept = true;                // first application of this hierarchy: cpr_prepare leaves its fixed correction factors alone from now on
    if (coarse) {
        const int ns = coarse_nsub;
        double* inv = cs_buf.p + ns * ns; double* cr = inv + ns * ns;
        if (cr_given) cr = const_cast<double*>(cr_given);       // the caller's recurrences hold the all-reduced restriction of d already
        else if (!emulated) {
            const int gp = fused_rsum ? g : std::min(grid_for(plan.nb), kMaxPart);
            double* parts = cs_parts;
            if (cs_m > 1) {
                if (!fused_rsum) hipLaunchKernelGGL((k_cs_rsum_blocks<S>), dim3(gp), dim3(kBlock), 0, stream, plan.nb, (const int8_t*)cs_blk.p, (const S*)L0.b.p, parts, ctl);
                hipLaunchKernelGGL(k_cs_place_cr, dim3(1), dim3(kBlock), 0, stream, gp, (const double*)parts, ns, cs_m, comm ? comm->my_rank() : 0, cr, ctl);
            } else {
                if (!fused_rsum) hipLaunchKernelGGL((k_cs_rsum<S>), dim3(gp), dim3(kBlock), 0, stream, plan.nb, comm ? comm->owner_mask() : (const int8_t*)nullptr, (const S*)L0.b.p, parts, ctl);
                hipLaunchKernelGGL(k_cs_place, dim3(1), dim3(kBlock), 0, stream, gp, (const double*)parts, ns, comm ? comm->my_rank() : 0, cr, ctl);
            }
            if (comm) comm->allreduce_sum(cr, ns, stream);
        } else {
            OPMGPU_HIP(hipMemsetAsync(cr, 0, ns * sizeof(double), stream));
            hipLaunchKernelGGL((k_cs_restrict<S>), dim3(g), dim3(kBlock), 0, stream, plan.nb, cs_sub.p, (const int8_t*)nullptr, (const S*)L0.b.p, cr, ctl);
        }
        if (!emulated)
            hipLaunchKernelGGL((k_cs_correct_fast<S>), dim3(g), dim3(kBlock), 0, stream, plan.nb, plan.nbp, ns, cs_slots, cs_sub.p, (const S*)w.csT.p, (const double*)inv,
                               (const double*)cr, S(w.amg->omega0()), (const S*)L0.dinv.p, L0.b.p, L0.x.p, w.cxc.p, ctl);
        else
            hipLaunchKernelGGL((k_cs_correct<S>), dim3(g), dim3(kBlock), 0, stream, plan.nb, plan.nbp, ns, dp.slice_ptr.p, dp.col.p, dp.rowlen.p, cs_sub.p,
                               (const S*)w.cprw.p, matrix<S>(), (const double*)inv, (const double*)cr, S(w.amg->omega0()), (const S*)L0.dinv.p, L0.b.p, L0.x.p, w.cxc.p, ctl);
    }
    kt.end(KT_CPR_OTHER, kt_a);
    kt_a = kt.begin();
    if (comm && cpr_l0_halo && !ell.inner && w.amg->ndist == 0) {
        S* const hx = w.hx.p; CommBase* const cm = comm; const int nbl = plan.nb; hipStream_t st = stream;
        w.amg->level0_halo = [=](S* x, S* b) {
            OPMGPU_HIP(hipMemcpyAsync(hx, x, size_t(nbl) * sizeof(S), hipMemcpyDeviceToDevice, st));
            halo(cm, hx, st);
            hipLaunchKernelGGL((k_l0_ghosts<S>), dim3(grid_for(nbl)), dim3(kBlock), 0, st, nbl, cm->owner_mask(), (const S*)hx, x, b, ctl);
        };
        w.amg->level0_halo_down = cpr_l0_halo_down;
    } else w.amg->level0_halo = nullptr;
    if (ell.inner) elliptic_solve<S>(); else w.amg->vcycle_graph(ctl, true);
    kt.end(KT_VCYCLE, kt_a);
    kt_a = kt.begin();
    const S* xp = L0.x.p;
    // multi-GPU: the AMG is rank-local (additive Schwarz: ghost rows are identity rows); the owners' x_p is copied to the
    // ghosts before the full-system residual so that stage 2 sees the neighbours' pressure correction on the rows next to the
    // cut.  Costs two halo exchanges per BiCGStab iteration; without it (OPMGPU_CPR_HALO_XP=0) the one-rank self-halo deck,
    // where half of the rows touch the cut, needs 25 % more iterations -- and with the coarse space it is essential: the
    // subdomain constants jump at the cut, and a stage 2 that does not see the jump needs 2.5x the iterations (emulated 8
    // ranks: 4.4 -> 11.5, OPMGPU_EMULATE_WHAT=7).  The exchange runs on the halo stream behind the rows that read no ghost (as in
    // bicgstab's products).
    bool exchange = false;
    if (coarse) {
        hipLaunchKernelGGL((k_cs_add<S>), dim3(g), dim3(kBlock), 0, stream, plan.nb, (const S*)L0.x.p, (const S*)w.cxc.p, w.hx.p, ctl);
        xp = w.hx.p;
        exchange = comm && cpr_halo_xp;
    } else if (comm && cpr_halo_xp) {
        OPMGPU_HIP(hipMemcpyAsync(w.hx.p, L0.x.p, size_t(plan.nb) * sizeof(S), hipMemcpyDeviceToDevice, stream));
        xp = w.hx.p;
        exchange = true;
    }
    const S* amat = (emulate_what & 4) ? pre_matrix<S>() : matrix<S>();
    const int8_t* own = comm ? comm->owner_mask() : (const int8_t*)nullptr;
    const bool overlap = exchange && halo_overlap && halo_stream && light_ok_for == comm && light_ok.n == size_t(plan.nbp);
    auto presidual = [&](int phase) {
        if (factor_p) {          // (plain_setup(): no exchange, phase 0, no owner mask)
            const int n0 = plan.level_ptr[1];
            if (n0 > 0) hipLaunchKernelGGL((k_cpr_presidual_l0<S>), dim3(grid8_for(n0)), dim3(kBlock), 0, stream, xcd_mode(), n0, plan.nbp, dp.slice_ptr.p, dp.col.p,
                                           dp.nlower.p, amat, d, xp, w.z.p, ctl);
            return;
        }
        hipLaunchKernelGGL((k_cpr_presidual<S>), dim3(grid8_for(plan.nb)), dim3(kBlock), 0, stream, xcd_mode(), plan.nb, plan.nbp, dp.slice_ptr.p, dp.col.p, amat, d, xp, w.z.p, own, ctl,
                           phase, phase ? (const int8_t*)light_ok.p : (const int8_t*)nullptr);
    };
    if (overlap) halo_overlapped(*this, w.hx.p, presidual);
    else { if (exchange) halo(comm, w.hx.p, stream); presidual(0); }
    kt.end(KT_CPR_OTHER, kt_a);
    if (now.point_stage2 && sizeof(S) == 8) point_ilu_apply(reinterpret_cast<const double*>(w.z.p), reinterpret_cast<double*>(v), relax);      // the reference's own stage 2 (pointilu.inl)
    else ilu_apply<S>(w.z.p, v, relax, ctl, cancel ? d : (const S*)nullptr, cancel ? xp : (const S*)nullptr, factor_p ? amat : (const S*)nullptr);
    kt_a = kt.begin();
    if (well_woodbury && wb_active && lowrank.nw > 0 && lowrank.P && !comm && wb_buf.p && fill_level == 0)
        hipLaunchKernelGGL((k_wb_apply<S>), dim3(lowrank.nw), dim3(kBlock), 0, stream, lowrank, plan.nbp, (const double*)wb_buf.p,
                           (const double*)(wb_buf.p + size_t(21) * lowrank.nperf), v, ctl);
    if (!cancel) hipLaunchKernelGGL((k_cpr_add_p<S>), dim3(g), dim3(kBlock), 0, stream, plan.nb, xp, v, ctl, S(ell.relax));
    kt.end(KT_CPR_OTHER, kt_a);
}
