// aquifer.hip -- analytic aquifers (AQUFETP: Fetkovich, AQUCT: Carter-Tracy, connected by AQUANCON) as source terms of the water equation.
//
// The reference has no aquifers: the rule is this library's own, stated in include/opmgpu.h at opmgpu_set_aquifers and restated in
// tests/aquifer_reference.py.  Every expression of the rule stands in a block with floating-point contraction off, so a product and the
// sum behind it are two roundings as the header says (the cell evaluator inlined next to them keeps its own arithmetic).
// Four kernels, all tiny next to the assembly and bound by the gathers of the cell evaluator:
//   k_aquifer_scalars    begin of a step, one thread per aquifer: J E and p_a, or P', T_c den and b; a bad den raises the aquifer's status
//   k_aquifer_coeffs     begin of a step, one thread per connection: rho0, p0 of its cell from the resident state, then A_j, B_j
//   k_aquifer_assemble   every assembly of a begun step, one thread per distinct connected cell: its connections in the listing order
//   k_aquifer_rates      commit (and the connections' read-out), one workgroup per aquifer: q_j, qs_j, their sums by a fixed tree
#include "aquifer.hpp"
#include "fluid_eval.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

namespace opmgpu {

__global__ __launch_bounds__(64) void k_aquifer_scalars(int naq, const int32_t* __restrict__ ipar, const double* __restrict__ par, const double* __restrict__ tab,
                                                        int ntab, const double* __restrict__ state, double dt, double* __restrict__ scal, int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= naq) return;
    const double* P = par + AQP_COUNT * a;
    const double We = state[AQT_COUNT * a + AQT_WE], t = state[AQT_COUNT * a + AQT_T];
    double* S = scal + AQS_COUNT * a;
    if (ipar[AQI_COUNT * a + AQI_KIND] == OPMGPU_AQUIFER_FETKOVICH) {
        const double pa = P[AQP_PA0] - We / P[AQP_CTV0];
        const double tau = P[AQP_CTV0] / P[AQP_J];
        const double x = dt / tau;
        const double E = -expm1(-x) / x;
        S[AQS_B] = P[AQP_J] * E; S[AQS_PA] = pa; S[AQS_PP] = 0.0; S[AQS_TDEN] = 0.0;
        status[a] = 0;
        return;
    }
    const int ta = ipar[AQI_COUNT * a + AQI_TAB], n = ipar[AQI_COUNT * a + AQI_NTAB];
    const double *td = tab + ta, *pd = tab + ntab + ta, *sl = tab + 2 * long(ntab) + ta;
    const double Tc = P[AQP_TC];
    const double tD = t / Tc, tDp = (t + dt) / Tc;
    const int i = pvt_seg(td, n, tDp);
    const double Pp = sl[i];
    const double Pv = pd[i] + Pp * (tDp - td[i]);
    const double den = Pv - tD * Pp;
    const double Tden = Tc * den;
    S[AQS_B] = P[AQP_BETA] / Tden; S[AQS_PA] = 0.0; S[AQS_PP] = Pp; S[AQS_TDEN] = Tden;
    status[a] = (den > 0.0 && den <= 1.79e308) ? 0 : 1;       // (NaN compares false)
}

template <int KM>
__global__ __launch_bounds__(kBlock) void k_aquifer_coeffs(int nconn, DevTables T, CellPlanes C, const int32_t* __restrict__ conn_row, const int32_t* __restrict__ conn_aq,
                                                           const double* __restrict__ alpha, const int32_t* __restrict__ ipar, const double* __restrict__ par,
                                                           const double* __restrict__ scal, const double* __restrict__ state, const double* __restrict__ zc,
                                                           double gravity, double* __restrict__ coef)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= nconn) return;
    const int row = conn_row[j], a = conn_aq[j];
    CellEval q;
    eval_row<KM>(T, row, C, q);
    {
#pragma clang fp contract(off)
        const double* P = par + AQP_COUNT * a;
        const double* S = scal + AQS_COUNT * a;
        const double rho0 = q.rho[0].v, p0 = q.pw.v, al = alpha[j];
        const double h = (rho0 * gravity) * (zc[row] - P[AQP_DATUM]);
        double A, B;
        if (ipar[AQI_COUNT * a + AQI_KIND] == OPMGPU_AQUIFER_FETKOVICH) {
            B = al * S[AQS_B];
            A = B * (S[AQS_PA] + h);
        } else {
            const double b = S[AQS_B];
            const double aj = (P[AQP_BETA] * ((P[AQP_PA0] + h) - p0) - state[AQT_COUNT * a + AQT_WE] * S[AQS_PP]) / S[AQS_TDEN];
            B = al * b;
            A = al * (aj + b * p0);
        }
        double* o = coef + long(AQC_COUNT) * j;
        o[AQC_RHO0] = rho0; o[AQC_P0] = p0; o[AQC_A] = A; o[AQC_B] = B;
    }
}

// One thread owns a connected cell: its connections' terms in the listing order, then ONE read-modify-write of the water residual and
// of the three entries of the water row of the diagonal block (MS: the precision being assembled).  No atomics.
template <class MS, int KM>
__device__ __forceinline__ void aquifer_assemble_dev(int ncells, const DevTables& T, const CellPlanes& C, const int32_t* __restrict__ cell_rows,
                                                     const int32_t* __restrict__ cell_ptr, const int32_t* __restrict__ cell_conn, const double* __restrict__ coef,
                                                     const int32_t* __restrict__ slice_ptr, const int16_t* __restrict__ nlower, double s0, double* __restrict__ R,
                                                     MS* __restrict__ Amat)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ncells) return;
    const int row = cell_rows[i];
    CellEval q;
    eval_row<KM>(T, row, C, q);
    {
#pragma clang fp contract(off)
        const V4 bw = q.b[0];
        const double pw = q.pw.v, dpw_w = q.pw.w;          // d pw / d (p, Sw, X) = (1, dpw_w, 0)
        double s = 0.0, d[3] = { 0.0, 0.0, 0.0 };
        for (int k = cell_ptr[i]; k < cell_ptr[i + 1]; ++k) {
            const double* o = coef + long(AQC_COUNT) * cell_conn[k];
            const double B = o[AQC_B];
            const double qj = o[AQC_A] - B * pw;
            const double bB = bw.v * B;
            s += bw.v * qj;
            d[0] += bw.p * qj - bB;
            d[1] += bw.w * qj - bB * dpw_w;
            d[2] += bw.x * qj;
        }
        R[row] -= s;
        MS* dptr = Amat + long(slice_ptr[row >> 6] + nlower[row]) * 576 + (row & 63);
        for (int v = 0; v < 3; ++v) dptr[v * 64] = MS(double(dptr[v * 64]) - s0 * d[v]);
    }
}
template <int KM>
__global__ __launch_bounds__(kBlock) void k_aquifer_assemble_d(int ncells, DevTables T, CellPlanes C, const int32_t* __restrict__ cell_rows, const int32_t* __restrict__ cell_ptr,
                                                               const int32_t* __restrict__ cell_conn, const double* __restrict__ coef, const int32_t* __restrict__ slice_ptr,
                                                               const int16_t* __restrict__ nlower, double s0, double* __restrict__ R, double* __restrict__ Amat)
{
    aquifer_assemble_dev<double, KM>(ncells, T, C, cell_rows, cell_ptr, cell_conn, coef, slice_ptr, nlower, s0, R, Amat);
}
template <int KM>
__global__ __launch_bounds__(kBlock) void k_aquifer_assemble_f(int ncells, DevTables T, CellPlanes C, const int32_t* __restrict__ cell_rows, const int32_t* __restrict__ cell_ptr,
                                                               const int32_t* __restrict__ cell_conn, const double* __restrict__ coef, const int32_t* __restrict__ slice_ptr,
                                                               const int16_t* __restrict__ nlower, double s0, double* __restrict__ R, float* __restrict__ Amat)
{
    aquifer_assemble_dev<float, KM>(ncells, T, C, cell_rows, cell_ptr, cell_conn, coef, slice_ptr, nlower, s0, R, Amat);
}

// One workgroup per aquifer.  Thread T takes the aquifer's connections T, T + 256, ... in ascending order; the sums Q = sum q_j and
// Qs = sum b_w q_j then go through the wave's shuffle tree (wave_sum: offsets 32 .. 1) and the four waves are added in order -- the tree
// the header documents.  apply: W_e += dt Q, W_s += dt Qs, t += dt (the commit); without it only q_j, qs_j are written (the read-out).
template <int KM>
__global__ __launch_bounds__(kBlock) void k_aquifer_rates(DevTables T, CellPlanes C, const int32_t* __restrict__ conn_ptr, const int32_t* __restrict__ conn_row,
                                                          const double* __restrict__ coef, double* __restrict__ qout, double dt, int apply, double* __restrict__ state)
{
    __shared__ double sm[8];
    const int a = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j1 = conn_ptr[a + 1];
    double Q = 0.0, Qs = 0.0;
    for (int j = conn_ptr[a] + threadIdx.x; j < j1; j += kBlock) {
        CellEval q;
        eval_row<KM>(T, conn_row[j], C, q);
        {
#pragma clang fp contract(off)
            const double* o = coef + long(AQC_COUNT) * j;
            const double qj = o[AQC_A] - o[AQC_B] * q.pw.v;
            const double qs = q.b[0].v * qj;
            Q += qj; Qs += qs;
            qout[2 * long(j)] = qj; qout[2 * long(j) + 1] = qs;
        }
    }
    Q = wave_sum(Q); Qs = wave_sum(Qs);
    if (lane == 0) { sm[w] = Q; sm[4 + w] = Qs; }
    __syncthreads();
    if (threadIdx.x == 0 && apply) {
#pragma clang fp contract(off)
        const double Qt = ((sm[0] + sm[1]) + sm[2]) + sm[3], Qst = ((sm[4] + sm[5]) + sm[6]) + sm[7];
        double* S = state + AQT_COUNT * a;
        S[AQT_WE] = S[AQT_WE] + dt * Qt;
        S[AQT_WS] = S[AQT_WS] + dt * Qst;
        S[AQT_T] = S[AQT_T] + dt;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
void BlackoilDevice::aquifer_free() { delete aq; aq = nullptr; }
bool BlackoilDevice::has_aquifers() const { return aq != nullptr; }
void BlackoilDevice::aquifer_discard() { if (aq) aq->begun = false; }
int BlackoilDevice::aquifer_rows(const int32_t** rows) const
{
    if (!aq || !aq->begun) return 0;
    *rows = aq->cell_rows.p;
    return aq->ncells;
}

void BlackoilDevice::set_aquifers(const opmgpu_aquifers* s)
{
    const std::string who = "opmgpu_set_aquifers: ";
    auto bad = [&](const std::string& m) { throw HipError(OPMGPU_EINVAL, who + m); };
    if (!s || s->naq == 0) {
        if (aq) { OPMGPU_HIP(hipStreamSynchronize(stream)); aquifer_free(); }
        return;
    }
    if (s->naq < 0) bad("naq is negative");
    if (ls.comm) bad("a communicator is attached; a decomposed run does not support aquifers");
    if (!s->kind || !s->p_a0 || !s->datum || !s->CtV0 || !s->J || !s->beta || !s->Tc || !s->conn_ptr || !s->conn_cell || !s->conn_alpha) bad("a required array is NULL");
    const int naq = s->naq;
    auto finite = [](double v) { return std::isfinite(v); };
    auto positive = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (s->conn_ptr[0] != 0) bad("conn_ptr[0] is not 0");
    std::vector<int32_t> seen(nc, -1), tab_ptr(naq + 1, 0);
    for (int a = 0; a < naq; ++a) {
        const std::string an = "aquifer " + std::to_string(a) + ": ";
        const bool fet = s->kind[a] == OPMGPU_AQUIFER_FETKOVICH;
        if (!fet && s->kind[a] != OPMGPU_AQUIFER_CARTER_TRACY) bad(an + "unknown kind");
        if (!finite(s->p_a0[a])) bad(an + "p_a0 is not finite");
        if (!finite(s->datum[a])) bad(an + "the datum depth is not finite");
        if (fet) {
            if (!positive(s->CtV0[a])) bad(an + "CtV0 is not finite and positive");
            if (!positive(s->J[a])) bad(an + "J is not finite and positive");
        } else {
            if (!positive(s->beta[a])) bad(an + "beta is not finite and positive");
            if (!positive(s->Tc[a])) bad(an + "Tc is not finite and positive");
            if (!s->tab_ptr || !s->tab_td || !s->tab_pd) bad(an + "a Carter-Tracy aquifer needs the influence table (tab_ptr, tab_td, tab_pd)");
        }
        if (s->tab_ptr) {
            if (a == 0 && s->tab_ptr[0] != 0) bad("tab_ptr[0] is not 0");
            const int t0 = s->tab_ptr[a], t1 = s->tab_ptr[a + 1];
            if (t1 < t0) bad(an + "tab_ptr decreases");
            tab_ptr[a + 1] = t1;
            if (!fet) {
                if (t1 - t0 < 2) bad(an + "the influence table has fewer than 2 rows");
                for (int k = t0; k < t1; ++k) {
                    if (!finite(s->tab_td[k]) || !finite(s->tab_pd[k])) bad(an + "the influence table has a non-finite entry");
                    if (k > t0 && !(s->tab_td[k] > s->tab_td[k - 1])) bad(an + "t_D of the influence table is not strictly increasing");
                }
            }
        }
        const int j0 = s->conn_ptr[a], j1 = s->conn_ptr[a + 1];
        if (j1 <= j0) bad(an + "no connections");
        double sum = 0.0;
        for (int j = j0; j < j1; ++j) {
            const int c = s->conn_cell[j];
            if (c < 0 || c >= nc) bad(an + "connection " + std::to_string(j - j0) + ": cell " + std::to_string(c) + " is out of range");
            if (seen[c] == a) bad(an + "cell " + std::to_string(c) + " is connected twice (merge the faces of a cell into one connection)");
            seen[c] = a;
            if (!positive(s->conn_alpha[j])) bad(an + "connection " + std::to_string(j - j0) + ": alpha is not finite and positive");
            sum += s->conn_alpha[j];
        }
        if (!(std::fabs(sum - 1.0) <= 1e-12)) bad(an + "the alphas do not sum to 1 within 1e-12");
    }
    // accepted: the new set replaces the old one and starts with W_e = W_s = t = 0
    OPMGPU_HIP(hipStreamSynchronize(stream));
    aquifer_free();
    aq = new AquiferDev();
    AquiferDev& Q = *aq;
    Q.naq = naq; Q.nconn = s->conn_ptr[naq]; Q.ntab = tab_ptr[naq];
    Q.kind.assign(s->kind, s->kind + naq);
    Q.pa0.assign(s->p_a0, s->p_a0 + naq); Q.datum.assign(s->datum, s->datum + naq); Q.CtV0.assign(s->CtV0, s->CtV0 + naq); Q.J.assign(s->J, s->J + naq);
    Q.beta.assign(s->beta, s->beta + naq); Q.Tc.assign(s->Tc, s->Tc + naq);
    Q.tab_ptr = tab_ptr;
    if (Q.ntab > 0) { Q.tab_td.assign(s->tab_td, s->tab_td + Q.ntab); Q.tab_pd.assign(s->tab_pd, s->tab_pd + Q.ntab); }
    Q.conn_ptr.assign(s->conn_ptr, s->conn_ptr + naq + 1);
    Q.conn_cell.assign(s->conn_cell, s->conn_cell + Q.nconn);
    Q.conn_alpha.assign(s->conn_alpha, s->conn_alpha + Q.nconn);
    std::vector<double> par(size_t(AQP_COUNT) * naq), st(size_t(AQT_COUNT) * naq, 0.0), tab(3 * size_t(std::max(Q.ntab, 1)), 0.0);
    std::vector<int32_t> ipar(size_t(AQI_COUNT) * naq), caq(Q.nconn);
    for (int a = 0; a < naq; ++a) {
        double* P = &par[size_t(AQP_COUNT) * a];
        const bool fet = Q.kind[a] == OPMGPU_AQUIFER_FETKOVICH;
        // (the other model's parameters are not read: ones, so that nothing non-finite rides along)
        P[AQP_PA0] = Q.pa0[a]; P[AQP_DATUM] = Q.datum[a]; P[AQP_CTV0] = fet ? Q.CtV0[a] : 1.0; P[AQP_J] = fet ? Q.J[a] : 1.0;
        P[AQP_BETA] = fet ? 1.0 : Q.beta[a]; P[AQP_TC] = fet ? 1.0 : Q.Tc[a];
        ipar[AQI_COUNT * a + AQI_KIND] = Q.kind[a]; ipar[AQI_COUNT * a + AQI_TAB] = tab_ptr[a]; ipar[AQI_COUNT * a + AQI_NTAB] = fet ? 0 : tab_ptr[a + 1] - tab_ptr[a];
        for (int j = Q.conn_ptr[a]; j < Q.conn_ptr[a + 1]; ++j) caq[j] = a;
        if (!fet)
            for (int k = tab_ptr[a]; k < tab_ptr[a + 1]; ++k) {
                tab[k] = Q.tab_td[k]; tab[size_t(Q.ntab) + k] = Q.tab_pd[k];
                if (k + 1 < tab_ptr[a + 1]) tab[2 * size_t(Q.ntab) + k] = (Q.tab_pd[k + 1] - Q.tab_pd[k]) / (Q.tab_td[k + 1] - Q.tab_td[k]);
            }
    }
    Q.par.upload(par, stream); Q.ipar.upload(ipar, stream); Q.tab.upload(tab, stream); Q.state.upload(st, stream);
    Q.scal.alloc(size_t(AQS_COUNT) * naq); Q.scal.zero(stream);
    Q.status.alloc(naq); Q.status.zero(stream);
    Q.alpha.upload(Q.conn_alpha, stream); Q.d_conn_ptr.upload(Q.conn_ptr, stream); Q.conn_aq.upload(caq, stream);
    Q.coef.alloc(size_t(AQC_COUNT) * Q.nconn); Q.coef.zero(stream);
    Q.qout.alloc(2 * size_t(Q.nconn)); Q.qout.zero(stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));        // the host vectors above go out of scope
    aquifer_rebind();
}

// the row-indexed maps of the current plan (after set_aquifers and after every re-plan); a begun step does not survive it
void BlackoilDevice::aquifer_rebind()
{
    if (!aq) return;
    AquiferDev& Q = *aq;
    const Plan& P = ls.plan;
    Q.begun = false;
    std::vector<int32_t> rows(Q.nconn);
    for (int j = 0; j < Q.nconn; ++j) rows[j] = P.pos[Q.conn_cell[j]];
    // distinct rows in the order of their first connection, each with its connections in ascending (listing) order
    std::vector<int32_t> slot_of_row(P.nbp, -1), cell_rows, count;
    for (int j = 0; j < Q.nconn; ++j) {
        int& sl = slot_of_row[rows[j]];
        if (sl < 0) { sl = int(cell_rows.size()); cell_rows.push_back(rows[j]); count.push_back(0); }
        ++count[sl];
    }
    Q.ncells = int(cell_rows.size());
    std::vector<int32_t> ptr(Q.ncells + 1, 0), fill(Q.ncells, 0), conn(Q.nconn);
    for (int i = 0; i < Q.ncells; ++i) ptr[i + 1] = ptr[i] + count[i];
    for (int j = 0; j < Q.nconn; ++j) { const int sl = slot_of_row[rows[j]]; conn[ptr[sl] + fill[sl]++] = j; }
    Q.conn_row.upload(rows, stream); Q.cell_rows.upload(cell_rows, stream); Q.cell_ptr.upload(ptr, stream); Q.cell_conn.upload(conn, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

void BlackoilDevice::aquifer_begin_step(double dt)
{
    const std::string who = "opmgpu_aquifer_begin_step: ";
    if (!aq) throw HipError(OPMGPU_EINVAL, who + "no aquifers are set (opmgpu_set_aquifers)");
    if (!(dt > 0.0) || std::isinf(dt)) throw HipError(OPMGPU_EINVAL, who + "dt is not positive and finite");
    if (!has_state) throw HipError(OPMGPU_EINVAL, who + "no state is resident (opmgpu_set_state)");
    AquiferDev& Q = *aq;
    Q.begun = false;            // a begun step that was not committed is discarded
    hipLaunchKernelGGL(k_aquifer_scalars, dim3(grid_for(Q.naq, 64)), dim3(64), 0, stream, Q.naq, (const int32_t*)Q.ipar.p, (const double*)Q.par.p, (const double*)Q.tab.p,
                       Q.ntab, (const double*)Q.state.p, dt, Q.scal.p, Q.status.p);
    hipLaunchKernelGGL(OPMGPU_BY_MODEL(k_aquifer_coeffs), dim3(grid_for(Q.nconn)), dim3(kBlock), 0, stream, Q.nconn, dtp_, cell_planes(), (const int32_t*)Q.conn_row.p,
                       (const int32_t*)Q.conn_aq.p, (const double*)Q.alpha.p, (const int32_t*)Q.ipar.p, (const double*)Q.par.p, (const double*)Q.scal.p,
                       (const double*)Q.state.p, (const double*)d_zc.p, gravity, Q.coef.p);
    std::vector<int32_t> status(Q.naq);
    Q.status.download(status.data(), size_t(Q.naq), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    for (int a = 0; a < Q.naq; ++a)
        if (status[a] != 0)
            throw HipError(OPMGPU_ENUMERICAL, who + "aquifer " + std::to_string(a) + ": den = P - t_D P' of the Carter-Tracy influence table is not positive and finite; no step is begun");
    Q.begun = true; Q.dt = dt;
}

void BlackoilDevice::aquifer_assemble()
{
    if (!aq || !aq->begun) return;
    AquiferDev& Q = *aq;
    const double s0 = prm.matbalscale[0];
    if (ls.matrix_is_float) {
        hipLaunchKernelGGL(OPMGPU_BY_MODEL(k_aquifer_assemble_f), dim3(grid_for(Q.ncells)), dim3(kBlock), 0, stream, Q.ncells, dtp_, cell_planes(), (const int32_t*)Q.cell_rows.p,
                           (const int32_t*)Q.cell_ptr.p, (const int32_t*)Q.cell_conn.p, (const double*)Q.coef.p, ls.dp.slice_ptr.p, ls.dp.nlower.p, s0, d_R.p, ls.matrix_f());
        ls.cpr_reweigh_rows<float>(Q.cell_rows.p, Q.ncells);
    } else {
        hipLaunchKernelGGL(OPMGPU_BY_MODEL(k_aquifer_assemble_d), dim3(grid_for(Q.ncells)), dim3(kBlock), 0, stream, Q.ncells, dtp_, cell_planes(), (const int32_t*)Q.cell_rows.p,
                           (const int32_t*)Q.cell_ptr.p, (const int32_t*)Q.cell_conn.p, (const double*)Q.coef.p, ls.dp.slice_ptr.p, ls.dp.nlower.p, s0, d_R.p, ls.matrix_d());
        ls.cpr_reweigh_rows<double>(Q.cell_rows.p, Q.ncells);
    }
}

void BlackoilDevice::aquifer_launch_rates(int apply)
{
    AquiferDev& Q = *aq;
    hipLaunchKernelGGL(OPMGPU_BY_MODEL(k_aquifer_rates), dim3(Q.naq), dim3(kBlock), 0, stream, dtp_, cell_planes(), (const int32_t*)Q.d_conn_ptr.p, (const int32_t*)Q.conn_row.p,
                       (const double*)Q.coef.p, Q.qout.p, Q.dt, apply, Q.state.p);
}
void BlackoilDevice::aquifer_commit_step()
{
    if (!aq || !aq->begun) throw HipError(OPMGPU_EINVAL, "opmgpu_aquifer_commit_step: no step has begun (opmgpu_aquifer_begin_step)");
    aquifer_launch_rates(1);
    aq->begun = false;
}

void BlackoilDevice::aquifer_state_get(double* We, double* Ws, double* t, double* pa)
{
    if (!aq) throw HipError(OPMGPU_EINVAL, "opmgpu_aquifer_state_get: no aquifers are set (opmgpu_set_aquifers)");
    AquiferDev& Q = *aq;
    std::vector<double> st(size_t(AQT_COUNT) * Q.naq);
    Q.state.download(st.data(), st.size(), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    for (int a = 0; a < Q.naq; ++a) {
        const double* S = &st[size_t(AQT_COUNT) * a];
        if (We) We[a] = S[AQT_WE];
        if (Ws) Ws[a] = S[AQT_WS];
        if (t) t[a] = S[AQT_T];
        if (pa) pa[a] = Q.pa0[a] - S[AQT_WE] / (Q.kind[a] == OPMGPU_AQUIFER_FETKOVICH ? Q.CtV0[a] : Q.beta[a]);
    }
}
void BlackoilDevice::aquifer_state_set(const double* We, const double* Ws, const double* t)
{
    const std::string who = "opmgpu_aquifer_state_set: ";
    if (!aq) throw HipError(OPMGPU_EINVAL, who + "no aquifers are set (opmgpu_set_aquifers)");
    AquiferDev& Q = *aq;
    const double* src[3] = { We, Ws, t };
    for (int k = 0; k < 3; ++k)
        for (int a = 0; src[k] && a < Q.naq; ++a) if (!std::isfinite(src[k][a])) throw HipError(OPMGPU_EINVAL, who + "a value is not finite");
    if (t) for (int a = 0; a < Q.naq; ++a) if (t[a] < 0.0) throw HipError(OPMGPU_EINVAL, who + "an aquifer time is negative");
    std::vector<double> st(size_t(AQT_COUNT) * Q.naq);
    Q.state.download(st.data(), st.size(), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    for (int k = 0; k < 3; ++k)
        for (int a = 0; src[k] && a < Q.naq; ++a) st[size_t(AQT_COUNT) * a + k] = src[k][a];
    Q.state.upload(st, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    Q.begun = false;
}
void BlackoilDevice::aquifer_connections_get(double* out)
{
    if (!aq || !aq->begun) throw HipError(OPMGPU_EINVAL, "opmgpu_aquifer_connections_get: no step has begun (opmgpu_aquifer_begin_step)");
    AquiferDev& Q = *aq;
    aquifer_launch_rates(0);
    std::vector<double> c(size_t(AQC_COUNT) * Q.nconn), r(2 * size_t(Q.nconn));
    Q.coef.download(c.data(), c.size(), stream); Q.qout.download(r.data(), r.size(), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    for (int j = 0; j < Q.nconn; ++j) {
        double* o = out + size_t(OPMGPU_AQUIFER_CONN_K) * j;
        for (int k = 0; k < AQC_COUNT; ++k) o[k] = c[size_t(AQC_COUNT) * j + k];
        o[4] = r[2 * size_t(j)]; o[5] = r[2 * size_t(j) + 1];
    }
}
int BlackoilDevice::aquifer_counts(int* nconn) const { if (nconn) *nconn = aq ? aq->nconn : 0; return aq ? aq->naq : 0; }

} // namespace opmgpu
