// blackoil.hip -- the Newton path of the black-oil model (see blackoil.hpp): the gfx950 kernels every iteration runs and the host
// methods that launch them -- assembly, convergence, right-hand side, update, the well-term and perforation kernels the well models call
// per iteration, the hysteresis history -- with the constructor, the state set / get / save / restore and attach_comm.  The fluid
// evaluators are fluid_eval.hpp; the host-only set-up (tables, re-planning, end-point planes) is blackoil_setup.inl, included below;
// whatever runs once per run or per report step is blackoil_output.hip.
// Two kernels per assembly (k_cell_values, k_assemble_rows; described where they stand), both one-thread-per-cell over the solver's
// internal (level-major) numbering so that every per-cell plane access of a wavefront is one contiguous segment.  Algorithmic HBM bytes
// per cell are given in DESIGN.md; the Jacobian write dominates.
#include "fluid_eval.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <type_traits>

namespace opmgpu {

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// What a row needs of its NEIGHBOURS are ten VALUES per cell -- the phase pressures p_w and p_g (p_o is the state's pressure), the three
// densities, the three b * mobility products, rs and rv -- and nothing else: a row computes the derivatives of each of its connections'
// fluxes with respect to its OWN variables only, from the derivatives eval_cell gives it for its own cell, and writes them twice -- into
// its own diagonal block, and (negated) into the block (neighbour, row) of the NEIGHBOUR's matrix row, which is exactly that entry:
// dR_j / d x_i = -(dR_i / d x_i)|this connection.  Every block is still written by exactly one thread and every residual entry by its own
// row (no atomics), but the 27 derivative planes round 2 exchanged between its two kernels (written once, read ~2.8 times: 1.37 GB of
// HBM traffic for 0.41 GB of algorithmic bytes at 100^3, PMC in profiles/r02_w_pmc_summary.json) no longer exist.
//   k_cell_values : state -> the ten value planes (+ 1 / b for getConvergence)                                  [pass 1, all cells]
//   k_assemble_rows: state -> own derivatives (eval_cell again: arithmetic is free next to the bytes), accumulation term, TPFA fluxes
//                    from the neighbours' value planes, residual, diagonal block, transposed off-diagonal blocks, CPR weights  [pass 2]
template <bool LDS, int KM>
__global__ __launch_bounds__(kBlock) void k_cell_values(int nb, int nbp, DevTables D, const int32_t* __restrict__ pvtnum, const int32_t* __restrict__ satnum,
                                                        const double* __restrict__ p, const double* __restrict__ sw, const double* __restrict__ sg,
                                                        const double* __restrict__ rs, const double* __restrict__ rv, const int8_t* __restrict__ hc,
                                                        const double* __restrict__ eps, const double* __restrict__ eps_u0, const double* __restrict__ somax,
                                                        double* __restrict__ vals, double* __restrict__ bpart, const int8_t* __restrict__ mask,
                                                        const double* __restrict__ tab_blob, int tab_words, HystArgs hy)
{
    extern __shared__ double tab_lds[];
    __shared__ double bsm[12];
    resolve_tables<LDS>(D, tab_blob, tab_words, tab_lds);
    const int row = blockIdx.x * kBlock + threadIdx.x;
    double ib[3] = { 0.0, 0.0, 0.0 };
    if (row < nb) {
        CellEval q;
        EpsD E, EI;
        HystD H;
        eps_load(eps, eps_u0, nbp, row, satnum[row], E);
        hyst_load<KM>(hy.imbnum, hy.hist, nbp, row, H);
        if (H.on) eps_load(hy.ieps, hy.iureg, nbp, row, H.ireg, EI);
        eval_cell<false, KM>(D, E, (D.t.vap1 > 0.0 || D.t.vap2 > 0.0) ? somax[row] : 0.0, pvtnum[row], satnum[row], p[row], sw[row], sg[row], rs[row], rv[row], hc[row], row, q, H, &EI, nullptr,
                             rs_cap_of<KM>(somax, nbp, row), rv_cap_of<KM>(somax, nbp, row), rocknum_of<KM>(satnum, nbp, row), rock_pmin_of<KM>(somax, nbp, row));
        // (no gas phase: the five water / oil planes only -- nobody reads the other five --, and 1 / b_g = 1 per cell)
        constexpr int NP = km_model(KM) == KM_OW ? 2 : 3;
        vals[long(VP_PW) * nbp + row] = q.pw.v; if constexpr (NP == 3) vals[long(VP_PG) * nbp + row] = q.pg.v;
        const bool owned = !mask || mask[row];
#pragma unroll
        for (int a = 0; a < NP; ++a) {
            vals[long(VP_RHO + a) * nbp + row] = q.rho[a].v;
            vals[long(VP_U + a) * nbp + row] = q.b[a].v * q.mob[a].v;
            if (owned) ib[a] = 1.0 / q.b[a].v;
        }
        if constexpr (NP == 3) { vals[long(VP_RS) * nbp + row] = q.rs.v; vals[long(VP_RV) * nbp + row] = q.rv.v; }
        else if (owned) ib[2] = 1.0;
    }
    // getConvergence needs only the SUMS of 1 / b_a over the owned cells (B_avg, BlackoilModelBase_impl.hpp:1650-1660): one partial per
    // workgroup here instead of three planes written now and read back by k_conv_partial (48 MB of traffic at 100^3)
    block_sum<3>(ib, bsm);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) bpart[long(a) * gridDim.x + blockIdx.x] = ib[a];
    }
}

// computeAccum / assembleMassBalanceEq / computeMassFlux / applyThresholdPressures / UpwindSelector (BlackoilModelBase_impl.hpp:709-751, 845-913,
// 1484-1545, AutoDiffHelpers.hpp:204-221; rs / rv cross terms :889-906, div = ngrad^T), one thread per row.
// Per SELL entry of a row: the neighbour's row (col), the connection's transmissibility with the row's SIDE of the connection in its sign
// bit (+: the row is c1, ngrad coefficient +1; NaN: not a connection -- the fill of an explicit well clique), g (z_c1 - z_c2), the
// threshold pressure, and the index of the transposed entry (tpos).  All four are read coalesced at known addresses: the only dependent
// loads of the loop are the neighbour's values.
// Shapes: MS the Jacobian's precision, LDS the tables staged in LDS (the blob fits), DUAL a float copy of a double Jacobian written in the
// same pass, KM the model.  Compiled for 3 waves per SIMD in the default model's plain LDS shape and for 2 everywhere else
// (asm_rows_waves; the two concluded experiments behind that are quoted at assemble_kernels).
constexpr int asm_rows_waves(bool lds, bool dual, int km) { return km == KM_DEFAULT && lds && !dual ? 3 : 2; }      // (the KM_DRDT and KM_ROCK shapes were never tuned: 2)
template <class MS, bool LDS, bool DUAL, int KM>
__global__ __launch_bounds__(kBlock, asm_rows_waves(LDS, DUAL, KM)) void k_assemble_rows(int xm, int nb, int nbp, DevTables DT, const int32_t* __restrict__ pvtnum, const int32_t* __restrict__ satnum,
                                                          const double* __restrict__ pv, const double* __restrict__ p, const double* __restrict__ sw,
                                                          const double* __restrict__ sg, const double* __restrict__ rs, const double* __restrict__ rv,
                                                          const int8_t* __restrict__ hc, double inv_dt, int initial, double s0, double s1, double s2,
                                                          const int32_t* __restrict__ slice_ptr, const int32_t* __restrict__ col, const int16_t* __restrict__ rowlen,
                                                          const int16_t* __restrict__ nlower, const int32_t* __restrict__ tpos,
                                                          const double* __restrict__ tr_e, const double* __restrict__ zc, double grav, const double* __restrict__ thp_e,
                                                          const double* __restrict__ eps, const double* __restrict__ eps_u0, const double* __restrict__ somax,
                                                          const double* __restrict__ vals, double* __restrict__ accum0, const int8_t* __restrict__ mask,
                                                          double* __restrict__ R, MS* __restrict__ A, MS* __restrict__ wout, const int32_t* __restrict__ chunk_perm,
                                                          const double* __restrict__ tab_blob, int tab_words, HystArgs hy, float* __restrict__ A32)
{
    // A32 != nullptr (mixed precision, opmgpu_params.preconditioner_single): every block is ALSO written as float into the preconditioner's
    // copy of the matrix -- 250 MB more written here instead of a conversion pass that reads 500 MB and writes 250 MB before the solve
    extern __shared__ double tab_lds[];
    constexpr bool BATCH = LDS;          // all ten neighbour values in one batch wherever the tables are in LDS (see the loop)
    const int nchunks = (nb + kBlock - 1) / kBlock;
    const int lch = xcd_first(nchunks, xm);
    if (lch >= xcd_end(nchunks, xm)) return;               // (uniform over the workgroup)
    resolve_tables<LDS>(DT, tab_blob, tab_words, tab_lds);
    const int ch = chunk_perm[lch];
    const int row = ch * kBlock + threadIdx.x;
    if (row >= nb) return;
    const int base = slice_ptr[row >> 6], lane = row & 63, nl = nlower[row], len = rowlen[row];
    const bool ghost = mask && !mask[row];                 // multi-GPU: a ghost row is an identity row with zero residual -- the owner rank
                                                           // assembles the real equation; its thread still writes the blocks (owned row, ghost column)
    // ---- the row's own cell: values from the planes (bit for bit what the neighbours read), derivatives from eval_cell ----
    CellEval q;
    {
        EpsD E, EI;
        HystD H;
        eps_load(eps, eps_u0, nbp, row, satnum[row], E);
        hyst_load<KM>(hy.imbnum, hy.hist, nbp, row, H);
        if (H.on) eps_load(hy.ieps, hy.iureg, nbp, row, H.ireg, EI);
        eval_cell<false, KM>(DT, E, (DT.t.vap1 > 0.0 || DT.t.vap2 > 0.0) ? somax[row] : 0.0, pvtnum[row], satnum[row], p[row], sw[row], sg[row], rs[row], rv[row], hc[row], row, q, H, &EI, nullptr,
                             rs_cap_of<KM>(somax, nbp, row), rv_cap_of<KM>(somax, nbp, row), rocknum_of<KM>(satnum, nbp, row), rock_pmin_of<KM>(somax, nbp, row));
    }
    // NP == 2, a deck without a gas phase (KM_OW): only water and oil flow.  Neither the own nor the neighbour's p_g, gas density, gas
    // b * mobility, rs and rv planes are loaded (5 of the 10 dependent loads per connection), the gas equation is the identity row and
    // the third column of every block is zero (see the end of the loop and of the kernel)
    constexpr int NP = km_model(KM) == KM_OW ? 2 : 3;
    const double scale[3] = { s0, s1, s2 };
    double op[3], orho[3], oU[3];                          // own values
    double dP[3][3], dRho[3][3], dU[3][3];                 // own derivatives d/d(P, Sw, Xvar) of phase pressure, density, b * mobility
    // (the row's own VALUES are read from the planes pass 1 wrote -- bit for bit what the neighbours see of this cell.  Taking them from this
    // kernel's own eval_cell instead saves 80 B per cell and was measured SLOWER, 0.239 against 0.202 ms: the values then stay live in
    // registers across the whole evaluation and the loop spills more; profiles/r03_asm_ownvals_ab.log)
    op[0] = vals[long(VP_PW) * nbp + row]; op[1] = p[row]; if constexpr (NP == 3) op[2] = vals[long(VP_PG) * nbp + row];
    dP[0][0] = 1.0; dP[0][1] = q.pw.w; dP[0][2] = 0.0;
    dP[1][0] = 1.0; dP[1][1] = 0.0; dP[1][2] = 0.0;
    dP[2][0] = 1.0; dP[2][1] = q.pg.w; dP[2][2] = q.pg.x;
#pragma unroll
    for (int a = 0; a < NP; ++a) {
        orho[a] = vals[long(VP_RHO + a) * nbp + row]; oU[a] = vals[long(VP_U + a) * nbp + row];
        const V4 u = vmul(q.b[a], q.mob[a]);
        dRho[a][0] = q.rho[a].p; dRho[a][1] = q.rho[a].w; dRho[a][2] = q.rho[a].x;
        dU[a][0] = u.p; dU[a][1] = u.w; dU[a][2] = u.x;
    }
    double oRs = 0.0, oRv = 0.0;
    if constexpr (NP == 3) { oRs = vals[long(VP_RS) * nbp + row]; oRv = vals[long(VP_RV) * nbp + row]; }
    const double dRs[3] = { q.rs.p, q.rs.w, q.rs.x }, dRv[3] = { q.rv.p, q.rv.w, q.rv.x };
    // ---- accumulation term pvdt * (accum1 - accum0) and its part of the diagonal block ----
    const double pvdt = pv[row] * inv_dt;
    double Rl[3], D[9];
#pragma unroll
    for (int a = 0; a < NP; ++a) {
        if (initial) accum0[long(a) * nbp + row] = q.accum[a].v;
        const double a0 = initial ? q.accum[a].v : accum0[long(a) * nbp + row];
        Rl[a] = pvdt * (q.accum[a].v - a0);
        D[3 * a] = scale[a] * pvdt * q.accum[a].p; D[3 * a + 1] = scale[a] * pvdt * q.accum[a].w; D[3 * a + 2] = scale[a] * pvdt * q.accum[a].x;
    }
    // CPR weights (formEllipticSystem, see k_cpr_weights): column sums of |dR_j[eq]/dp_i| over the rows j != i -- the blocks (j, i) this
    // row writes itself, so the sums come for free (systems without explicit well cliques; k_cpr_weights stays for everything else)
    double sod[3] = { 0.0, 0.0, 0.0 };
    int k0 = (nl == 0) ? 1 : 0;
    // per entry: the neighbour (4 B), the transmissibility with the side in its sign bit (8 B), the index of the transposed entry (4 B; as a
    // one-byte slot of the neighbour's row it was measured slower: one more dependent load per connection, 0.240 against 0.210 ms), the
    // threshold pressure where the deck has one.  g (z_c1 - z_c2) is formed from the depth plane: the neighbour's depth rides on the gather
    // of its values (round 3 kept a per-entry word for it: 55 MB at 100^3 against ~16 MB now; 0.210 against 0.245 ms, profiles/r04_f_ab.log)
    const double z_own = zc[row];
    int nbr_n = 0, tp_n = 0; double T_n = 0.0, th_n = 0.0;
    if (k0 < len) {
        const long e0 = long(base + k0) * 64 + lane;
        nbr_n = __builtin_nontemporal_load(&col[e0]); tp_n = __builtin_nontemporal_load(&tpos[e0]);
        T_n = __builtin_nontemporal_load(&tr_e[e0]);
        if (thp_e) th_n = __builtin_nontemporal_load(&thp_e[e0]);
    }
    for (int k = k0; k < len; ) {
        const int nbr = nbr_n, tp = tp_n; const double Te = T_n, thp = th_n;
        const int kn = (k + 1 == nl) ? k + 2 : k + 1;
        if (kn < len) {           // the next entry's words are in flight while this one is computed
            const long en = long(base + kn) * 64 + lane;
            nbr_n = __builtin_nontemporal_load(&col[en]); tp_n = __builtin_nontemporal_load(&tpos[en]);
            T_n = __builtin_nontemporal_load(&tr_e[en]);
            if (thp_e) th_n = __builtin_nontemporal_load(&thp_e[en]);
        }
        MS* bptr = A + long(base + k) * 576 + lane;
        float* bptr32 = DUAL ? A32 + long(base + k) * 576 + lane : nullptr;
        k = kn;
        if (Te != Te) {          // pure well fill: the host adds the Schur block later
#pragma unroll
            for (int c = 0; c < 9; ++c) { bptr[c * 64] = MS(0); if (DUAL) bptr32[c * 64] = 0.f; }
            continue;
        }
        const int side = __builtin_signbit(Te) ? 1 : 0;     // side 0: this row is c1 (ngrad +1), side 1: it is c2
        const double Tf = fabs(Te);
        const double z_n = zc[nbr];
        const double g = grav * (side ? z_n - z_own : z_own - z_n);          // g (z_c1 - z_c2): the expression the host evaluated per entry in round 3
        // neighbour values that every connection needs: phase pressures and densities
        double np_[3], nrho[3];
        np_[0] = vals[long(VP_PW) * nbp + nbr]; np_[1] = p[nbr]; if constexpr (NP == 3) np_[2] = vals[long(VP_PG) * nbp + nbr];
#pragma unroll
        for (int a = 0; a < NP; ++a) nrho[a] = vals[long(VP_RHO + a) * nbp + nbr];
        double nU[3] = { 0.0, 0.0, 0.0 }, nRs = 0.0, nRv = 0.0;
        if (BATCH) {
#pragma unroll
            for (int a = 0; a < NP; ++a) nU[a] = vals[long(VP_U + a) * nbp + nbr];
            if constexpr (NP == 3) { nRs = vals[long(VP_RS) * nbp + nbr]; nRv = vals[long(VP_RV) * nbp + nbr]; }
        }
        double Tdh[3], ddh[3][3];
        bool own_up[3];
#pragma unroll
        for (int a = 0; a < NP; ++a) {
            const double p1 = side ? np_[a] : op[a], p2 = side ? op[a] : np_[a];
            const double r1 = side ? nrho[a] : orho[a], r2 = side ? orho[a] : nrho[a];
            double dh = (p1 - p2) - g * (0.5 * r1 + 0.5 * r2);
            double keep = 1.0;
            if (thp_e) {
                keep = (fabs(dh) >= thp) ? 1.0 : 0.0;
                const double sg_ = (dh > 0.0) ? 1.0 : ((dh < 0.0) ? -1.0 : 0.0);
                dh = keep * (dh - sg_ * thp);
            }
            const double hg = 0.5 * g, sp = side ? -1.0 : 1.0;          // d dh / d(own variables): own is c1 (+) or c2 (-) in the pressure difference
#pragma unroll
            for (int v = 0; v < 3; ++v) ddh[a][v] = keep * (sp * dP[a][v] - hg * dRho[a][v]);
            own_up[a] = ((dh >= 0.0) ? 0 : 1) == side;                   // upwind cell = c1 if dh >= 0 else c2
            Tdh[a] = Tf * dh;
        }
        // upwind-dependent values of the neighbour.  BATCH: all five loaded with the pressures and densities above (one dependent round trip
        // per connection instead of two; the lines are fetched by some lane of the wave anyway); otherwise only the ones the upwinding asks for
        double Uv[3] = { oU[0], oU[1], NP == 3 ? oU[2] : 0.0 }, rsu = oRs, rvu = oRv;
        if (BATCH) {
#pragma unroll
            for (int a = 0; a < NP; ++a) Uv[a] = own_up[a] ? oU[a] : nU[a];
            if constexpr (NP == 3) { rsu = own_up[1] ? oRs : nRs; rvu = own_up[2] ? oRv : nRv; }
        } else {
#pragma unroll
            for (int a = 0; a < NP; ++a) if (!own_up[a]) Uv[a] = vals[long(VP_U + a) * nbp + nbr];
            if constexpr (NP == 3) {
                if (!own_up[1]) rsu = vals[long(VP_RS) * nbp + nbr];
                if (!own_up[2]) rvu = vals[long(VP_RV) * nbp + nbr];
            }
        }
        double F[3], dF[3][3];
#pragma unroll
        for (int a = 0; a < NP; ++a) {
            F[a] = Uv[a] * Tdh[a];
#pragma unroll
            for (int v = 0; v < 3; ++v) dF[a][v] = Uv[a] * (Tf * ddh[a][v]) + (own_up[a] ? dU[a][v] * Tdh[a] : 0.0);
        }
        if constexpr (NP == 2) {
            // G_w = F_w, G_o = F_o, nothing depends on the dummy unknown: block (nbr, row) = -s scale dF / d(P, Sw) in its water / oil
            // rows, exact zeros in its third column and in its gas row
            const double s = side ? -1.0 : 1.0;
            const bool nbr_ghost = mask && !mask[nbr];
            MS* tptr = A + long(tp >> 6) * 576 + (tp & 63);
            float* tptr32 = DUAL ? A32 + long(tp >> 6) * 576 + (tp & 63) : nullptr;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (a < 2) Rl[a] += s * F[a];
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                    double own = 0.0;
                    if (a < 2 && v < 2) {
                        own = s * scale[a] * dF[a][v];
                        if (v == 0) sod[a] += fabs(own);
                        D[3 * a + v] += own;
                    }
                    const bool z = nbr_ghost || a == 2 || v == 2;
                    __builtin_nontemporal_store(z ? MS(0) : MS(-own), &tptr[(3 * a + v) * 64]);
                    if (DUAL) __builtin_nontemporal_store(z ? 0.f : float(-own), &tptr32[(3 * a + v) * 64]);
                }
            }
            continue;
        }
        // G_o = F_o + rv_up(g) F_g ; G_g = F_g + rs_up(o) F_o
        const double G[3] = { F[0], F[1] + rvu * F[2], F[2] + rsu * F[1] };
        double dG[3][3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            dG[0][v] = dF[0][v];
            dG[1][v] = dF[1][v] + rvu * dF[2][v] + (own_up[2] ? dRv[v] * F[2] : 0.0);
            dG[2][v] = dF[2][v] + rsu * dF[1][v] + (own_up[1] ? dRs[v] * F[1] : 0.0);
        }
        const double s = side ? -1.0 : 1.0;
        // the neighbour's row sees this flux with the opposite sign: block (nbr, row) = -s scale dG / d(own); zero where that row is a ghost's
        const bool nbr_ghost = mask && !mask[nbr];
        MS* tptr = A + long(tp >> 6) * 576 + (tp & 63);
        float* tptr32 = DUAL ? A32 + long(tp >> 6) * 576 + (tp & 63) : nullptr;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            Rl[a] += s * G[a];
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const double own = s * scale[a] * dG[a][v];
                if (v == 0) sod[a] += fabs(own);
                D[3 * a + v] += own;
                __builtin_nontemporal_store(nbr_ghost ? MS(0) : MS(-own), &tptr[(3 * a + v) * 64]);
                if (DUAL) __builtin_nontemporal_store(nbr_ghost ? 0.f : float(-own), &tptr32[(3 * a + v) * 64]);
            }
        }
    }
    MS* dptr = A + long(base + nl) * 576 + lane;
    float* dptr32 = DUAL ? A32 + long(base + nl) * 576 + lane : nullptr;
    if (ghost) {
#pragma unroll
        for (int c = 0; c < 9; ++c) { dptr[c * 64] = (c == 0 || c == 4 || c == 8) ? MS(1) : MS(0); if (DUAL) dptr32[c * 64] = (c == 0 || c == 4 || c == 8) ? 1.f : 0.f; }
        R[row] = 0.0; R[nbp + row] = 0.0; R[2 * long(nbp) + row] = 0.0;
        if (wout) { wout[row] = MS(1); wout[nbp + row] = MS(0); wout[2 * long(nbp) + row] = MS(0); }      // identity row: its pressure entry
        return;
    }
    if constexpr (NP == 2) {      // the pinned gas unknown: identity row (exactly 1, whatever the scale), zero third column, zero residual
        D[2] = 0.0; D[5] = 0.0; D[6] = 0.0; D[7] = 0.0; D[8] = 1.0; Rl[2] = 0.0;
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) { __builtin_nontemporal_store(MS(D[c]), &dptr[c * 64]); if (DUAL) __builtin_nontemporal_store(float(D[c]), &dptr32[c * 64]); }
    if (wout) {
        const bool w_ = fabs(D[0]) / sod[0] > 0.01, g_ = NP == 3 && fabs(D[6]) / sod[2] > 0.01;       // NaN (0/0) compares false like the reference's Eigen cast
        bool o_ = fabs(D[3]) / sod[1] > 0.01;
        if (!o_ && !w_ && !g_) o_ = true;
        wout[row] = w_ ? MS(1) : MS(0); wout[nbp + row] = o_ ? MS(1) : MS(0); wout[2 * long(nbp) + row] = g_ ? MS(1) : MS(0);
    }
    R[row] = Rl[0]; R[nbp + row] = Rl[1]; R[2 * long(nbp) + row] = Rl[2];
}

// mixed precision: the device well model adds its own-cell derivatives to the DOUBLE diagonal blocks of the perforated cells after the
// reservoir assembly; their float copies follow
__global__ __launch_bounds__(kBlock) void k_refresh_f32_diag(int nperf, const int32_t* __restrict__ rows, const int32_t* __restrict__ slice_ptr,
                                                            const int16_t* __restrict__ nlower, const double* __restrict__ A, float* __restrict__ A32)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= nperf) return;
    const int row = rows[j];
    const long e = long(slice_ptr[row >> 6] + nlower[row]) * 576 + (row & 63);
#pragma unroll
    for (int c = 0; c < 9; ++c) A32[e + c * 64] = float(A[e + c * 64]);
}

// convergenceReduction (BlackoilModelBase_impl.hpp:1633-1714): per phase sum(1/b), sum R, non-finite flag (sums: slots 0..6),
// max|R|/pv, max|R| (maxima: slots 7..12); owned rows only (multi-GPU: followed by an all-reduce of each group)
__device__ __forceinline__ bool conv_is_max(int q) { return q >= 7; }
__global__ __launch_bounds__(kBlock) void k_conv_partial(int nb, int nbp, const double* __restrict__ R, const double* __restrict__ bpart, int nbpart,
                                                         const double* __restrict__ pv, const int8_t* __restrict__ mask, double* __restrict__ part)
{
    __shared__ double sm[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double vals[13];
#pragma unroll
    for (int q = 0; q < 13; ++q) vals[q] = 0.0;
    // sums of 1 / b: the per-workgroup partials of k_cell_values (owned cells only), spread over this launch's threads in a fixed order
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < nbpart; i += long(gridDim.x) * kBlock) {
#pragma unroll
        for (int a = 0; a < 3; ++a) vals[a] += bpart[long(a) * nbpart + i];
    }
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < nb; i += long(gridDim.x) * kBlock) {
        if (mask && !mask[i]) continue;
        const double ipv = 1.0 / pv[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double r = R[long(a) * nbp + i];
            vals[3 + a] += r;
            vals[7 + a] = fmax(vals[7 + a], fabs(r) * ipv);
            vals[10 + a] = fmax(vals[10 + a], fabs(r));
            if (!(fabs(r) <= 1.79e308)) vals[6] = 1.0;
        }
    }
#pragma unroll
    for (int q = 0; q < 13; ++q) {
        const bool is_max = conv_is_max(q);
        const double s = is_max ? wave_max(vals[q]) : wave_sum(vals[q]);
        __syncthreads();
        if (lane == 0) sm[w] = s;
        __syncthreads();
        if (threadIdx.x == 0) part[long(q) * gridDim.x + blockIdx.x] = is_max ? fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3])) : (sm[0] + sm[1]) + (sm[2] + sm[3]);
    }
}
__global__ __launch_bounds__(kBlock) void k_conv_final(int nblocks, const double* __restrict__ part, double* __restrict__ out)
{
    // one workgroup per scalar (13 of them), fixed order within each
    __shared__ double sm[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = blockIdx.x;
    const bool is_max = conv_is_max(q);
    double v = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kBlock) { const double x = part[long(q) * nblocks + i]; v = is_max ? fmax(v, x) : v + x; }
    const double s_ = is_max ? wave_max(v) : wave_sum(v);
    if (lane == 0) sm[w] = s_;
    __syncthreads();
    if (threadIdx.x == 0) out[q] = is_max ? fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3])) : (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// decomposed runs: the 7 sums and 6 (+ 6) maxima of getConvergence through ONE sum-all-reduce (see BlackoilDevice::convergence).
// phase 0: table[rank][:] = red[:], every other row zero; phase 1: red[q] = sum (q < 7) or max over the ranks' rows, in rank order
__global__ __launch_bounds__(kBlock) void k_conv_gather(int phase, int nv, int nranks, int rank, double* __restrict__ red, double* __restrict__ table)
{
    if (phase == 0) {
        for (int i = threadIdx.x; i < nranks * nv; i += kBlock) table[i] = (i / nv == rank) ? red[i % nv] : 0.0;
        return;
    }
    for (int q = threadIdx.x; q < nv; q += kBlock) {
        double v = table[q];
        for (int r = 1; r < nranks; ++r) { const double x = table[r * nv + q]; v = conv_is_max(q) ? fmax(v, x) : v + x; }
        red[q] = v;
    }
}

// updateState (BlackoilModelBase_impl.hpp:1147-1389), one thread per cell.  DRDT (dissolution limits, opmgpu_set_dissolution_limits): each of
// the four saturated ratios the switching logic compares against is the smaller of its present value and the cell's cap, which rides
// behind so_max (rs_cap_of / rv_cap_of), and a cell the decision leaves OIL_ONLY (GAS_ONLY) takes min(new rs, rs_cap) (min(new rv, rv_cap)):
// the decision itself is taken with the unlimited value.  Nothing else changes.
template <bool LDS, bool DRDT>
__global__ __launch_bounds__(kBlock) void k_update_state(int nb, int nbp, DevTables D, const int32_t* __restrict__ pvtnum,
                                                         const int32_t* __restrict__ satnum, const double* __restrict__ dx, double relax,
                                                         double dp_max_rel, double ds_max, double dr_max_rel,
                                                         double* __restrict__ p, double* __restrict__ sw, double* __restrict__ so,
                                                         double* __restrict__ sg, double* __restrict__ rs, double* __restrict__ rv, int8_t* __restrict__ hc,
                                                         const double* __restrict__ eps_planes, const double* __restrict__ eps_u0,
                                                         const double* __restrict__ somax, const double* __restrict__ tab_blob, int tab_words)
{
    extern __shared__ double tab_lds[];
    resolve_tables<LDS>(D, tab_blob, tab_words, tab_lds);
    const opmgpu_tables& T = D.t;
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nb) return;
    const double eps = 1.4901161193847656e-08;      // sqrt(DBL_EPSILON)
    const int preg = pvtnum[c], sreg = satnum[c];
    const int h = hc[c];
    const bool isSg = h == OPMGPU_HC_GAS_AND_OIL, isRs = h == OPMGPU_HC_OIL_ONLY, isRv = h == OPMGPU_HC_GAS_ONLY;
    const double dp = relax * dx[c], dsw = relax * dx[nbp + c], dxv = relax * dx[2 * long(nbp) + c];
    auto sgn = [](double x) { return (x > 0.0) ? 1.0 : ((x < 0.0) ? -1.0 : 0.0); };
    const double p_old = p[c];
    const double pn = fmax(p_old - sgn(dp) * fmin(fabs(dp), dp_max_rel * fabs(p_old)), 0.0);
    const double sw_old = sw[c], so_old = so[c], sg_old = sg[c];
    const double dsg = (isSg ? dxv : 0.0) - (isRv ? dsw : 0.0);
    const double dso = -dsw - dsg;
    const double maxVal = fmax(fabs(dso), fmax(fabs(dsg), fabs(dsw)));
    const double step = fmin(ds_max / maxVal, 1.0);
    double w_ = sw_old - step * dsw, g_ = sg_old - step * dsg, o_ = so_old - step * dso;
    if (g_ < 0) { w_ = w_ / (1 - g_); o_ = o_ / (1 - g_); g_ = 0; }
    if (o_ < 0) { w_ = w_ / (1 - o_); g_ = g_ / (1 - o_); o_ = 0; }
    if (w_ < 0) { o_ = o_ / (1 - w_); g_ = g_ / (1 - w_); w_ = 0; }
    const double rs_old = rs[c], rv_old = rv[c];
    double rsn = rs_old, rvn = rv_old;
    if (T.has_disgas) {
        const double d = isRs ? dxv : 0.0;
        rsn = fmax(rs_old - sgn(d) * fmin(fabs(d), fmax(fabs(rs_old) * dr_max_rel, 1.0)), 0.0);
    }
    if (T.has_vapoil) {
        const double d = isRv ? dxv : 0.0;
        rvn = fmax(rv_old - sgn(d) * fmin(fabs(d), fmax(fabs(rv_old) * dr_max_rel, 1e-3)), 0.0);
    }
    const bool watOnly = w_ > (1 - eps);
    int hn = OPMGPU_HC_GAS_AND_OIL;
    double f, df;
    if (T.has_disgas) {
        double v0, v1;
        vap_factor(T.vap2, so_old, somax[c], v0, df);
        vap_factor(T.vap2, o_, somax[c], v1, df);
        double rsSat0 = v0 * rs_sat_d(D, preg, p_old), rsSat = v1 * rs_sat_d(D, preg, pn);
        if constexpr (DRDT) { const double cap = rs_cap_of<KM_DRDT>(somax, nbp, c); rsSat0 = fmin(rsSat0, cap); rsSat = fmin(rsSat, cap); }
        const bool hasGas = (g_ > 0 && !isRs);
        const bool gasVaporized = ((rsn > rsSat * (1 + eps) && isRs) && (rs_old > rsSat0 * (1 - eps)));
        if (watOnly || hasGas || gasVaporized) { rsn = rsSat; if (watOnly) { o_ = 0; g_ = 0; rsn = 0; } }
        else {
            hn = OPMGPU_HC_OIL_ONLY;
            if constexpr (DRDT) rsn = fmin(rsn, rs_cap_of<KM_DRDT>(somax, nbp, c));
        }
    }
    if (T.has_vapoil) {
        const int ga = T.sgof_ptr[sreg], ng = T.sgof_ptr[sreg + 1] - ga;
        EpsD E;
        eps_load(eps_planes, eps_u0, nbp, c, sreg, E);
        sat_curve_s<true>(T.sgof_sg + ga, T.sgof_pcgo + ga, D.x.sgof_dpcgo + ga, ng, sg_old, E, EC_PCGO, f, df); const double pg_old = p_old + f;
        sat_curve_s<true>(T.sgof_sg + ga, T.sgof_pcgo + ga, D.x.sgof_dpcgo + ga, ng, g_, E, EC_PCGO, f, df); const double pg_new = pn + f;
        double v0, v1;
        vap_factor(T.vap1, so_old, somax[c], v0, df);
        vap_factor(T.vap1, o_, somax[c], v1, df);
        double rvSat0 = v0 * rv_sat_d(D, preg, pg_old), rvSat = v1 * rv_sat_d(D, preg, pg_new);
        if constexpr (DRDT) { const double cap = rv_cap_of<KM_DRDT>(somax, nbp, c); rvSat0 = fmin(rvSat0, cap); rvSat = fmin(rvSat, cap); }
        const bool hasOil = (o_ > 0 && !isRv);
        const bool oilCondensed = ((rvn > rvSat * (1 + eps) && isRv) && (rv_old > rvSat0 * (1 - eps)));
        if (watOnly || hasOil || oilCondensed) { rvn = rvSat; if (watOnly) { o_ = 0; g_ = 0; rvn = 0; } }
        else {
            hn = OPMGPU_HC_GAS_ONLY;
            if constexpr (DRDT) rvn = fmin(rvn, rv_cap_of<KM_DRDT>(somax, nbp, c));
        }
    }
    p[c] = pn; sw[c] = w_; so[c] = o_; sg[c] = g_;
    if (T.has_disgas) rs[c] = rsn;
    if (T.has_vapoil) rv[c] = rvn;
    hc[c] = int8_t(hn);
}

// b = matbalscale * R in the solver's precision (NewtonIterationBlackoilInterleaved.cpp:234-236, 263-269)
template <class S>
__global__ __launch_bounds__(kBlock) void k_build_rhs(int nb, int nbp, double s0, double s1, double s2, const double* __restrict__ R,
                                                      const double* __restrict__ extra, S* __restrict__ b)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nb) return;
    const long i1 = nbp + i, i2 = 2 * long(nbp) + i;
    double r0 = R[i], r1 = R[i1], r2 = R[i2];
    if (extra) { r0 += extra[i]; r1 += extra[i1]; r2 += extra[i2]; }
    b[i] = S(s0 * r0); b[i1] = S(s1 * r1); b[i2] = S(s2 * r2);
}
__global__ __launch_bounds__(kBlock) void k_gather_perf3(int nperf, int nbp, const int32_t* __restrict__ cells, const double* __restrict__ v, double* __restrict__ out)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nperf) return;
    const int c = cells[i];
    out[3 * long(i)] = v[c]; out[3 * long(i) + 1] = v[nbp + c]; out[3 * long(i) + 2] = v[2 * long(nbp) + c];
}

// per-perforation properties for the host well model (extractWellPerfProperties)
template <int KM>
__global__ __launch_bounds__(kBlock) void k_perf_props(int nperf, DevTables T, const int32_t* __restrict__ cells, CellPlanes C, double* __restrict__ out)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nperf) return;
    const int c = cells[i];
    CellEval q;
    eval_row<KM>(T, c, C, q);
    const V4 list[9] = { mk(C.p[c], 1, 0, 0), q.rs, q.rv, q.b[0], q.b[1], q.b[2], q.mob[0], q.mob[1], q.mob[2] };
    double* o = out + long(i) * OPMGPU_PERF_K;
#pragma unroll
    for (int k = 0; k < 9; ++k) { o[4 * k] = list[k].v; o[4 * k + 1] = list[k].p; o[4 * k + 2] = list[k].w; o[4 * k + 3] = list[k].x; }
}

// computePropertiesForWellConnectionPressures (StandardWells_impl.hpp:218-296): b_w, b_o, b_g, rsSat, rvSat of the perforated cells at
// GIVEN pressures (the average well-block pressures) with the cells' own rs / rv / phase condition / oil saturation
__global__ __launch_bounds__(kBlock) void k_perf_pvt(int nperf, DevTables D, const int32_t* __restrict__ cells, const int32_t* __restrict__ pvtnum,
                                                     const double* __restrict__ so, const double* __restrict__ rs, const double* __restrict__ rv,
                                                     const int8_t* __restrict__ hc, const double* __restrict__ somax, const double* __restrict__ press,
                                                     const int32_t* __restrict__ gate, double* __restrict__ out)
{
    if (gate && !*gate) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nperf) return;
    const opmgpu_tables& T = D.t;
    const int c = cells[i], preg = pvtnum[c], h = hc[c];
    const bool freeGas = h != OPMGPU_HC_OIL_ONLY, freeOil = h != OPMGPU_HC_GAS_ONLY;
    const double p = press[i];
    double* o = out + 5 * long(i);
    b_values(D, preg, p, rs[c], rv[c], freeGas || !T.has_disgas, freeOil || !T.has_vapoil, o[0], o[1], o[2]);
    double f = rs_sat_d(D, preg, p), v, df;
    if (T.vap2 > 0.0) { vap_factor(T.vap2, so[c], somax[c], v, df); f *= v; }
    o[3] = f;
    f = rv_sat_d(D, preg, p);
    if (T.vap1 > 0.0) { vap_factor(T.vap1, so[c], somax[c], v, df); f *= v; }
    o[4] = f;
}

__global__ __launch_bounds__(kBlock) void k_add_well_resid(int nperf, int nbp, const int32_t* __restrict__ cells, const double* __restrict__ delta, double* __restrict__ R)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nperf) return;
    for (int a = 0; a < 3; ++a) atomicAdd(&R[long(a) * nbp + cells[i]], delta[3 * i + a]);
}
__global__ __launch_bounds__(kBlock) void k_add_well_blocks(int nblk, const int32_t* __restrict__ entries, const double* __restrict__ blocks,
                                                            double s0, double s1, double s2, double* __restrict__ A)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nblk) return;
    const int e = entries[i];
    const double scale[3] = { s0, s1, s2 };
    double* o = A + long(e >> 6) * 576 + (e & 63);
    for (int a = 0; a < 3; ++a) for (int v = 0; v < 3; ++v) atomicAdd(&o[(3 * a + v) * 64], scale[a] * blocks[9 * long(i) + 3 * a + v]);
}

// stabilizeNonlinearUpdate: dx_old <- dx; dx <- omega*dx (+ (1-omega)*previous dx_old for SOR)
__global__ __launch_bounds__(kBlock) void k_stabilize(long n, int sor, double omega, double* __restrict__ dx, double* __restrict__ dx_old)
{
    const long i = long(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    const double d = dx[i], o = dx_old[i];
    dx_old[i] = d;
    if (omega == 1.0) return;
    dx[i] = sor ? omega * d + (1.0 - omega) * o : omega * d;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
void BlackoilDevice::check_transmissibilities(const opmgpu_grid* g)
{
    if (g->nconn > 0 && !g->trans) throw HipError(OPMGPU_EINVAL, "opmgpu_grid.trans is NULL");
    for (int f = 0; f < g->nconn; ++f)
        if (!(g->trans[f] >= 0.0) || !std::isfinite(g->trans[f]))
            throw HipError(OPMGPU_EINVAL, "the transmissibility of connection " + std::to_string(f) + " (cells " + std::to_string(g->conn_cells[2 * f]) + ", " +
                                          std::to_string(g->conn_cells[2 * f + 1]) + ") is negative or not finite");
}

BlackoilDevice::BlackoilDevice(hipStream_t s, LinSolver& ls_, const opmgpu_grid* g, const opmgpu_tables* t, const opmgpu_params* prm_)
    : prm(*prm_), stream(s), ls(ls_)
{
    nc = g->nc; nconn = g->nconn; gravity = g->gravity;
    n_owned_cells = nc;
    h_conn.assign(g->conn_cells, g->conn_cells + 2 * size_t(nconn));
    check_transmissibilities(g);
    h_trans.assign(g->trans, g->trans + nconn);
    h_pv.assign(g->pv, g->pv + nc);
    h_z.assign(g->z, g->z + nc);
    use_thpres = g->thpres != nullptr;
    if (use_thpres) h_thpres.assign(g->thpres, g->thpres + nconn);
    h_pvtnum.assign(nc, 0); h_satnum.assign(nc, 0);
    if (g->pvtnum) h_pvtnum.assign(g->pvtnum, g->pvtnum + nc);
    if (g->satnum) h_satnum.assign(g->satnum, g->satnum + nc);
    if (t->active_phases != OPMGPU_PHASES_ALL && t->active_phases != OPMGPU_PHASES_OIL_WATER)
        throw HipError(OPMGPU_EINVAL, "active_phases is neither 0 (water, oil and gas) nor OPMGPU_PHASES_OIL_WATER: oil-gas, gas-water and single-phase decks are not supported");
    const bool ow = t->active_phases == OPMGPU_PHASES_OIL_WATER;
    if (ow) {
        if (t->has_disgas || t->has_vapoil) throw HipError(OPMGPU_EINVAL, "OPMGPU_PHASES_OIL_WATER: has_disgas / has_vapoil (DISGAS / VAPOIL) need a gas phase");
        if (t->vap1 != 0.0 || t->vap2 != 0.0) throw HipError(OPMGPU_EINVAL, "OPMGPU_PHASES_OIL_WATER: vap1 / vap2 (VAPPARS) need a gas phase");
        if (t->threephase_model != OPMGPU_KRO_DEFAULT) throw HipError(OPMGPU_EINVAL, "OPMGPU_PHASES_OIL_WATER: threephase_model must be OPMGPU_KRO_DEFAULT (a Stone law needs a gas phase)");
        if (g->imbnum) throw HipError(OPMGPU_EINVAL, "OPMGPU_PHASES_OIL_WATER together with hysteresis (imbnum) is not supported");
    }
    has_endpoints = g->eps[0] != nullptr;
    if (has_endpoints)
        for (int k = 0; k < 8; ++k) {
            if (ow && k >= 4) continue;                   // no gas phase: the gas end points are not read (set below)
            if (!g->eps[k]) throw HipError(OPMGPU_EINVAL, "ENDSCALE needs all eight end-point arrays (SWL SWCR SWU SOWCR SGL SGCR SGU SOGCR)");
            h_eps[k].assign(g->eps[k], g->eps[k] + nc);
        }
    if (has_endpoints && ow) {
        // what the gas curves of the internal stand-in tables (upload_tables) would be scaled with; only SGL = 0 enters an oil-water curve
        h_eps[4].assign(nc, 0.0); h_eps[5].assign(nc, 0.0); h_eps[6].resize(nc); h_eps[7] = h_eps[3];
        for (int c = 0; c < nc; ++c) h_eps[6][c] = 1.0 - h_eps[0][c];
    }
    scalecrs = g->scalecrs != 0;
    if (scalecrs && !has_endpoints) throw HipError(OPMGPU_EINVAL, "SCALECRS needs the end-point arrays");
    bool vert = false;
    for (int k = 0; k < 5; ++k) if (g->eps_v[k] && !(ow && (k == 2 || k == 4))) { h_eps_v[k].assign(g->eps_v[k], g->eps_v[k] + nc); vert = true; }
    use_hyst = g->imbnum != nullptr;
    if (use_hyst) {
        h_imbnum.assign(g->imbnum, g->imbnum + nc);
        for (int c = 0; c < nc; ++c) if (h_imbnum[c] < 0 || h_imbnum[c] >= t->n_sat_regions) throw HipError(OPMGPU_EINVAL, "IMBNUM region out of range");
        has_iendpoints = g->ieps[0] != nullptr;
        if (has_iendpoints)
            for (int k = 0; k < 8; ++k) {
                if (!g->ieps[k]) throw HipError(OPMGPU_EINVAL, "imbibition end points: all eight arrays or none");
                h_ieps[k].assign(g->ieps[k], g->ieps[k] + nc);
            }
    }
    use_eps = has_endpoints || vert || use_hyst;
    if (t->threephase_model != OPMGPU_KRO_DEFAULT && t->threephase_model != OPMGPU_KRO_STONE1 && t->threephase_model != OPMGPU_KRO_STONE2)
        throw HipError(OPMGPU_EINVAL, "threephase_model is none of OPMGPU_KRO_DEFAULT, OPMGPU_KRO_STONE1, OPMGPU_KRO_STONE2");
    if (t->threephase_model != OPMGPU_KRO_DEFAULT && use_hyst)
        throw HipError(OPMGPU_EINVAL, "a Stone three-phase model together with hysteresis (imbnum) is not supported");
    if (t->stone1_exponent)
        for (int r = 0; r < t->n_sat_regions; ++r) if (!(t->stone1_exponent[r] > 0.0)) throw HipError(OPMGPU_EINVAL, "stone1_exponent must be positive in every saturation region");
    pvsum = 0.0;
    for (int c = 0; c < nc; ++c) pvsum += h_pv[c];
    upload_tables(t);
    OPMGPU_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_red), 32 * sizeof(double)));
    h_well_connpos.assign(1, 0);
    rebuild_structure();
}

BlackoilDevice::~BlackoilDevice()
{
    wells_free();
    vfp_free();
    aquifer_free();
    if (h_red) (void)hipHostFree(h_red);
    for (auto e : ev_well) if (e) (void)hipEventDestroy(e);
    if (well_stream) (void)hipStreamDestroy(well_stream);
}

#include "blackoil_setup.inl"

HystArgs BlackoilDevice::hyst_args() const
{
    HystArgs h;
    h.imbnum = use_hyst ? d_imbnum.p : nullptr; h.hist = d_hist.p; h.ieps = d_ieps.p; h.iureg = d_ieps_u0.p;
    return h;
}
CellPlanes BlackoilDevice::cell_planes() const
{
    CellPlanes c;
    c.pvtnum = d_pvtnum.p; c.satnum = d_satnum.p;
    c.p = d_p.p; c.sw = d_sw.p; c.so = d_so.p; c.sg = d_sg.p; c.rs = d_rs.p; c.rv = d_rv.p; c.hc = d_hc.p;
    c.eps = eps_planes(); c.eps_u0 = d_eps_u0.p; c.somax = d_somax.p;
    c.nbp = ls.plan.nbp; c.hy = hyst_args();
    return c;
}

// ---- hysteresis history -------------------------------------------------------------------------------------------------------
// smallest abscissa at which the monotone piecewise-linear table takes the value yv (flat pieces: the left end)
__device__ double table_inverse(const double* __restrict__ x, const double* __restrict__ y, int n, double yv, bool ascending)
{
    if (ascending) {
        if (yv <= y[0]) return x[0];
        for (int i = 0; i + 1 < n; ++i) if (y[i] < yv && yv <= y[i + 1]) return x[i] + (yv - y[i]) / (y[i + 1] - y[i]) * (x[i + 1] - x[i]);
        return x[n - 1];
    }
    if (yv >= y[0]) return x[0];
    for (int i = 0; i + 1 < n; ++i) if (y[i] > yv && yv >= y[i + 1]) return x[i] + (yv - y[i]) / (y[i + 1] - y[i]) * (x[i + 1] - x[i]);
    return x[n - 1];
}
// the end of the run of zero ordinates at the low (low = true) or the high end of a table: the abscissa of the run's innermost node; the
// end node itself where the curve is not zero there
__device__ double table_zero_end(const double* __restrict__ x, const double* __restrict__ y, int n, bool low)
{
    if (low) { int i = 0; while (i + 1 < n && y[i + 1] <= 0.0) ++i; return x[i]; }
    int i = n - 1;
    while (i > 0 && y[i - 1] <= 0.0) --i;
    return x[i];
}
// Killough's scanning curve of one two-phase system in the non-wetting saturation Sn (the rule is stated in include/opmgpu.h at
// opmgpu_set_hysteresis_model): trapped saturation, slope and ratio from the turning point shy, the critical saturations of the cell's
// drainage and imbibition curves, the drainage curve's largest saturation and the cell's two curves themselves
template <class KD, class KI>
__device__ void killough_scan(double shy, double sncrd, double sncri, double snmax, double a, KD&& krnd, KI&& krni, double& sncrt, double& m, double& R)
{
    shy = fmin(shy, snmax);
    const double kd = krnd(shy), ki = krni(snmax), D = shy - sncrd;
    sncrt = sncrd;
    if (sncri > sncrd && snmax > sncrd) {
        const double C = 1.0 / (sncri - sncrd) - 1.0 / (snmax - sncrd);
        sncrt = sncrd + D / (1.0 + a * (snmax - shy) + C * D);
    }
    m = 0.0; R = 0.0;
    if (kd > 0.0 && ki > 0.0 && snmax > sncri) { m = (snmax - sncri) / (shy - sncrt); R = kd / ki; }
}
// EclDefaultMaterial::updateHysteresis ("inconsistent" form: krnSw = 1 - So / 1 - Sg) + EclHysteresisTwoPhaseLawParams::update +
// updateDynamicParams_ (Carlson shift: delta = Sw_imb(krn_drain(mdc)) - mdc), one thread per cell.  model == OPMGPU_HYST_KILLOUGH: the
// parameters of Killough's scanning curves instead, in the affine form the evaluator takes (HystD); Carlson fills m = R = 1.
__global__ __launch_bounds__(kBlock) void k_hyst_update(int nb, int nbp, DevTables D, const int32_t* __restrict__ satnum, const int32_t* __restrict__ imbnum,
                                                        const double* __restrict__ so, const double* __restrict__ sg, const double* __restrict__ eps,
                                                        const double* __restrict__ ieps, const double* __restrict__ ureg, const double* __restrict__ iureg,
                                                        double* __restrict__ hist, int force, int model, double kill_a)
{
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nb) return;
    double mow = hist[c], mgo = hist[nbp + c];
    bool upd = force != 0;
    const double sgc = fmin(1.0, fmax(0.0, sg[c]));
    if (!force) {
        if (1.0 - so[c] < mow) { mow = 1.0 - so[c]; upd = true; }
        if (1.0 - sgc < mgo) { mgo = 1.0 - sgc; upd = true; }
    }
    if (!upd) return;
    const opmgpu_tables& T = D.t;
    const int sreg = satnum[c], ireg = imbnum[c];
    EpsD E, EI;
    eps_load(eps, ureg, nbp, c, sreg, E);
    eps_load(ieps, iureg, nbp, c, ireg, EI);
    double dow = 0.0, dgo = 0.0, f, df;
    double m_ow = 1.0, m_go = 1.0, r_ow = 1.0, r_go = 1.0, t_ow = 0.0, t_go = 0.0;
    const long np = nbp;
    if (model == OPMGPU_HYST_KILLOUGH) {
        const TabX& X = D.x;
        if (mow < 2.0) {        // oil against water: Sn = 1 - Sw_ow, the curves are krow at 1 - Sn
            const int wa = T.swof_ptr[sreg], wi = T.swof_ptr[ireg], nw = T.swof_ptr[sreg + 1] - wa, ni = T.swof_ptr[ireg + 1] - wi;
            const double* xd = T.swof_sw + wa; const double* xi = T.swof_sw + wi;
            const double sncrd = 1.0 - eps_unmap(E, EC_KROW, table_zero_end(xd, T.swof_krow + wa, nw, false));
            const double sncri = 1.0 - eps_unmap(EI, EC_KROW, table_zero_end(xi, T.swof_krow + wi, ni, false));
            const double snmax = 1.0 - eps_unmap(E, EC_KROW, xd[0]);
            auto kd = [&](double S) { double g, dg; sat_curve_s<false>(xd, T.swof_krow + wa, X.swof_dkrow + wa, nw, 1.0 - S, E, EC_KROW, g, dg); return g; };
            auto ki = [&](double S) { double g, dg; sat_curve_s<false>(xi, T.swof_krow + wi, X.swof_dkrow + wi, ni, 1.0 - S, EI, EC_KROW, g, dg); return g; };
            killough_scan(1.0 - mow, sncrd, sncri, snmax, kill_a, kd, ki, t_ow, m_ow, r_ow);
            dow = 1.0 - sncri - m_ow * (1.0 - t_ow);            // Sw_imb = 1 - (Sncri + m (1 - Sw_ow - Sncrt)) = d_ow + m Sw_ow
        }
        if (mgo < 2.0) {        // gas against oil: Sn = Sg
            const int ga = T.sgof_ptr[sreg], gi = T.sgof_ptr[ireg], ng = T.sgof_ptr[sreg + 1] - ga, ni = T.sgof_ptr[ireg + 1] - gi;
            const double* xd = T.sgof_sg + ga; const double* xi = T.sgof_sg + gi;
            const double sncrd = eps_unmap(E, EC_KRG, table_zero_end(xd, T.sgof_krg + ga, ng, true));
            const double sncri = eps_unmap(EI, EC_KRG, table_zero_end(xi, T.sgof_krg + gi, ni, true));
            const double snmax = eps_unmap(E, EC_KRG, xd[ng - 1]);
            auto kd = [&](double S) { double g, dg; sat_curve_s<true>(xd, T.sgof_krg + ga, X.sgof_dkrg + ga, ng, S, E, EC_KRG, g, dg); return g; };
            auto ki = [&](double S) { double g, dg; sat_curve_s<true>(xi, T.sgof_krg + gi, X.sgof_dkrg + gi, ni, S, EI, EC_KRG, g, dg); return g; };
            killough_scan(1.0 - mgo, sncrd, sncri, snmax, kill_a, kd, ki, t_go, m_go, r_go);
            dgo = m_go * t_go - sncri;                          // Sg_imb = Sncri + m (Sg - Sncrt) = m Sg - d_go
        }
        hist[c] = mow; hist[np + c] = mgo; hist[HP_D_OW * np + c] = dow; hist[HP_D_GO * np + c] = dgo;
        hist[HP_M_OW * np + c] = m_ow; hist[HP_M_GO * np + c] = m_go; hist[HP_R_OW * np + c] = r_ow; hist[HP_R_GO * np + c] = r_go;
        hist[HP_SNCRT_OW * np + c] = t_ow; hist[HP_SNCRT_GO * np + c] = t_go;
        return;
    }
    if (mow < 2.0) {
        const int wa = T.swof_ptr[sreg], wi = T.swof_ptr[ireg];
        sat_curve_s<false>(T.swof_sw + wa, T.swof_krow + wa, D.x.swof_dkrow + wa, T.swof_ptr[sreg + 1] - wa, mow, E, EC_KROW, f, df);
        const double ku = f / EI.v[EC_KROW];
        if (ku > 0.0) dow = eps_unmap(EI, EC_KROW, table_inverse(T.swof_sw + wi, T.swof_krow + wi, T.swof_ptr[ireg + 1] - wi, ku, false)) - mow;
    }
    if (mgo < 2.0) {
        const int ga = T.sgof_ptr[sreg], gi = T.sgof_ptr[ireg];
        const double sgm = 1.0 - mgo;
        sat_curve_s<true>(T.sgof_sg + ga, T.sgof_krg + ga, D.x.sgof_dkrg + ga, T.sgof_ptr[sreg + 1] - ga, sgm, E, EC_KRG, f, df);
        const double ku = f / EI.v[EC_KRG];
        if (ku > 0.0) dgo = sgm - eps_unmap(EI, EC_KRG, table_inverse(T.sgof_sg + gi, T.sgof_krg + gi, T.sgof_ptr[ireg + 1] - gi, ku, true));
    }
    hist[c] = mow; hist[nbp + c] = mgo; hist[2 * long(nbp) + c] = dow; hist[3 * long(nbp) + c] = dgo;
    if (force) {        // Carlson's m = R = 1, Sncrt = 0 are what the planes start with (hist_planes): only a change of model rewrites them
        hist[HP_M_OW * np + c] = m_ow; hist[HP_M_GO * np + c] = m_go; hist[HP_R_OW * np + c] = r_ow; hist[HP_R_GO * np + c] = r_go;
        hist[HP_SNCRT_OW * np + c] = t_ow; hist[HP_SNCRT_GO * np + c] = t_go;
    }
}
// the HP_COUNT planes of a plan without a history: mdc = 2, zero shifts, m = R = 1 (Carlson's affine form), Sncrt = 0 -- padding rows included
std::vector<double> BlackoilDevice::hist_planes() const
{
    const size_t nbp = ls.plan.nbp;
    std::vector<double> hp(size_t(HP_COUNT) * nbp, 0.0);
    for (size_t r = 0; r < nbp; ++r) {
        hp[r] = 2.0; hp[nbp + r] = 2.0;
        for (int k = HP_M_OW; k <= HP_R_GO; ++k) hp[size_t(k) * nbp + r] = 1.0;
    }
    return hp;
}
void BlackoilDevice::launch_hyst_update(int force)
{
    hipLaunchKernelGGL(k_hyst_update, dim3(grid_for(nc)), dim3(kBlock), 0, stream, nc, ls.plan.nbp, dtp_, d_satnum.p, d_imbnum.p, d_so.p, d_sg.p,
                       (const double*)d_eps.p, (const double*)d_ieps.p, (const double*)d_eps_u0.p, (const double*)d_ieps_u0.p, d_hist.p, force, hyst_model, killough_a);
}

int BlackoilDevice::update_hysteresis()
{
    if (!use_hyst) return OPMGPU_OK;
    if (!has_state) return OPMGPU_EINVAL;
    launch_hyst_update(0);
    return OPMGPU_OK;
}
int BlackoilDevice::set_hysteresis(const double* mdc_ow, const double* mdc_go)
{
    if (!use_hyst || !mdc_ow || !mdc_go) return OPMGPU_EINVAL;
    const Plan& P = ls.plan;
    std::vector<double> hp = hist_planes();
    for (int r = 0; r < nc; ++r) { hp[r] = mdc_ow[P.nat[r]]; hp[size_t(P.nbp) + r] = mdc_go[P.nat[r]]; }
    d_hist.upload(hp, stream);
    // the shifts (the scanning parameters) follow from the history
    launch_hyst_update(1);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    return OPMGPU_OK;
}
// The scanning-curve model of the hysteresis (opmgpu_set_hysteresis_model).  With a resident history its derived planes are recomputed
// from the two history planes (the force path of k_hyst_update, as set_hysteresis does).
int BlackoilDevice::set_hysteresis_model(int model, double a)
{
    if (!use_hyst) throw HipError(OPMGPU_EINVAL, "opmgpu_set_hysteresis_model: the context has no hysteresis (opmgpu_grid.imbnum is NULL)");
    if (model != OPMGPU_HYST_CARLSON && model != OPMGPU_HYST_KILLOUGH)
        throw HipError(OPMGPU_EINVAL, "opmgpu_set_hysteresis_model: model " + std::to_string(model) + " is neither OPMGPU_HYST_CARLSON (0) nor OPMGPU_HYST_KILLOUGH (2)");
    if (!std::isfinite(a)) throw HipError(OPMGPU_EINVAL, "opmgpu_set_hysteresis_model: killough_a is not finite");
    if (a < 0.0) throw HipError(OPMGPU_EINVAL, "opmgpu_set_hysteresis_model: killough_a is negative");
    hyst_model = model; killough_a = a;
    launch_hyst_update(1);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    return OPMGPU_OK;
}
int BlackoilDevice::get_hysteresis_scanning(double* sncrt_ow, double* m_ow, double* r_ow, double* sncrt_go, double* m_go, double* r_go)
{
    if (!use_hyst) throw HipError(OPMGPU_EINVAL, "opmgpu_get_hysteresis_scanning: the context has no hysteresis (opmgpu_grid.imbnum is NULL)");
    const Plan& P = ls.plan;
    std::vector<double> hp(size_t(HP_COUNT) * P.nbp);
    d_hist.download(hp.data(), hp.size(), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    double* out[6] = { sncrt_ow, m_ow, r_ow, sncrt_go, m_go, r_go };
    const int plane[6] = { HP_SNCRT_OW, HP_M_OW, HP_R_OW, HP_SNCRT_GO, HP_M_GO, HP_R_GO };
    for (int k = 0; k < 6; ++k) if (out[k]) for (int r = 0; r < nc; ++r) out[k][P.nat[r]] = hp[size_t(plane[k]) * P.nbp + r];
    return OPMGPU_OK;
}
int BlackoilDevice::get_hysteresis(double* mdc_ow, double* mdc_go, double* d_ow, double* d_go)
{
    if (!use_hyst) return OPMGPU_EINVAL;
    const Plan& P = ls.plan;
    std::vector<double> hp(4 * size_t(P.nbp));
    d_hist.download(hp.data(), hp.size(), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    double* out[4] = { mdc_ow, mdc_go, d_ow, d_go };
    for (int k = 0; k < 4; ++k) if (out[k]) for (int r = 0; r < nc; ++r) out[k][P.nat[r]] = hp[size_t(k) * P.nbp + r];
    return OPMGPU_OK;
}

void BlackoilDevice::set_state(const double* p, const double* sat, const double* rs, const double* rv, const int8_t* hc)
{
    const Plan& P = ls.plan;
    const int nbp = P.nbp;
    hbuf.assign(6 * size_t(nbp), 0.0); hbuf8.assign(nbp, int8_t(OPMGPU_HC_GAS_AND_OIL));
    for (int r = 0; r < nc; ++r) {
        const int c = P.nat[r];
        hbuf[r] = p[c]; hbuf[nbp + r] = sat[3 * size_t(c)]; hbuf[2 * size_t(nbp) + r] = sat[3 * size_t(c) + 1];
        hbuf[3 * size_t(nbp) + r] = sat[3 * size_t(c) + 2]; hbuf[4 * size_t(nbp) + r] = rs[c]; hbuf[5 * size_t(nbp) + r] = rv[c];
        hbuf8[r] = hc[c];
        if (oil_water()) {        // no gas phase: Sg = rs = rv = 0 exactly, the phase condition is not the caller's
            hbuf[3 * size_t(nbp) + r] = 0.0; hbuf[4 * size_t(nbp) + r] = 0.0; hbuf[5 * size_t(nbp) + r] = 0.0;
            hbuf8[r] = int8_t(OPMGPU_HC_GAS_AND_OIL);
        }
    }
    DevArray<double>* planes[] = { &d_p, &d_sw, &d_so, &d_sg, &d_rs, &d_rv };
    for (int k = 0; k < 6; ++k) OPMGPU_HIP(hipMemcpyAsync(planes[k]->p, hbuf.data() + size_t(k) * nbp, nbp * sizeof(double), hipMemcpyHostToDevice, stream));
    OPMGPU_HIP(hipMemcpyAsync(d_hc.p, hbuf8.data(), nbp, hipMemcpyHostToDevice, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
    has_state = true;
}

void BlackoilDevice::get_state(double* p, double* sat, double* rs, double* rv, int8_t* hc)
{
    const Plan& P = ls.plan;
    const int nbp = P.nbp;
    hbuf.resize(6 * size_t(nbp)); hbuf8.resize(nbp);
    DevArray<double>* planes[] = { &d_p, &d_sw, &d_so, &d_sg, &d_rs, &d_rv };
    for (int k = 0; k < 6; ++k) OPMGPU_HIP(hipMemcpyAsync(hbuf.data() + size_t(k) * nbp, planes[k]->p, nbp * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipMemcpyAsync(hbuf8.data(), d_hc.p, nbp, hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
    for (int r = 0; r < nc; ++r) {
        const int c = P.nat[r];
        if (p) p[c] = hbuf[r];
        if (sat) { sat[3 * size_t(c)] = hbuf[nbp + r]; sat[3 * size_t(c) + 1] = hbuf[2 * size_t(nbp) + r]; sat[3 * size_t(c) + 2] = hbuf[3 * size_t(nbp) + r]; }
        if (rs) rs[c] = hbuf[4 * size_t(nbp) + r];
        if (rv) rv[c] = hbuf[5 * size_t(nbp) + r];
        if (hc) hc[c] = hbuf8[r];
    }
}

// THE statement of the shapes the two assembly kernels are compiled in: (tables in LDS or not) x (the three models), run time -> compile
// time.  pick(L, K) gets the shape as two integral constants and returns the kernel's pointer (the same type in every shape).
template <class F> static auto kernel_by_shape(bool lds, int km, F&& pick)
{
    auto by_model = [&](auto L) {
        // dissolution limits (KM_DRDT): the three three-phase models with the tabulated oil, nothing else (set_dissolution_limits refuses the rest)
        if (km_rock(km)) {      // rock regions (KM_ROCK): the four models with the tabulated oil and without limits (set_rock_regions refuses the rest)
            auto by_rock = [&](auto K) { return pick(L, std::integral_constant<int, decltype(K)::value | KM_ROCK>{}); };
            return km_model(km) == KM_OW ? by_rock(std::integral_constant<int, KM_OW>{})
                 : km_model(km) == KM_STONE ? by_rock(std::integral_constant<int, KM_STONE>{})
                 : km_model(km) == KM_KILLOUGH ? by_rock(std::integral_constant<int, KM_KILLOUGH>{}) : by_rock(std::integral_constant<int, KM_DEFAULT>{});
        }
        if (km_drdt(km))
            return km_model(km) == KM_STONE ? pick(L, std::integral_constant<int, KM_STONE | KM_DRDT>{})
                 : km_model(km) == KM_KILLOUGH ? pick(L, std::integral_constant<int, KM_KILLOUGH | KM_DRDT>{}) : pick(L, std::integral_constant<int, KM_DEFAULT | KM_DRDT>{});
        auto by_oil = [&](auto K) {       // the tabulated oil, or the analytic one of opmgpu_set_pvcdo
            return km_pvcdo(km) ? pick(L, std::integral_constant<int, decltype(K)::value | KM_PVCDO>{}) : pick(L, K);
        };
        return km_model(km) == KM_OW ? by_oil(std::integral_constant<int, KM_OW>{})
             : km_model(km) == KM_STONE ? by_oil(std::integral_constant<int, KM_STONE>{})
             : km_model(km) == KM_KILLOUGH ? by_oil(std::integral_constant<int, KM_KILLOUGH>{}) : by_oil(std::integral_constant<int, KM_DEFAULT>{});
    };
    return lds ? by_model(std::true_type{}) : by_model(std::false_type{});
}
// k_assemble_rows of a shape.  The float copy is only ever written next to a DOUBLE Jacobian: no float dual kernel exists.
template <class MS> static auto assemble_rows_kernel(bool lds, bool dual, int km)
{
    if constexpr (sizeof(MS) == 8)
        if (dual) return kernel_by_shape(lds, km, [](auto L, auto K) { return &k_assemble_rows<MS, decltype(L)::value, true, decltype(K)::value>; });
    return kernel_by_shape(lds, km, [](auto L, auto K) { return &k_assemble_rows<MS, decltype(L)::value, false, decltype(K)::value>; });
}

void BlackoilDevice::launch_cell_values()
{
    const Plan& P = ls.plan;
    auto kern = kernel_by_shape(tab_lds_words() > 0, kmodel(), [](auto L, auto K) { return &k_cell_values<decltype(L)::value, decltype(K)::value>; });
    hipLaunchKernelGGL(kern, dim3(grid_for(nc)), dim3(kBlock), tab_lds_bytes(), stream, nc, P.nbp, dto_, d_pvtnum.p, d_satnum.p,
                       d_p.p, d_sw.p, d_sg.p, d_rs.p, d_rv.p, d_hc.p, eps_planes(), d_eps_u0.p, d_somax.p, d_vals.p, d_bpart.p,
                       ls.comm ? ls.comm->owner_mask() : (const int8_t*)nullptr, (const double*)d_tab.p, tab_lds_words(), hyst_args());
}
template <class MS> void BlackoilDevice::assemble_kernels(double dt, bool initial, MS* A, bool props_only)
{
    const Plan& P = ls.plan;
    const double* sc = prm.matbalscale;
    // CPR: k_assemble_rows also writes the weights of the pressure equation (the device well model redoes those of its perforated cells after
    // its diagonal contributions, wells_assemble; explicit host well cliques change off-diagonal blocks: the solver's own pass then)
    MS* wout = nullptr;
    if (prm.use_cpr && (nperf == 0 || device_wells) && ls.cpr_weight_mode == 0 && ls.emulate_ranks <= 1) { ls.ensure_work<MS>(); ls.work<MS>().cprw.alloc(3 * size_t(P.nbp)); wout = ls.work<MS>().cprw.p; }
    hipEvent_t kt_a = ls.kt.begin();
    launch_cell_values();
    ls.kt.end(KT_CELL_PROPS, kt_a);
    if (props_only) return;
    KtScope kts(ls.kt, KT_FLUX);
    // Two concluded experiments fixed the shapes (asm_rows_waves, BATCH in the kernel), both measured at 100^3 on the default model:
    //  - 3 waves per SIMD (168 VGPRs, 7 spilled, 56 B of scratch per lane) against 2 (173 VGPRs, none spilled): 0.232 against 0.240 ms with
    //    a double Jacobian, 0.181 against 0.206 ms with a float one (profiles/r03_asm_waves_ab.log).  The dual-write, Stone and oil-water
    //    shapes were never tuned: 2 waves;
    //  - all ten neighbour values in one batch against the upwind-dependent five on demand: 0.202 against 0.211 ms with a double Jacobian
    //    (profiles/r03_asm_batch_ab.log).  Untried on the shapes that read the tables from the blob: those keep the on-demand loads.
    // mixed precision: the float copy of a DOUBLE Jacobian is written in the same pass (A/B: OPMGPU_MIXED_DUALWRITE=0 converts before the solve)
    static const bool dual = env_flag("OPMGPU_MIXED_DUALWRITE", true);
    float* a32 = nullptr;
    if (dual && sizeof(MS) == 8 && prm.preconditioner_single && !props_only && ls.emulate_ranks <= 1 && !(prm.use_cpr && prm.cpr_reference_transform)) { a32 = ls.matrix_f(); dual_written = true; }
    auto kern = assemble_rows_kernel<MS>(tab_lds_words() > 0, a32 != nullptr, kmodel());
    hipLaunchKernelGGL(kern, dim3(grid8_for(nc)), dim3(kBlock), tab_lds_bytes(), stream, xcd_mode(), nc, P.nbp, dto_, d_pvtnum.p, d_satnum.p, d_pv.p,
                       d_p.p, d_sw.p, d_sg.p, d_rs.p, d_rv.p, d_hc.p, 1.0 / dt, int(initial), sc[0], sc[1], sc[2],
                       ls.dp.slice_ptr.p, ls.dp.col.p, ls.dp.rowlen.p, ls.dp.nlower.p, ls.dp.tpos.p, d_tr_e.p, (const double*)d_zc.p, gravity, use_thpres ? d_thp_e.p : (const double*)nullptr,
                       eps_planes(), d_eps_u0.p, d_somax.p, (const double*)d_vals.p, d_accum0.p, ls.comm ? ls.comm->owner_mask() : (const int8_t*)nullptr, d_R.p, A, wout,
                       (const int32_t*)ls.dp.flux_perm.p, (const double*)d_tab.p, tab_lds_words(), hyst_args(), a32);
    ls.weights_from_assembly = wout != nullptr;
}

// The Jacobian is written in the precision of the coming solve (opmgpu_set_solve_precision): float saves the f64 -> f32 copy
// of the whole matrix and half of the assembly's write traffic.  The host-well path adds f64 blocks, so it keeps the double matrix.
void BlackoilDevice::assemble(double dt, bool initial)
{
    well_words_valid = false; well_red_valid = false;
    last_dt = dt;
    has_rhs_extra = false;
    if (initial) { d_dx_old.zero(stream); ls.new_step_hint = true; }       // first matrix of a time step: coarse AMG operators are rebuilt
    const bool host_wells = nperf > 0 && !device_wells;
    ls.corr_policy.external = false;           // a matrix of the model's own assembly: the correction-factor policy may score its time steps
    ls.float_copy_valid = false;               // (mixed precision: the float copy of the previous matrix is stale)
    dual_written = false;
    ls.coarse_single_ok = nperf == 0;          // no wells of either kind: the global constant is the near-null-space vector
    ls.matrix_is_float = assemble_single && !host_wells;
    if (prm.update_equations_scaling) {
        // updateEquationsScaling (BlackoilModelBase_impl.hpp:919-947; default off): every equation scaled by the mean 1/b of its phase in the
        // state being assembled.  The reference sets it at the end of assemble() and its linear solver scales this assembly's system with
        // it; here the scaling is applied while the Jacobian is written, so the mean is taken first: one extra property pass (it fills
        // d_bpart), the three sums, then the assembly proper with the new factors (wells and right-hand side read prm.matbalscale too).
        if (ls.matrix_is_float) assemble_kernels<float>(dt, initial, ls.matrix_f(), true);
        else assemble_kernels<double>(dt, initial, ls.matrix_d(), true);
        double B[3];
        average_b(B);
        for (int a = 0; a < 3; ++a) { prm.matbalscale[a] = B[a]; ls.lowrank.scale[a] = B[a]; }      // the wells' bordered pressure column is built from the same factors (k_cpr_border)
    }
    const bool forked = wells_prologue_async(initial);
    if (ls.matrix_is_float) assemble_kernels<float>(dt, initial, ls.matrix_f());
    else assemble_kernels<double>(dt, initial, ls.matrix_d());
    if (forked) OPMGPU_HIP(hipStreamWaitEvent(stream, ev_well[1], 0));
    {
        KtScope kts(ls.kt, KT_WELLS);
        wells_assemble(initial);
        aquifer_assemble();          // (nothing without aquifers or before a step has begun)
    }
    // the matrix is final (the host well model, if any, adds its blocks later: not then): the solver may start its ILU0 factorisation now
    // (LinSolver::factor_ahead decides).  What only the model can do for it comes first: the float copy that came with the assembly gets the
    // wells' diagonal contributions, which followed it
    ls.factor_ahead(prm, host_wells, [&] {
        if (!dual_written || ls.matrix_is_float) return;
        if (device_wells && nperf > 0)
            hipLaunchKernelGGL(k_refresh_f32_diag, dim3(grid_for(nperf)), dim3(kBlock), 0, stream, nperf, (const int32_t*)d_perf_cells.p, ls.dp.slice_ptr.p, ls.dp.nlower.p,
                               (const double*)ls.matrix_d(), ls.matrix_f());
        const int32_t* aq_rows = nullptr;                  // the aquifers' connected rows likewise
        if (const int naq_rows = aquifer_rows(&aq_rows))
            hipLaunchKernelGGL(k_refresh_f32_diag, dim3(grid_for(naq_rows)), dim3(kBlock), 0, stream, naq_rows, aq_rows, ls.dp.slice_ptr.p, ls.dp.nlower.p,
                               (const double*)ls.matrix_d(), ls.matrix_f());
        ls.float_copy_valid = true;
    });
}

int BlackoilDevice::convergence(double dt, double* B3, double* CNV3, double* MB3, double* linf3, int* converged)
{
    const Plan& P = ls.plan;
    const int g = std::min(grid_for(nc), kMaxRedBlocks);
    const int8_t* mask = ls.comm ? ls.comm->owner_mask() : nullptr;
    hipEvent_t kt_a = ls.kt.begin();
    hipLaunchKernelGGL(k_conv_partial, dim3(g), dim3(kBlock), 0, stream, nc, P.nbp, d_R.p, (const double*)d_bpart.p, grid_for(nc), d_pv.p, mask, d_red.p + kRedPart);
    hipLaunchKernelGGL(k_conv_final, dim3(13), dim3(kBlock), 0, stream, g, d_red.p + kRedPart, d_red.p);
    ls.kt.end(KT_CONV, kt_a);
    // decomposed run with device wells somewhere: their convergence maxima (flux equations, control equation, error marks) ride on the same
    // max-all-reduce in the slots 13..18 -- well_convergence() then needs neither its own all-reduce nor a stream synchronisation
    const bool wells_ride = ls.comm && has_device_wells();
    if (wells_ride) well_conv_pack(d_red.p + 13);
    if (ls.comm) {
        // sums (7) and maxima (6 + the wells' 6) in ONE all-reduce: every rank places its numbers in its own slot of a zeroed
        // [ranks][nv] table, the table is sum-all-reduced (= gathered), and every rank reduces the columns itself in rank order --
        // the same bits everywhere, and one small-message latency (~13 us over RCCL) instead of two per Newton iteration
        const int nv = wells_ride ? 19 : 13, nr = ls.comm->num_ranks();
        d_gather.ensure(size_t(nr) * 19);
        hipLaunchKernelGGL(k_conv_gather, dim3(1), dim3(kBlock), 0, stream, 0, nv, nr, ls.comm->my_rank(), d_red.p, d_gather.p);
        ls.comm->allreduce_sum(d_gather.p, nr * nv, stream);
        hipLaunchKernelGGL(k_conv_gather, dim3(1), dim3(kBlock), 0, stream, 1, nv, nr, ls.comm->my_rank(), d_red.p, d_gather.p);
    }
    // (polled host-mapped copy: no stream synchronisation); the device wells' residuals and error flags come along for well_convergence()
    const void *we = nullptr, *wf = nullptr; int nwe = 0;
    const bool with_wells = !ls.comm && well_words_sources(we, nwe, wf) && 26 + nwe + 1 <= LinSolver::kPubWords;
    const uint32_t* h = with_wells ? ls.fetch_words(d_red.p, 26, we, nwe, wf, 1) : ls.fetch_words(d_red.p, wells_ride ? 38 : 26);
    std::memcpy(h_red, h, (wells_ride ? 19 : 13) * sizeof(double));
    well_red_valid = wells_ride;
    well_words_valid = with_wells;
    if (with_wells) well_words.assign(h + 26, h + 26 + nwe + 1);
    bool conv = true; int status = OPMGPU_OK;
    const double ncg = ls.comm ? double(ls.comm->n_owned_global) : double(nc);
    const double pvs = ls.comm ? pvsum_global : pvsum;
    if (h_red[6] != 0.0) status = OPMGPU_ENUMERICAL;                                    // non-finite residual, :1562-1566
    for (int a = 0; a < 3; ++a) {
        const double B = h_red[a] / ncg;
        const double cnv = B * dt * h_red[7 + a], mb = std::fabs(B * h_red[3 + a]) * dt / pvs;
        if (B3) B3[a] = B; if (CNV3) CNV3[a] = cnv; if (MB3) MB3[a] = mb; if (linf3) linf3[a] = h_red[10 + a];
        conv = conv && (mb < prm.tolerance_mb) && (cnv < prm.tolerance_cnv);
        if (std::isnan(mb) || std::isnan(cnv)) status = OPMGPU_ENUMERICAL;              // :1828-1836
        if (mb > prm.max_residual_allowed || cnv > prm.max_residual_allowed) status = OPMGPU_ENUMERICAL;   // :1837-1845
    }
    if (converged) *converged = conv ? 1 : 0;
    return status;
}

// relativeChange (BlackoilModelBase_impl.hpp:1595-1631): partial sums of |p0-p|^2 + |s0-s|^2 and |p|^2 + |s|^2, owned rows
__global__ __launch_bounds__(kBlock) void k_relchange_partial(int nb, const double* __restrict__ p, const double* __restrict__ sw,
                                                              const double* __restrict__ so, const double* __restrict__ sg,
                                                              const double* __restrict__ p0, const double* __restrict__ sw0,
                                                              const double* __restrict__ so0, const double* __restrict__ sg0,
                                                              const int8_t* __restrict__ mask, double* __restrict__ part)
{
    __shared__ double sm[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double vals[2] = { 0.0, 0.0 };
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < nb; i += long(gridDim.x) * kBlock) {
        if (mask && !mask[i]) continue;
        const double a = p[i], b = sw[i], c = so[i], d = sg[i];
        const double da = p0[i] - a, db = sw0[i] - b, dc = so0[i] - c, dd = sg0[i] - d;
        vals[0] += da * da + (db * db + dc * dc + dd * dd);
        vals[1] += a * a + (b * b + c * c + d * d);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const double s = wave_sum(vals[q]);
        __syncthreads();
        if (lane == 0) sm[w] = s;
        __syncthreads();
        if (threadIdx.x == 0) part[long(q) * gridDim.x + blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    }
}
__global__ __launch_bounds__(kBlock) void k_sum2_final(int nblocks, const double* __restrict__ part, double* __restrict__ out)
{
    __shared__ double sm[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int q = 0; q < 2; ++q) {
        double v = 0.0;
        for (int i = threadIdx.x; i < nblocks; i += kBlock) v += part[long(q) * nblocks + i];
        const double s = wave_sum(v);
        __syncthreads();
        if (lane == 0) sm[w] = s;
        __syncthreads();
        if (threadIdx.x == 0) out[q] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    }
}

// device-side copy of the reservoir state: what AdaptiveTimeStepping keeps as last_state (AdaptiveTimeStepping_impl.hpp:211-212)
void BlackoilDevice::save_state()
{
    const size_t nbp = size_t(ls.plan.nbp);
    d_saved.alloc(6 * nbp); d_saved_hc.alloc(nbp);
    DevArray<double>* planes[] = { &d_p, &d_sw, &d_so, &d_sg, &d_rs, &d_rv };
    for (int k = 0; k < 6; ++k) OPMGPU_HIP(hipMemcpyAsync(d_saved.p + size_t(k) * nbp, planes[k]->p, nbp * sizeof(double), hipMemcpyDeviceToDevice, stream));
    OPMGPU_HIP(hipMemcpyAsync(d_saved_hc.p, d_hc.p, nbp, hipMemcpyDeviceToDevice, stream));
    wells_save();
    has_saved = true;
}
void BlackoilDevice::restore_state()
{
    const size_t nbp = size_t(ls.plan.nbp);
    DevArray<double>* planes[] = { &d_p, &d_sw, &d_so, &d_sg, &d_rs, &d_rv };
    for (int k = 0; k < 6; ++k) OPMGPU_HIP(hipMemcpyAsync(planes[k]->p, d_saved.p + size_t(k) * nbp, nbp * sizeof(double), hipMemcpyDeviceToDevice, stream));
    OPMGPU_HIP(hipMemcpyAsync(d_hc.p, d_saved_hc.p, nbp, hipMemcpyDeviceToDevice, stream));
    wells_restore();
    aquifer_discard();          // a begun aquifer step belongs to the sub-step that failed; the committed aquifer state is not touched
}
double BlackoilDevice::relative_change()
{
    const size_t nbp = size_t(ls.plan.nbp);
    const int g = std::min(grid_for(nc), kMaxRedBlocks);
    const int8_t* mask = ls.comm ? ls.comm->owner_mask() : nullptr;
    hipLaunchKernelGGL(k_relchange_partial, dim3(g), dim3(kBlock), 0, stream, nc, d_p.p, d_sw.p, d_so.p, d_sg.p, d_saved.p, d_saved.p + nbp,
                       d_saved.p + 2 * nbp, d_saved.p + 3 * nbp, mask, d_red.p + kRedPart);
    hipLaunchKernelGGL(k_sum2_final, dim3(1), dim3(kBlock), 0, stream, g, d_red.p + kRedPart, d_red.p);
    if (ls.comm) ls.comm->allreduce_sum(d_red.p, 2, stream);
    OPMGPU_HIP(hipMemcpyAsync(h_red, d_red.p, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
    return h_red[1] > 0.0 ? h_red[0] / h_red[1] : 0.0;
}

// multi-GPU: the communicator knows rank-local caller numbering; (re)derive internal rows + global sums
void BlackoilDevice::attach_comm(CommBase* c, int n_owned)
{
    if (shared_well_rows() > 0) throw HipError(OPMGPU_EINVAL, "multi-GPU: a cell is perforated by several wells; a decomposed run (a communicator is attached) does not support that");
    ls.comm = c;
    n_owned_cells = n_owned;
    for (int32_t pc : h_well_cells) if (device_wells && pc >= n_owned) throw HipError(OPMGPU_EINVAL, "multi-GPU: a well perforates a ghost cell; keep every well on one rank");
    double loc[2] = { 0.0, double(n_owned) };
    for (int i = 0; i < n_owned; ++i) loc[0] += h_pv[i];
    OPMGPU_HIP(hipMemcpyAsync(d_red.p, loc, 2 * sizeof(double), hipMemcpyHostToDevice, stream));
    c->allreduce_sum(d_red.p, 2, stream);
    OPMGPU_HIP(hipMemcpyAsync(h_red, d_red.p, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
    pvsum_global = h_red[0];
    c->n_owned_global = int(h_red[1] + 0.5);
}

void BlackoilDevice::perf_props_device()
{
    if (nperf == 0) return;
    hipLaunchKernelGGL(OPMGPU_BY_MODEL(k_perf_props), dim3(grid_for(nperf)), dim3(kBlock), 0, stream, nperf, dtp_, d_perf_cells.p, cell_planes(), d_perf.p);
}

void BlackoilDevice::perf_pvt_device(const double* press_dev, double* out_dev, const int32_t* gate)
{
    if (nperf == 0) return;
    hipLaunchKernelGGL(k_perf_pvt, dim3(grid_for(nperf)), dim3(kBlock), 0, stream, nperf, dtp_, d_perf_cells.p, d_pvtnum.p, d_so.p, d_rs.p, d_rv.p, d_hc.p,
                       d_somax.p, press_dev, gate, out_dev);
}

// sum of 1/b per phase over the owned cells (-> B_avg of getWellConvergence) into out_dev[0..2] (sums; the caller divides by the cell count)
void BlackoilDevice::binv_sums_device(double* out13_dev, double* scratch_dev)
{
    const Plan& P = ls.plan;
    const int g = std::min(grid_for(nc), kMaxRedBlocks);
    const int8_t* mask = ls.comm ? ls.comm->owner_mask() : nullptr;
    hipLaunchKernelGGL(k_conv_partial, dim3(g), dim3(kBlock), 0, stream, nc, P.nbp, d_R.p, (const double*)d_bpart.p, grid_for(nc), d_pv.p, mask, scratch_dev);
    hipLaunchKernelGGL(k_conv_final, dim3(13), dim3(kBlock), 0, stream, g, scratch_dev, out13_dev);
    if (ls.comm) ls.comm->allreduce_sum(out13_dev, 3, stream);
}

void BlackoilDevice::average_b(double* B3)
{
    DevArray<double> out, scratch; out.alloc(16); scratch.alloc(13 * size_t(kMaxRedBlocks));
    binv_sums_device(out.p, scratch.p);
    double h[3];
    OPMGPU_HIP(hipMemcpyAsync(h, out.p, 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
    const double ncg = ls.comm ? double(ls.comm->n_owned_global) : double(nc);
    for (int a = 0; a < 3; ++a) B3[a] = h[a] / ncg;
}

int BlackoilDevice::add_well_terms(const double* resid_delta, int nblk, const int32_t* rc, const double* blocks)
{
    const Plan& P = ls.plan;
    const double* sc = prm.matbalscale;
    if (nperf > 0 && resid_delta) {
        DevArray<double> dd; dd.upload(resid_delta, 3 * size_t(nperf), stream);
        hipLaunchKernelGGL(k_add_well_resid, dim3(grid_for(nperf)), dim3(kBlock), 0, stream, nperf, P.nbp, d_perf_cells.p, dd.p, d_R.p);
        OPMGPU_HIP(hipStreamSynchronize(stream));
    }
    if (nblk > 0) {
        std::vector<int32_t> ent(nblk);
        for (int k = 0; k < nblk; ++k) {
            const int r = rc[2 * k], c = rc[2 * k + 1];
            if (r < 0 || r >= nc) return OPMGPU_EINVAL;
            const int32_t* b = P.col.data() + P.rowptr[r]; const int32_t* e = P.col.data() + P.rowptr[r + 1];
            const int32_t* it = std::lower_bound(b, e, c);
            if (it == e || *it != c) return OPMGPU_EINVAL;
            ent[k] = P.entry_of_block[it - P.col.data()];
        }
        DevArray<int32_t> de; de.upload(ent, stream);
        DevArray<double> db; db.upload(blocks, 9 * size_t(nblk), stream);
        hipLaunchKernelGGL(k_add_well_blocks, dim3(grid_for(nblk)), dim3(kBlock), 0, stream, nblk, de.p, db.p, sc[0], sc[1], sc[2], ls.matrix_d());
        OPMGPU_HIP(hipStreamSynchronize(stream));
    }
    return OPMGPU_OK;
}

__global__ __launch_bounds__(kBlock) void k_f2d(long n, const float* __restrict__ a, double* __restrict__ b)
{
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) b[i] = double(a[i]);
}
void launch_convert_f2d(long n, const float* a, double* b, hipStream_t s)
{
    hipLaunchKernelGGL(k_f2d, dim3(std::min(grid_for(n), kMaxRedBlocks)), dim3(kBlock), 0, s, n, a, b);
}

void BlackoilDevice::add_well_rhs(const double* rhs_delta)
{
    if (nperf == 0) return;
    const Plan& P = ls.plan;
    d_rhs_extra.alloc(3 * size_t(P.nbp));
    d_rhs_extra.zero(stream);
    DevArray<double> dd; dd.upload(rhs_delta, 3 * size_t(nperf), stream);
    hipLaunchKernelGGL(k_add_well_resid, dim3(grid_for(nperf)), dim3(kBlock), 0, stream, nperf, P.nbp, d_perf_cells.p, dd.p, d_rhs_extra.p);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    has_rhs_extra = true;
}

void BlackoilDevice::perf_dx(double* out)
{
    if (nperf == 0) return;
    hipLaunchKernelGGL(k_gather_perf3, dim3(grid_for(nperf)), dim3(kBlock), 0, stream, nperf, ls.plan.nbp, d_perf_cells.p, d_dx.p, d_perf.p);
    OPMGPU_HIP(hipMemcpyAsync(out, d_perf.p, size_t(nperf) * 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

template <class S> void BlackoilDevice::build_rhs()
{
    const Plan& P = ls.plan;
    const double* sc = prm.matbalscale;
    hipLaunchKernelGGL((k_build_rhs<S>), dim3(grid_for(nc)), dim3(kBlock), 0, stream, nc, P.nbp, sc[0], sc[1], sc[2], d_R.p,
                       has_rhs_extra ? d_rhs_extra.p : (const double*)nullptr, ls.work<S>().b.p);
}
template <class S> void BlackoilDevice::store_dx()
{
    const Plan& P = ls.plan;
    const long n = 3 * long(P.nbp);
    if (sizeof(S) == 8) {
        // (the GMRES combination stored the solution here already when it was handed d_dx as its mirror: LinSolver::solution_mirror)
        if (!ls.mirror_written) OPMGPU_HIP(hipMemcpyAsync(d_dx.p, ls.work<S>().x.p, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    } else {
        launch_convert_f2d(n, reinterpret_cast<const float*>(ls.work<S>().x.p), d_dx.p, stream);
    }
    has_dx = true;
}
template void BlackoilDevice::build_rhs<float>();
template void BlackoilDevice::build_rhs<double>();
template void BlackoilDevice::store_dx<float>();
template void BlackoilDevice::store_dx<double>();

void BlackoilDevice::dx_to_host(double* dx)
{
    ls.vec_to_host<double>(d_dx.p, VEC_EQUATION_MAJOR, dx);
}

void BlackoilDevice::update_state(const double* dx_host, double relax)
{
    const Plan& P = ls.plan;
    if (dx_host) { ls.vec_from_host<double>(dx_host, VEC_EQUATION_MAJOR, d_dx.p); OPMGPU_HIP(hipStreamSynchronize(stream)); has_dx = true; }   // caller's buffer: done with it on return
    KtScope kts(ls.kt, KT_UPDATE_STATE);
    if (device_wells) wells_update(relax, dx_host != nullptr);          // updateWellState from the recovered (and possibly relaxed) well increment
    auto kern = drdt_on() ? (tab_lds_words() > 0 ? k_update_state<true, true> : k_update_state<false, true>)
                          : (tab_lds_words() > 0 ? k_update_state<true, false> : k_update_state<false, false>);
    hipLaunchKernelGGL(kern, dim3(grid_for(nc)), dim3(kBlock), tab_lds_bytes(), stream, nc, P.nbp, dto_, d_pvtnum.p, d_satnum.p, d_dx.p, relax,
                       prm.dp_max_rel, prm.ds_max, prm.dr_max_rel, d_p.p, d_sw.p, d_so.p, d_sg.p, d_rs.p, d_rv.p, d_hc.p, eps_planes(), d_eps_u0.p, d_somax.p,
                       (const double*)d_tab.p, tab_lds_words());
}

__global__ __launch_bounds__(kBlock) void k_somax_update(int nb, const double* __restrict__ so, double* __restrict__ somax)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nb) somax[i] = fmax(somax[i], so[i]);
}

void BlackoilDevice::update_sat_oil_max()
{
    hipLaunchKernelGGL(k_somax_update, dim3(grid_for(nc)), dim3(kBlock), 0, stream, nc, d_so.p, d_somax.p);
}
void BlackoilDevice::set_sat_oil_max(const double* v)
{
    const Plan& P = ls.plan;
    std::vector<double> h(P.nbp, 0.0);
    for (int r = 0; r < nc; ++r) h[r] = v[P.nat[r]];
    d_somax.upload(h, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
}
void BlackoilDevice::get_sat_oil_max(double* v)
{
    const Plan& P = ls.plan;
    std::vector<double> h(P.nbp);
    OPMGPU_HIP(hipMemcpyAsync(h.data(), d_somax.p, size_t(P.nbp) * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
    for (int r = 0; r < nc; ++r) v[P.nat[r]] = h[r];
}

// ---- DRSDT / DRVDT: the dissolution limits (the rule is stated in include/opmgpu.h at opmgpu_set_dissolution_limits) -----------------------
// The caps of a time step from the resident state, one thread per cell: rs_cap = rs + d_s (+inf where free_only and the cell holds no
// free gas, or the rate is off), rv_cap = rv + d_v.  d_s = a_s dt and d_v = a_v dt are formed once on the host; the sum is ONE rounding
// (an addition alone: nothing to contract into an FMA), so a float64 restatement on the host matches bit for bit.
__global__ __launch_bounds__(kBlock) void k_dissolution_caps(int nb, const double* __restrict__ rs, const double* __restrict__ rv, const double* __restrict__ sg,
                                                            int on_s, int free_only, double d_s, int on_v, double d_v,
                                                            double* __restrict__ rs_cap, double* __restrict__ rv_cap)
{
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nb) return;
    const double inf = __builtin_inf();
    rs_cap[c] = (on_s && !(free_only && sg[c] == 0.0)) ? rs[c] + d_s : inf;
    rv_cap[c] = on_v ? rv[c] + d_v : inf;
}
// d_somax with (so_max | rs_cap | rv_cap) or without the planes of the caps, so_max kept; new caps are +inf (padding rows included).
// A context with rock regions (never one with caps) has two planes, so_max | p_min, a new p_min +inf likewise.
void BlackoilDevice::resize_somax(bool with_caps)
{
    const size_t nbp = size_t(ls.plan.nbp), planes = with_caps ? 3 : (rock_on() ? 2 : 1);
    if (d_somax.n == planes * nbp) return;
    OPMGPU_HIP(hipStreamSynchronize(stream));        // no kernel in flight reads the array that is replaced
    std::vector<double> h(3 * nbp, std::numeric_limits<double>::infinity());
    d_somax.download(h.data(), nbp, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    d_somax.alloc(planes * nbp);
    d_somax.upload(h.data(), d_somax.n, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
}
void BlackoilDevice::set_dissolution_limits(double a_s, int free_only, double a_v)
{
    const char* who = "opmgpu_set_dissolution_limits: ";
    if (std::isnan(a_s) || std::isinf(a_s)) throw HipError(OPMGPU_EINVAL, std::string(who) + "drsdt is not finite");
    if (std::isnan(a_v) || std::isinf(a_v)) throw HipError(OPMGPU_EINVAL, std::string(who) + "drvdt is not finite");
    const bool on_s = a_s >= 0.0, on_v = a_v >= 0.0;
    if (on_s || on_v) {
        if (oil_water()) throw HipError(OPMGPU_EINVAL, std::string(who) + "the context has no gas phase (OPMGPU_PHASES_OIL_WATER)");
        if (dtp_.x.oil_pvcdo) throw HipError(OPMGPU_EINVAL, std::string(who) + "the context has the analytic dead oil (opmgpu_set_pvcdo); dissolution limits are not supported with it");
        if (on_s && !dto_.t.has_disgas) throw HipError(OPMGPU_EINVAL, std::string(who) + "drsdt needs dissolved gas (has_disgas)");
        if (on_v && !dto_.t.has_vapoil) throw HipError(OPMGPU_EINVAL, std::string(who) + "drvdt needs vaporised oil (has_vapoil)");
        if (ls.comm) throw HipError(OPMGPU_EINVAL, std::string(who) + "a communicator is attached; a decomposed run does not support dissolution limits");
        if (rock_on()) throw HipError(OPMGPU_EINVAL, std::string(who) + "the context has rock regions (opmgpu_set_rock_regions); dissolution limits are not supported with them");
    }
    drsdt = on_s ? a_s : -1.0; drsdt_free_only = on_s && free_only != 0; drvdt = on_v ? a_v : -1.0;
    resize_somax(drdt_on());
}
void BlackoilDevice::begin_dissolution_step(double dt)
{
    const char* who = "opmgpu_begin_dissolution_step: ";
    if (!drdt_on()) throw HipError(OPMGPU_EINVAL, std::string(who) + "no dissolution limit is set (opmgpu_set_dissolution_limits)");
    if (!(dt > 0.0) || std::isinf(dt)) throw HipError(OPMGPU_EINVAL, std::string(who) + "dt is not positive and finite");
    if (!has_state) throw HipError(OPMGPU_EINVAL, std::string(who) + "no state is resident (opmgpu_set_state)");
    const size_t nbp = size_t(ls.plan.nbp);
    const double d_s = drsdt >= 0.0 ? drsdt * dt : 0.0, d_v = drvdt >= 0.0 ? drvdt * dt : 0.0;
    hipLaunchKernelGGL(k_dissolution_caps, dim3(grid_for(nc)), dim3(kBlock), 0, stream, nc, (const double*)d_rs.p, (const double*)d_rv.p, (const double*)d_sg.p,
                       int(drsdt >= 0.0), int(drsdt_free_only), d_s, int(drvdt >= 0.0), d_v, d_somax.p + nbp, d_somax.p + 2 * nbp);
}
// the caps in the caller's cell order (restart, tests); either pointer may be null.  Without limits there are no caps: +inf, and nothing to set
void BlackoilDevice::get_dissolution_caps(double* rs_cap, double* rv_cap)
{
    const Plan& P = ls.plan;
    const size_t nbp = size_t(P.nbp);
    std::vector<double> h(2 * nbp, std::numeric_limits<double>::infinity());
    if (drdt_on()) { OPMGPU_HIP(hipMemcpyAsync(h.data(), d_somax.p + nbp, 2 * nbp * sizeof(double), hipMemcpyDeviceToHost, stream)); OPMGPU_HIP(hipStreamSynchronize(stream)); }
    for (int r = 0; r < nc; ++r) { if (rs_cap) rs_cap[P.nat[r]] = h[r]; if (rv_cap) rv_cap[P.nat[r]] = h[nbp + r]; }
}
void BlackoilDevice::set_dissolution_caps(const double* rs_cap, const double* rv_cap)
{
    if (!drdt_on()) throw HipError(OPMGPU_EINVAL, "opmgpu_set_dissolution_caps: no dissolution limit is set (opmgpu_set_dissolution_limits)");
    const Plan& P = ls.plan;
    const size_t nbp = size_t(P.nbp);
    const double* src[2] = { rs_cap, rv_cap };
    for (int k = 0; k < 2; ++k) {
        if (!src[k]) continue;
        for (int c = 0; c < nc; ++c) if (std::isnan(src[k][c])) throw HipError(OPMGPU_EINVAL, "opmgpu_set_dissolution_caps: a cap is NaN");
    }
    std::vector<double> h(nbp, std::numeric_limits<double>::infinity());
    for (int k = 0; k < 2; ++k) {
        if (!src[k]) continue;
        for (int r = 0; r < nc; ++r) h[r] = src[k][P.nat[r]];
        OPMGPU_HIP(hipMemcpyAsync(d_somax.p + (1 + k) * nbp, h.data(), nbp * sizeof(double), hipMemcpyHostToDevice, stream));
        OPMGPU_HIP(hipStreamSynchronize(stream));
    }
}

// ---- rock regions and irreversible compaction (the rule is stated in include/opmgpu.h at opmgpu_set_rock_regions) ---------------------------
// The regions' tables ride in the blob behind everything else (upload_rock_tables), rocknum behind satnum and p_min behind so_max
// (rocknum_of / rock_pmin_of): no kernel has an argument more, and only the KM_ROCK instantiations read any of it.  The two kernels of
// the history and of the multipliers are in blackoil_output.hip.
void BlackoilDevice::set_rock_regions(const opmgpu_rock_regions* s)
{
    const std::string who = "opmgpu_set_rock_regions: ";
    auto bad = [&](const std::string& what) { return HipError(OPMGPU_EINVAL, who + what); };
    if (!s) {
        if (!rock_on()) return;
        OPMGPU_HIP(hipStreamSynchronize(stream));
        h_rocknum.clear(); h_rock_ptr.clear(); h_rock_ref.clear(); h_rock_tab.clear(); rock_mode = OPMGPU_ROCK_REVERSIBLE;
        upload_rock_tables();
        upload_region_numbers();
        resize_somax(drdt_on());
        return;
    }
    // everything is checked before anything changes: a refused set leaves the previous one in force
    if (s->nregions < 1) throw bad("nregions is smaller than 1");
    if (s->mode != OPMGPU_ROCK_REVERSIBLE && s->mode != OPMGPU_ROCK_IRREVERSIBLE) throw bad("unknown mode " + std::to_string(s->mode));
    if (!s->rocknum || !s->rock_pref || !s->rock_comp || !s->tab_ptr) throw bad("rocknum, rock_pref, rock_comp or tab_ptr is NULL");
    const int nr = s->nregions;
    if (s->tab_ptr[0] != 0) throw bad("tab_ptr does not start at 0");
    for (int r = 0; r < nr; ++r) {
        const int n = s->tab_ptr[r + 1] - s->tab_ptr[r];
        if (n < 0) throw bad("tab_ptr decreases at region " + std::to_string(r));
        if (n == 1) throw bad("the table of region " + std::to_string(r) + " has exactly 1 row (0 = the ROCK form, else at least 2)");
    }
    const int rows = s->tab_ptr[nr];
    if (rows > 0 && (!s->tab_p || !s->tab_pvmult || !s->tab_transmult)) throw bad("tab_p, tab_pvmult or tab_transmult is NULL");
    for (int c = 0; c < nc; ++c)
        if (s->rocknum[c] < 0 || s->rocknum[c] >= nr) throw bad("rocknum of cell " + std::to_string(c) + " is outside [0, nregions)");
    for (int r = 0; r < nr; ++r) {
        if (!std::isfinite(s->rock_pref[r]) || !std::isfinite(s->rock_comp[r])) throw bad("rock_pref or rock_comp of region " + std::to_string(r) + " is not finite");
        for (int i = s->tab_ptr[r]; i < s->tab_ptr[r + 1]; ++i) {
            const std::string at = "row " + std::to_string(i - s->tab_ptr[r]) + " of the table of region " + std::to_string(r);
            if (!std::isfinite(s->tab_p[i]) || !std::isfinite(s->tab_pvmult[i]) || !std::isfinite(s->tab_transmult[i])) throw bad(at + " has an entry that is not finite");
            if (!(s->tab_pvmult[i] > 0.0)) throw bad("pv_mult in " + at + " is not positive");
            if (s->tab_transmult[i] < 0.0) throw bad("trans_mult in " + at + " is negative");
            if (i > s->tab_ptr[r] && !(s->tab_p[i] > s->tab_p[i - 1])) throw bad("p in " + at + " is not above the row before it (strictly increasing)");
        }
    }
    if (dtp_.x.oil_pvcdo) throw bad("the context has the analytic dead oil (opmgpu_set_pvcdo); rock regions are not supported with it");
    if (drdt_on()) throw bad("the context has dissolution limits (opmgpu_set_dissolution_limits); rock regions are not supported with them");
    // the history lasts through a new set of regions (a schedule may change them); the first set starts it at +inf
    OPMGPU_HIP(hipStreamSynchronize(stream));
    h_rocknum.assign(s->rocknum, s->rocknum + nc);
    h_rock_ptr.assign(s->tab_ptr, s->tab_ptr + nr + 1);
    h_rock_ref.resize(2 * size_t(nr));
    for (int r = 0; r < nr; ++r) { h_rock_ref[2 * size_t(r)] = s->rock_pref[r]; h_rock_ref[2 * size_t(r) + 1] = s->rock_comp[r]; }
    // five planes p | pv_mult | slopes | trans_mult | slopes; a slope is the segment's, formed once here by the IEEE division
    const size_t m = size_t(std::max(rows, 1));
    h_rock_tab.assign(5 * m, 0.0);
    for (int i = 0; i < rows; ++i) { h_rock_tab[i] = s->tab_p[i]; h_rock_tab[m + i] = s->tab_pvmult[i]; h_rock_tab[3 * m + i] = s->tab_transmult[i]; }
    for (int r = 0; r < nr; ++r)
        for (int i = s->tab_ptr[r]; i + 1 < s->tab_ptr[r + 1]; ++i) {
            const double h = s->tab_p[i + 1] - s->tab_p[i];
            h_rock_tab[2 * m + i] = (s->tab_pvmult[i + 1] - s->tab_pvmult[i]) / h;
            h_rock_tab[4 * m + i] = (s->tab_transmult[i + 1] - s->tab_transmult[i]) / h;
        }
    rock_mode = s->mode;
    upload_rock_tables();
    upload_region_numbers();
    resize_somax(false);
}
// the blob as upload_tables formed it, with the regions' arrays behind it when there are regions (never together with PVCDO rows)
void BlackoilDevice::upload_rock_tables()
{
    std::vector<double> blob = h_tab;
    opmgpu_tables& t = dto_.t;
    t.rock_pref = plain_rock_.rock_pref; t.rock_comp = plain_rock_.rock_comp; t.rocktab_n = plain_rock_.rocktab_n;
    t.rocktab_p = plain_rock_.rocktab_p; t.rocktab_pvmult = plain_rock_.rocktab_pvmult; t.rocktab_transmult = plain_rock_.rocktab_transmult;
    if (rock_on()) {        // the rock fields carry the regions (RockView, fluid_eval.hpp); word offsets like every pointer of dto_
        const size_t np = h_rock_ptr.size();
        t.rocktab_transmult = reinterpret_cast<const double*>(blob.size());
        blob.resize(blob.size() + (np + 1) / 2, 0.0);
        std::memcpy(&blob[blob.size() - (np + 1) / 2], h_rock_ptr.data(), np * sizeof(int32_t));
        t.rocktab_pvmult = reinterpret_cast<const double*>(blob.size());
        blob.insert(blob.end(), h_rock_ref.begin(), h_rock_ref.end());
        t.rocktab_p = reinterpret_cast<const double*>(blob.size());
        blob.insert(blob.end(), h_rock_tab.begin(), h_rock_tab.end());
        t.rocktab_n = int32_t(h_rock_tab.size() / 5); t.rock_pref = 0.0; t.rock_comp = double(rock_mode);
    }
    OPMGPU_HIP(hipStreamSynchronize(stream));        // no kernel in flight reads the blob that upload may replace
    upload_blob(blob);
}
// d_satnum for the current plan: the saturation regions and, with rock regions, the rock regions behind them (internal numbering)
void BlackoilDevice::upload_region_numbers()
{
    const Plan& P = ls.plan;
    const size_t nbp = size_t(P.nbp);
    std::vector<int32_t> sn((rock_on() ? 2 : 1) * nbp, 0);
    for (int r = 0; r < nc; ++r) { sn[r] = h_satnum[P.nat[r]]; if (rock_on()) sn[nbp + r] = h_rocknum[P.nat[r]]; }
    OPMGPU_HIP(hipStreamSynchronize(stream));
    d_satnum.alloc(sn.size());
    d_satnum.upload(sn, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
}
// p_min in the caller's cell order (restart, tests); +inf without regions
void BlackoilDevice::get_rock_history(double* p_min)
{
    const Plan& P = ls.plan;
    const size_t nbp = size_t(P.nbp);
    std::vector<double> h(nbp, std::numeric_limits<double>::infinity());
    if (rock_on()) { OPMGPU_HIP(hipMemcpyAsync(h.data(), d_somax.p + nbp, nbp * sizeof(double), hipMemcpyDeviceToHost, stream)); OPMGPU_HIP(hipStreamSynchronize(stream)); }
    for (int r = 0; r < nc; ++r) p_min[P.nat[r]] = h[r];
}
void BlackoilDevice::set_rock_history(const double* p_min)
{
    if (!rock_on()) throw HipError(OPMGPU_EINVAL, "opmgpu_set_rock_history: no rock regions are set (opmgpu_set_rock_regions)");
    if (!p_min) throw HipError(OPMGPU_EINVAL, "opmgpu_set_rock_history: p_min is NULL");
    for (int c = 0; c < nc; ++c) if (std::isnan(p_min[c])) throw HipError(OPMGPU_EINVAL, "opmgpu_set_rock_history: p_min of cell " + std::to_string(c) + " is NaN");
    const Plan& P = ls.plan;
    const size_t nbp = size_t(P.nbp);
    std::vector<double> h(nbp, std::numeric_limits<double>::infinity());
    for (int r = 0; r < nc; ++r) h[r] = p_min[P.nat[r]];
    OPMGPU_HIP(hipMemcpyAsync(d_somax.p + nbp, h.data(), nbp * sizeof(double), hipMemcpyHostToDevice, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

void BlackoilDevice::stabilize_update(int relax_type, double omega)
{
    // dampening by 1 changes nothing, and the previous increment (dx_old) is only ever read by the SOR form: no launch then.  (A run
    // uses one relaxation type throughout -- NonlinearSolver's parameter --, so SOR never meets a dx_old that was skipped here.)
    if (relax_type != OPMGPU_RELAX_SOR && omega == 1.0) return;
    const long n = 3 * long(ls.plan.nbp);
    if (device_wells) wells_stabilize(relax_type == OPMGPU_RELAX_SOR ? 1 : 0, omega);      // the well part first: it is recovered from the UNRELAXED dx
    hipLaunchKernelGGL(k_stabilize, dim3(unsigned((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, n, relax_type == OPMGPU_RELAX_SOR ? 1 : 0, omega,
                       d_dx.p, d_dx_old.p);
}

} // namespace opmgpu
