// wells.hip -- standard well model on the device.
//
// Restates, per well and without leaving the GPU, what Opm::StandardWells does with AutoDiffBlocks:
//   computeWellFlux                    opm/autodiff/StandardWells_impl.hpp:396-571
//   addWellFluxEq / addWellControlEq   :806-829 / :836-998   (BHP and SURFACE_RATE controls, dead wells)
//   updateWellState                    :611-650              computeWellConnectionPressures :223-298
//   WellDensitySegmented               WellDensitySegmented.cpp:66-181
//   addWellContributionToMassBalanceEq opm/autodiff/BlackoilModelBase_impl.hpp:953-975
//   eliminateVariable / recoverVariable opm/autodiff/NewtonIterationUtilities.cpp:45-184
// Difference by design: the reference forms the Schur complement S = A - B D^-1 C explicitly, which fills the reservoir
// matrix with a dense clique per well.  Here the same reduced system is kept in factored form: the perforated cells' own
// derivatives go into the diagonal blocks, everything that couples different perforations of a well is a rank-7 operator
// P_w Q_w (3 mixture fractions + 4 well unknowns) applied matrix-free by the solver (LowRankOp, linsolver.hpp).
// One workgroup per well; derivatives by a small forward-AD type (the work is O(nperf), AD costs nothing here).
// Round 2: the control logic of the reference runs on the device too --
//   updateWellControls / updateWellStateWithTarget   StandardWells_impl.hpp:709-800 / :1452-1550   (k_well_controls)
//   solveWellEq (explicit well pre-solve, default on) BlackoilModelBase_impl.hpp:1018-1133          (k_well_presolve_fused / _serial / k_well_assemble<PRE> + k_well_presolve_step)
//   THP control through VFP tables                   :655-700, :895-960; VFPProd/InjPropertiesLegacy.cpp   (vfp_* of vfp.hpp)
//   PVT at the average well-block pressure           :218-296                                       (k_well_avg_press + k_perf_pvt)
//   RESERVOIR_RATE conversion coefficients          RateConverterLegacy.hpp:495-548, :718-768        (k_voidage_coeff, region_state_sums in blackoil_output.hip)
//   well efficiency factors (WEFAC)                 StandardWells_impl.hpp:1405-1434; BlackoilModelBase_impl.hpp:953-975   (WellArgs::eff, k_well_assemble)
//   group rate control shared by guide rates        BlackoilModelBase_impl.hpp:779-792, :1090-1093 call it; WellCollection / WellsGroup are
//                                                   opm-core and not in the reference tree: the sharing rule is OURS, stated at
//                                                   opmgpu_set_well_groups in include/opmgpu.h   (k_group_targets, group_targets_dev)
// Not restated: GEFAC, group modes other than a surface rate, nested targets.
#include "blackoil.hpp"
#include "vfp.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

namespace opmgpu {

namespace {

template <int N> struct Du { double v; double d[N]; };

template <int N> __device__ __forceinline__ Du<N> du_const(double v) { Du<N> r; r.v = v; for (int i = 0; i < N; ++i) r.d[i] = 0.0; return r; }
template <int N> __device__ __forceinline__ Du<N> du_var(double v, int k) { Du<N> r = du_const<N>(v); r.d[k] = 1.0; return r; }
template <int N> __device__ __forceinline__ Du<N> operator+(const Du<N>& a, const Du<N>& b) { Du<N> r; r.v = a.v + b.v; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
template <int N> __device__ __forceinline__ Du<N> operator-(const Du<N>& a, const Du<N>& b) { Du<N> r; r.v = a.v - b.v; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
template <int N> __device__ __forceinline__ Du<N> operator*(const Du<N>& a, const Du<N>& b) { Du<N> r; r.v = a.v * b.v; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b.v + b.d[i] * a.v; return r; }
template <int N> __device__ __forceinline__ Du<N> operator/(const Du<N>& a, const Du<N>& b) { Du<N> r; r.v = a.v / b.v; for (int i = 0; i < N; ++i) r.d[i] = (a.d[i] - b.d[i] * r.v) / b.v; return r; }
template <int N> __device__ __forceinline__ Du<N> operator*(double s, const Du<N>& a) { Du<N> r; r.v = s * a.v; for (int i = 0; i < N; ++i) r.d[i] = s * a.d[i]; return r; }
template <int N> __device__ __forceinline__ Du<N> operator-(double s, const Du<N>& a) { Du<N> r; r.v = s - a.v; for (int i = 0; i < N; ++i) r.d[i] = -a.d[i]; return r; }

// perforation property k of OPMGPU_PERF_K (value, d/dP, d/dSw, d/dXvar) as a dual over the first three variables
template <int N> __device__ __forceinline__ Du<N> perf_q(const double* __restrict__ pp, int k)
{
    Du<N> r = du_const<N>(pp[4 * k]);
    r.d[0] = pp[4 * k + 1]; r.d[1] = pp[4 * k + 2]; r.d[2] = pp[4 * k + 3];
    return r;
}

// variables: 0..2 = (P, Sw, Xvar) of the perforated cell, 3 = bhp, 4..6 = mixture fractions (only with N == 7)
template <int N> struct PerfFlux { Du<N> cq_ps[3]; Du<N> cqt_i; };

template <int N>
__device__ void perf_flux(const double* __restrict__ pp, double bhp_v, double cdp, double Tw, bool sel_inj, bool sel_prod, PerfFlux<N>& f)
{
    const Du<N> p = perf_q<N>(pp, 0), rs = perf_q<N>(pp, 1), rv = perf_q<N>(pp, 2);
    const Du<N> b[3] = { perf_q<N>(pp, 3), perf_q<N>(pp, 4), perf_q<N>(pp, 5) };
    const Du<N> mob[3] = { perf_q<N>(pp, 6), perf_q<N>(pp, 7), perf_q<N>(pp, 8) };
    Du<N> bhp = du_var<N>(bhp_v, 3);
    const Du<N> drawdown = p - (bhp + du_const<N>(cdp));
    const double sp = sel_prod ? Tw : 0.0, si = sel_inj ? Tw : 0.0;
    for (int a = 0; a < 3; ++a) f.cq_ps[a] = b[a] * ((-sp) * (mob[a] * drawdown));           // :457-463, flow INTO the wellbore
    const Du<N> oil = f.cq_ps[1], gas = f.cq_ps[2];
    f.cq_ps[2] = f.cq_ps[2] + rs * oil;                                                         // :466-474
    f.cq_ps[1] = f.cq_ps[1] + rv * gas;
    f.cqt_i = (-si) * ((mob[0] + mob[1] + mob[2]) * drawdown);                                  // :481-486, flow OUT of the wellbore
}


// ---- VFP tables on the device (THP control): the evaluators vfp_bhp / vfp_thp and the table layout live in vfp.hpp ------------

struct WellArgs {
    int nbp;
    const int32_t *connpos, *perf_row, *type, *allow_cf, *ctrl_type;
    const double *WI, *comp_frac, *ctrl_distr, *depth_ref, *z_perf, *surf_dens_perf;
    double* ctrl_target;         // [nctrl]; written by group_targets_dev alone (the group slots), read by everything else
    const int32_t *ctrl_ptr, *ctrl_vfp, *thp_ctrl;       // controls of well w: [ctrl_ptr[w], ctrl_ptr[w+1]); VFP table INDEX per control (-1); first THP control of the well (-1)
    const double* ctrl_alq;
    int32_t* current;            // [nw] currentControls(): index relative to ctrl_ptr[w]
    double* thp;                 // [nw]
    double* perf_dens;           // [nperf] well_perforation_densities_
    const double* perf_pvt;      // [nperf][5] b_w b_o b_g rsSat rvSat at the average well-block pressure (k_perf_pvt)
    double* wdy;                 // [nw][4] recovered Newton increment of the well unknowns
    double* ctrl_row;            // [nw][4] d control equation / d (qs, bhp)
    VfpArgs V;
    double gravity;
    const double* perf;          // [nperf][OPMGPU_PERF_K]
    double* wstate;              // [nw][4] qs(3), bhp
    double* cdp;                 // [nperf]
    double* perf_rates;          // [nperf][3]
    double* perf_press;          // [nperf]
    double* P; double* Q;        // [nperf][21]
    double* Fsave;               // [nperf][9+9+3]: F_i, M_i, fb_i
    double* wellE;               // [nw][4]
    double* Dinv;                // [nw][16]
    const double* eff;           // [nw] well efficiency factor e_w in (0, 1] (ones by default): weighs what the CELLS see of the well, never the well equations
    // rows perforated by several wells: perf_of_row[row] = the row's FIRST (lowest-index) perforation or -1, perf_next[j] = the next
    // perforation of the same row or -1.  A perforation of such a row leaves the row's R, diagonal block and rhs_extra to k_well_shared_rows,
    // which sums the wells' terms in ascending perforation index; bde[nperf][3] = its B_i D^-1 E (unweighted) for that kernel.
    // perf_shared[j] != 0: perforation j shares its row (one load next to perf_row[j], nothing that waits for the row).
    const int32_t *perf_of_row, *perf_next, *perf_well, *perf_shared;
    double* bde;
    // controlled groups (opmgpu_set_well_groups; ngroups == 0: none, nothing below is read): members of group g =
    // group_wells[group_ptr[g] .. group_ptr[g + 1]), guide rates in the same positions; group_rate[g] = the members' weighted rate sum
    int ngroups;
    const int32_t *group_ptr, *group_wells;
    const double *group_sign, *group_target, *group_distr, *group_guide;
    double* group_rate;
};

// average well-block pressure per perforation (computePropertiesForWellConnectionPressures, StandardWells_impl.hpp:228-237):
// mean of the perforation's pressure and the one above it (bhp for the first), both from the WELL STATE
__global__ void k_well_avg_press(int nw, WellArgs A, const int32_t* __restrict__ gate, double* __restrict__ avg)
{
    if (gate && !*gate) return;
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    for (int perf = A.connpos[w]; perf < A.connpos[w + 1]; ++perf) {
        const double p_above = perf == A.connpos[w] ? A.wstate[4 * w + 3] : A.perf_press[perf - 1];
        avg[perf] = (A.perf_press[perf] + p_above) / 2;
    }
}

// computeWellConnectionPressures: WellDensitySegmented::computeConnectionDensities + computeConnectionPressureDelta.  One wavefront per
// well: the lanes stage a tile of perforation data in LDS with parallel loads, lane 0 then walks the tile in the reference's order (the
// running sums are sequential by definition; a thread fetching every perforation's operands itself spends 1.6 us per perforation waiting
// for them: 164 us for a 100-perforation well, 8x this version).
// qout[nperf][3]: q_out of every perforation, filled bottom to top EXACTLY as the reference does.  The segment below the lowest flowing
// perforation must carry a flow of exactly 0.0 (its mixture is then the well's comp_frac, WellDensitySegmented.cpp:103-109): a total taken
// at the top and reduced on the way down leaves rounding residue there, and with it the mixture of that residue.
// A well's part of qout is written and read back by that well's workgroup alone: the barrier between the two passes orders it.
constexpr int kCdpTile = 128;
__global__ __launch_bounds__(64) void k_well_cdp(int nw, WellArgs A, double gravity, const int32_t* __restrict__ gate, double* __restrict__ qout)
{
    __shared__ double s_rate[3 * kCdpTile], s_pvt[5 * kCdpTile], s_sd[3 * kCdpTile], s_z[kCdpTile], s_dens[kCdpTile], s_cdp[kCdpTile];
    if (gate && !*gate) return;
    const int w = blockIdx.x, lane = threadIdx.x;
    if (w >= nw) return;
    const int lo = A.connpos[w], hi = A.connpos[w + 1];
    // q_out[perf] = flow out of the segment above perforation perf = sum_{k >= perf} (-rate_k), from the bottom up
    // (WellDensitySegmented.cpp:83-95): q_out[perf] = q_out[perf + 1] - rate[perf], 0.0 below the last one
    {
        double q[3] = { 0.0, 0.0, 0.0 };
        for (int t1 = hi; t1 > lo; t1 -= kCdpTile) {
            const int t0 = t1 - kCdpTile > lo ? t1 - kCdpTile : lo, nt = t1 - t0;
            for (int i = lane; i < 3 * nt; i += 64) s_rate[i] = A.perf_rates[3 * long(t0) + i];
            __syncthreads();
            if (lane == 0) for (int i = nt - 1; i >= 0; --i) for (int a = 0; a < 3; ++a) { q[a] -= s_rate[3 * i + a]; s_sd[3 * i + a] = q[a]; }
            __syncthreads();
            for (int i = lane; i < 3 * nt; i += 64) qout[3 * long(t0) + i] = s_sd[i];
            __syncthreads();
        }
    }
    double run = 0.0, z_above = A.depth_ref[w];
    for (int t0 = lo; t0 < hi; t0 += kCdpTile) {
        const int nt = hi - t0 < kCdpTile ? hi - t0 : kCdpTile;
        for (int i = lane; i < 3 * nt; i += 64) { s_rate[i] = qout[3 * long(t0) + i]; s_sd[i] = A.surf_dens_perf[3 * long(t0) + i]; }
        for (int i = lane; i < 5 * nt; i += 64) s_pvt[i] = A.perf_pvt[5 * long(t0) + i];
        for (int i = lane; i < nt; i += 64) s_z[i] = A.z_perf[t0 + i];
        __syncthreads();
        if (lane == 0) {
            for (int i = 0; i < nt; ++i) {
                const double* pv = s_pvt + 5 * i;
                const double* q = s_rate + 3 * i;
                const double tot = q[0] + q[1] + q[2];
                double mix[3], x[3];
                for (int a = 0; a < 3; ++a) { mix[a] = tot != 0.0 ? fabs(q[a] / tot) : A.comp_frac[3 * w + a]; x[a] = mix[a]; }
                const double rsmax = pv[3], rvmax = pv[4];
                double rs = 0.0, rv = 0.0;
                if (mix[1] > 0.0) rs = fmin(mix[2] / mix[1], rsmax);
                if (mix[2] > 0.0) rv = fmin(mix[1] / mix[2], rvmax);
                if (rs != 0.0) x[2] = (mix[2] - mix[1] * rs) / (1.0 - rs * rv);
                if (rv != 0.0) x[1] = (mix[1] - mix[2] * rv) / (1.0 - rs * rv);
                const double volrat = x[0] / pv[0] + x[1] / pv[1] + x[2] / pv[2];
                const double* sd = s_sd + 3 * i;
                const double dens = (sd[0] * mix[0] + sd[1] * mix[1] + sd[2] * mix[2]) / volrat;
                s_dens[i] = dens;
                run += (s_z[i] - z_above) * dens * gravity;
                z_above = s_z[i];
                s_cdp[i] = run;
            }
        }
        __syncthreads();
        for (int i = lane; i < nt; i += 64) { A.perf_dens[t0 + i] = s_dens[i]; A.cdp[t0 + i] = s_cdp[i]; }
        __syncthreads();
    }
}

// ---- control logic shared by k_well_controls and the pre-solve ---------------------------------------------------------------
// wellhelpers::computeHydrostaticCorrection with the density of the well's first perforation
__device__ __forceinline__ double vfp_dp(const WellArgs& A, int w, int t)
{
    if (A.connpos[w + 1] == A.connpos[w]) return 0.0;
    return A.perf_dens[A.connpos[w]] * A.gravity * (A.V.datum[t] - A.depth_ref[w]);
}
// updateWellStateWithTarget (StandardWells_impl.hpp:1452-1550)
__device__ void well_apply_target(const WellArgs& A, int w, int c)
{
    const int typ = A.ctrl_type[c];
    const double target = A.ctrl_target[c];
    double* ws = A.wstate + 4 * w;
    if (typ == OPMGPU_CTRL_BHP) ws[3] = target;
    else if (typ == OPMGPU_CTRL_THP) {
        const int t = A.ctrl_vfp[c];
        const double q[3] = { ws[0], ws[1], ws[2] };
        ws[3] = vfp_bhp(A.V, t, q, target, A.ctrl_alq[c], nullptr) - vfp_dp(A, w, t);
    } else if (typ == OPMGPU_CTRL_SURFACE_RATE) {
        const double* distr = A.ctrl_distr + 3 * c;
        if (A.type[w] == 0) { for (int a = 0; a < 3; ++a) if (A.comp_frac[3 * w + a] > 0.0) ws[a] = target * A.comp_frac[3 * w + a]; }
        else {
            int n = 0;
            for (int a = 0; a < 3; ++a) n += distr[a] > 0.0 ? 1 : 0;
            if (n < 2) for (int a = 0; a < 3; ++a) if (distr[a] > 0.0) ws[a] = target * distr[a];
        }
    }
}
// wellhelpers::constraintBroken (opm-simulators WellHelpers.hpp): injectors break a limit from above, producers from below
__device__ bool well_constraint_broken(const WellArgs& A, int w, int c)
{
    const int typ = A.ctrl_type[c];
    const double target = A.ctrl_target[c];
    const double* ws = A.wstate + 4 * w;
    double val;
    if (typ == OPMGPU_CTRL_BHP) val = ws[3];
    else if (typ == OPMGPU_CTRL_THP) val = A.thp[w];
    else { const double* d = A.ctrl_distr + 3 * c; val = ws[0] * d[0] + ws[1] * d[1] + ws[2] * d[2]; }
    return A.type[w] == 0 ? val > target : val < target;
}
// updateWellControls for one well (:709-800); returns false when no consistent control is found within 2 * ncontrols rounds
__device__ bool well_update_controls(const WellArgs& A, int w)
{
    const int c0 = A.ctrl_ptr[w], nwc = A.ctrl_ptr[w + 1] - c0;
    int current = A.current[w], rounds = 0;
    for (;;) {
        well_apply_target(A, w, c0 + current);
        int broken = -1;
        for (int k = 0; k < nwc; ++k) if (k != current && well_constraint_broken(A, w, c0 + k)) { broken = k; break; }
        if (broken >= 0) { current = broken; A.current[w] = current; }
        ++rounds;
        if (rounds > 2 * nwc) return false;
        if (broken < 0) return true;
    }
}
// updateWellState for one well (:611-700): rates, limited bhp, thp of a well that has a THP control
__device__ void well_apply_increment(const WellArgs& A, int w, const double dy[4], double dbhp_max_rel)
{
    double* ws = A.wstate + 4 * w;
    for (int a = 0; a < 3; ++a) ws[a] -= dy[a];
    const double d = dy[3], bhp = ws[3];
    const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    ws[3] = bhp - sg * fmin(fabs(d), fabs(bhp) * dbhp_max_rel);
    const int tc = A.thp_ctrl[w];
    if (tc >= 0) {
        const int t = A.ctrl_vfp[tc];
        const double q[3] = { ws[0], ws[1], ws[2] };
        A.thp[w] = vfp_thp(A.V, t, q, ws[3] + vfp_dp(A, w, t), A.ctrl_alq[tc]);
    }
}

// ---- group rate control: the slot targets of one controlled group (the rule: opmgpu_set_well_groups, include/opmgpu.h) ----------
// Called by ALL kBlock threads of a workgroup.  The three sums of the group -- guide rates of the wells on their slot, weighted rates of
// the wells under individual control, weighted rates of all members -- are taken per thread over a fixed stride and then through
// block_sum's fixed tree: no atomics, the same bits in every run, any group size.  What the calling workgroup wrote to wstate / current
// before must be behind a __syncthreads(); the function ends with one, so the targets are visible to the workgroup on return.
__device__ void group_targets_dev(const WellArgs& A, int g)
{
    __shared__ double gsm[12];
    __shared__ double gtot[3];
    const int tid = threadIdx.x;
    const int lo = A.group_ptr[g], hi = A.group_ptr[g + 1];
    const double sg = A.group_sign[g], T = A.group_target[g];
    const double d0 = A.group_distr[3 * g], d1 = A.group_distr[3 * g + 1], d2 = A.group_distr[3 * g + 2];
    double acc[3] = { 0.0, 0.0, 0.0 };          // Gamma = sum of gamma over C; sum of r over I; sum of r over all members
    for (int i = lo + tid; i < hi; i += kBlock) {
        const int w = A.group_wells[i];
        const double* ws = A.wstate + 4 * w;
        const double r = A.eff[w] * (d0 * ws[0] + d1 * ws[1] + d2 * ws[2]);
        if (A.current[w] != A.ctrl_ptr[w + 1] - A.ctrl_ptr[w] - 1) acc[1] += r; else acc[0] += A.group_guide[i];
        acc[2] += r;
    }
    block_sum<3>(acc, gsm);
    if (tid == 0) { gtot[0] = acc[0]; gtot[1] = acc[1]; gtot[2] = acc[2]; A.group_rate[g] = acc[2]; }
    __syncthreads();
    const double Gamma = gtot[0], RI = gtot[1];
    for (int i = lo + tid; i < hi; i += kBlock) {
        const int w = A.group_wells[i];
        const double* ws = A.wstate + 4 * w;
        const double e = A.eff[w], gam = A.group_guide[i];
        const int slot = A.ctrl_ptr[w + 1] - 1;
        double share, rem;
        if (A.current[w] != slot - A.ctrl_ptr[w]) {     // under individual control: what the well would get if it joined
            const double r = e * (d0 * ws[0] + d1 * ws[1] + d2 * ws[2]);
            share = gam / (gam + Gamma); rem = T - sg * (RI - r);
        } else { share = gam / Gamma; rem = T - sg * RI; }
        A.ctrl_target[slot] = sg * share * fmax(0.0, rem) / e;
    }
    __syncthreads();
}
// one workgroup per controlled group
__global__ __launch_bounds__(kBlock) void k_group_targets(WellArgs A) { group_targets_dev(A, blockIdx.x); }

// flags[]: 0 = error bits (WE_*), 1 = pre-solve done, 2 = pre-solve converged, 3 = pre-solve iterations
enum { WF_ERR = 0, WF_DONE, WF_CONV, WF_ITS, WF_COUNT };
// error bits: singular D of a well; updateWellControls found no consistent control; NaN / too large well residual in the pre-solve; the
// fused pre-solve's barrier gave up (presolve_barrier raises it, k_well_presolve_serial consumes it).  All but the first are what the
// reference reports as a NumericalIssue.
enum { WE_SINGULAR = 2, WE_NO_CONTROL = 4, WE_BAD_RESIDUAL = 8, WE_BARRIER = 16, WE_NUMERICAL = WE_NO_CONTROL | WE_BAD_RESIDUAL | WE_BARRIER };

__global__ void k_well_controls(int nw, WellArgs A, int32_t* __restrict__ flags)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    if (!well_update_controls(A, w)) atomicOr(&flags[WF_ERR], WE_NO_CONTROL);
}

// 4x4 inverse with partial pivoting (D of one well); returns false when singular
__device__ bool inv4(const double* m, double* out)
{
    double a[4][8];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { a[i][j] = m[4 * i + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
    for (int p = 0; p < 4; ++p) {
        int piv = p;
        for (int i = p + 1; i < 4; ++i) if (fabs(a[i][p]) > fabs(a[piv][p])) piv = i;
        if (a[piv][p] == 0.0) return false;
        if (piv != p) for (int j = 0; j < 8; ++j) { const double t = a[p][j]; a[p][j] = a[piv][j]; a[piv][j] = t; }
        const double d = 1.0 / a[p][p];
        for (int j = 0; j < 8; ++j) a[p][j] *= d;
        for (int i = 0; i < 4; ++i) if (i != p) { const double f = a[i][p]; for (int j = 0; j < 8; ++j) a[i][j] -= f * a[p][j]; }
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) out[4 * i + j] = a[i][4 + j];
    return true;
}

// well equations + reduced (Schur) contributions of one well by one workgroup.  PRE = the explicit well pre-solve (solveWellEq,
// BlackoilModelBase_impl.hpp:1043-1062): the reservoir is frozen, only E and D^-1 of the well are formed (nothing is written to the
// reservoir system).  Eout: where the four well-equation residuals go (PRE + published: agent-scope stores, read by other workgroups).
template <class MS, bool PRE>
__device__ void well_assemble_dev(const WellArgs& A, int w, const int32_t* __restrict__ slice_ptr, const int16_t* __restrict__ nlower,
                                  double s0, double s1, double s2, double* __restrict__ R, MS* __restrict__ Amat,
                                  double* __restrict__ rhs_extra, int32_t* __restrict__ flags, double* Eout, bool publish)
{
    __shared__ double sm[64];
    __shared__ int any_flag[2];
    __shared__ double wl[64];         // well-level values shared by all threads
    const int tid = threadIdx.x;
    const int lo = A.connpos[w], hi = A.connpos[w + 1];
    const double qs[3] = { A.wstate[4 * w], A.wstate[4 * w + 1], A.wstate[4 * w + 2] };
    const double bhp = A.wstate[4 * w + 3];
    const double compi[3] = { A.comp_frac[3 * w], A.comp_frac[3 * w + 1], A.comp_frac[3 * w + 2] };
    // well efficiency factor (addWellContributionToMassBalanceEq subtracts efficiency_factors * cq_s): it weighs the cell rows -- R, the
    // diagonal blocks, P, rhs_extra -- and nothing of the well equations.  e_w = 1 gives the unweighted bits (1 * x is exact).
    const double ew = PRE ? 1.0 : A.eff[w];
    const double escale[3] = { ew * s0, ew * s1, ew * s2 };
    // ---- phase 0: which perforations inject (drawdown < 0), cross-flow rule (:418-452) ----
    if (tid < 2) any_flag[tid] = 0;
    __syncthreads();
    for (int j = lo + tid; j < hi; j += kBlock) {
        const double dd = A.perf[long(j) * OPMGPU_PERF_K] - (bhp + A.cdp[j]);
        atomicOr(&any_flag[dd < 0.0 ? 0 : 1], 1);
    }
    __syncthreads();
    const bool any_inj = any_flag[0] != 0, any_prod = any_flag[1] != 0;
    const bool kill_prod = !A.allow_cf[w] && A.type[w] == 0 && any_inj;          // injector: no producing perforations
    const bool kill_inj = !A.allow_cf[w] && A.type[w] == 1 && any_prod && !kill_prod;
    // ---- phase A: sums of cq_ps and of d cq_ps / d bhp ----
    double acc[6] = { 0, 0, 0, 0, 0, 0 };
    for (int j = lo + tid; j < hi; j += kBlock) {
        const double* pp = A.perf + long(j) * OPMGPU_PERF_K;
        const double dd = pp[0] - (bhp + A.cdp[j]);
        const bool si = dd < 0.0 && !kill_inj, sp = !(dd < 0.0) && !kill_prod;
        PerfFlux<4> f;
        perf_flux<4>(pp, bhp, A.cdp[j], A.WI[j], si, sp, f);
        for (int a = 0; a < 3; ++a) { acc[a] += f.cq_ps[a].v; acc[3 + a] += f.cq_ps[a].d[3]; }
    }
    block_sum<6>(acc, sm);
    // ---- phase B: mixture in the wellbore (:489-519) ----
    if (tid == 0) {
        double wbq[3], wbqt = 0.0, inj[3], dinj[3];
        for (int a = 0; a < 3; ++a) { inj[a] = qs[a] > 0.0 ? qs[a] : 0.0; dinj[a] = qs[a] > 0.0 ? 1.0 : 0.0; wbq[a] = compi[a] * inj[a] - acc[a]; wbqt += wbq[a]; }
        const bool alive = wbqt != 0.0;
        double Sb = acc[3] + acc[4] + acc[5];
        for (int a = 0; a < 3; ++a) {
            const double cm = alive ? wbq[a] / wbqt : compi[a];
            wl[a] = cm;
            for (int b = 0; b < 3; ++b)       // g_q[a][b] = d cmix_a / d qs_b
                wl[3 + 3 * a + b] = alive ? ((a == b ? compi[b] * dinj[b] : 0.0) - cm * compi[b] * dinj[b]) / wbqt : 0.0;
            wl[12 + a] = alive ? (-acc[3 + a] + cm * Sb) / wbqt : 0.0;      // g_b[a] = d cmix_a / d bhp
        }
        wl[15] = alive ? 1.0 : 0.0;
        wl[16] = wbqt;
    }
    __syncthreads();
    const double cmix[3] = { wl[0], wl[1], wl[2] };
    const bool alive = wl[15] != 0.0;
    const double wbqt = wl[16];
    // ---- phase C: component rates per perforation with all partials; residual, diagonal blocks, sums ----
    double acc2[15];
    for (int k = 0; k < 15; ++k) acc2[k] = 0.0;          // 0..2 sum cq_s, 3..11 sum M, 12..14 sum fb
    for (int j = lo + tid; j < hi; j += kBlock) {
        const double* pp = A.perf + long(j) * OPMGPU_PERF_K;
        const double dd = pp[0] - (bhp + A.cdp[j]);
        const bool si = dd < 0.0 && !kill_inj, sp = !(dd < 0.0) && !kill_prod;
        PerfFlux<7> f;
        perf_flux<7>(pp, bhp, A.cdp[j], A.WI[j], si, sp, f);
        const Du<7> rs = perf_q<7>(pp, 1), rv = perf_q<7>(pp, 2);
        const Du<7> b[3] = { perf_q<7>(pp, 3), perf_q<7>(pp, 4), perf_q<7>(pp, 5) };
        const Du<7> cm[3] = { du_var<7>(cmix[0], 4), du_var<7>(cmix[1], 5), du_var<7>(cmix[2], 6) };
        const Du<7> d = 1.0 - rv * rs;
        const Du<7> vol = cm[0] / b[0] + ((cm[1] - rv * cm[2]) / d) / b[1] + ((cm[2] - rs * cm[1]) / d) / b[2];     // :521-551
        const Du<7> cqt_is = f.cqt_i / vol;
        Du<7> cq_s[3];
        for (int a = 0; a < 3; ++a) cq_s[a] = f.cq_ps[a] + cm[a] * cqt_is;                                          // :553-560
        const int row = A.perf_row[j];
        const bool shared = !PRE && A.perf_shared[j] != 0;
        if (PRE) {
            for (int a = 0; a < 3; ++a) {
                A.perf_rates[3 * j + a] = cq_s[a].v;                                 // updatePerfPhaseRatesAndPressures (:1059)
                acc2[a] += cq_s[a].v;
                acc2[12 + a] += cq_s[a].d[3];
                for (int v = 0; v < 3; ++v) acc2[3 + 3 * a + v] += cq_s[a].d[4 + v];
            }
            A.perf_press[j] = bhp + A.cdp[j];
            continue;
        }
        MS* dptr = Amat + long(slice_ptr[row >> 6] + nlower[row]) * 576 + (row & 63);
        double* Qj = A.Q + 21 * long(j); double* Fs = A.Fsave + 21 * long(j);
        // H = d cq_ps / d cell, G = d cmix / d cell = (-H + cmix (1^T H)) / wbqt
        for (int v = 0; v < 3; ++v) {
            const double hs = f.cq_ps[0].d[v] + f.cq_ps[1].d[v] + f.cq_ps[2].d[v];
            for (int a = 0; a < 3; ++a) Qj[3 * a + v] = alive ? (-f.cq_ps[a].d[v] + cmix[a] * hs) / wbqt : 0.0;
        }
        for (int a = 0; a < 3; ++a) {
            if (!shared) R[long(a) * A.nbp + row] -= ew * cq_s[a].v;                 // addWellContributionToMassBalanceEq
            A.perf_rates[3 * j + a] = cq_s[a].v;
            acc2[a] += cq_s[a].v;
            acc2[12 + a] += cq_s[a].d[3];
            Fs[18 + a] = cq_s[a].d[3];
            for (int v = 0; v < 3; ++v) {
                if (!shared) dptr[(3 * a + v) * 64] = MS(double(dptr[(3 * a + v) * 64]) - escale[a] * cq_s[a].d[v]);   // own-cell part of -e_w d cq_s / d cell
                Fs[3 * a + v] = cq_s[a].d[v];
                Fs[9 + 3 * a + v] = cq_s[a].d[4 + v];
                acc2[3 + 3 * a + v] += cq_s[a].d[4 + v];
            }
        }
        A.perf_press[j] = bhp + A.cdp[j];
    }
    __syncthreads();
    block_sum<15>(acc2, sm);
    // ---- phase D: well equations E, D = dE/d(qs, bhp), D^-1 ----
    if (tid == 0) {
        const double* gq = wl + 3; const double* gb = wl + 12;
        const double* Ms = acc2 + 3; const double* fbs = acc2 + 12;
        double D[16], E[4];
        for (int a = 0; a < 3; ++a) {
            E[a] = qs[a] - acc2[a];                                                  // addWellFluxEq
            for (int b = 0; b < 3; ++b) {
                double mg = 0.0;
                for (int c = 0; c < 3; ++c) mg += Ms[3 * a + c] * gq[3 * c + b];
                D[4 * a + b] = (a == b ? 1.0 : 0.0) - mg;
            }
            double mgb = 0.0;
            for (int c = 0; c < 3; ++c) mgb += Ms[3 * a + c] * gb[c];
            D[4 * a + 3] = -(fbs[a] + mgb);
        }
        // addWellControlEq (:836-998) for the well's CURRENT control: dead well -> sum of rates; BHP; THP through the VFP table; rate
        const int cc = A.ctrl_ptr[w] + A.current[w];
        const int ctyp = A.ctrl_type[cc];
        if (!alive) { E[3] = qs[0] + qs[1] + qs[2]; D[12] = 1.0; D[13] = 1.0; D[14] = 1.0; D[15] = 0.0; }
        else if (ctyp == OPMGPU_CTRL_BHP) { E[3] = bhp - A.ctrl_target[cc]; D[12] = 0.0; D[13] = 0.0; D[14] = 0.0; D[15] = 1.0; }
        else if (ctyp == OPMGPU_CTRL_THP) {         // bhp - bhp_from_thp(qs) + dp (:944-949)
            const int t = A.ctrl_vfp[cc];
            double dq[3];
            const double bt = vfp_bhp(A.V, t, qs, A.ctrl_target[cc], A.ctrl_alq[cc], dq) - vfp_dp(A, w, t);
            E[3] = bhp - bt; D[12] = -dq[0]; D[13] = -dq[1]; D[14] = -dq[2]; D[15] = 1.0;
        } else {
            const double* ds = A.ctrl_distr + 3 * cc;
            E[3] = ds[0] * qs[0] + ds[1] * qs[1] + ds[2] * qs[2] - A.ctrl_target[cc];
            D[12] = ds[0]; D[13] = ds[1]; D[14] = ds[2]; D[15] = 0.0;
        }
        double Di[16];
        if (!inv4(D, Di)) { atomicOr(&flags[WF_ERR], WE_SINGULAR); for (int k = 0; k < 16; ++k) Di[k] = 0.0; }
        for (int k = 0; k < 16; ++k) { wl[20 + k] = Di[k]; A.Dinv[16 * w + k] = Di[k]; }
        if (!PRE) for (int k = 0; k < 4; ++k) A.ctrl_row[4 * w + k] = D[12 + k];      // gradient of the control equation (bordered pressure system, linsolver.hip)
        for (int k = 0; k < 4; ++k) {
            wl[36 + k] = E[k];
            if (publish) __hip_atomic_store(&Eout[k], E[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else Eout[k] = E[k];
        }
        for (int k = 0; k < 9; ++k) wl[40 + k] = Ms[k];
    }
    __syncthreads();
    if (PRE) return;
    // ---- phase E: P_i = -e_w [M_i | B_i D^-1], Q_i = [G_i ; C_i], rhs extra = -e_w (B_i D^-1 E) ----
    {
        const double* gq = wl + 3; const double* gb = wl + 12; const double* Di = wl + 20; const double* E = wl + 36; const double* Ms = wl + 40;
        for (int j = lo + tid; j < hi; j += kBlock) {
            const double* Fs = A.Fsave + 21 * long(j);
            const double* F = Fs; const double* M = Fs + 9; const double* fb = Fs + 18;
            double* Pj = A.P + 21 * long(j); double* Qj = A.Q + 21 * long(j);
            double B[12];                                       // B_i = -[M_i g_q | fb_i + M_i g_b]  (3 x 4)
            for (int a = 0; a < 3; ++a) {
                for (int b = 0; b < 3; ++b) { double s = 0.0; for (int c = 0; c < 3; ++c) s += M[3 * a + c] * gq[3 * c + b]; B[4 * a + b] = -s; }
                double s = 0.0; for (int c = 0; c < 3; ++c) s += M[3 * a + c] * gb[c];
                B[4 * a + 3] = -(fb[a] + s);
            }
            const int row = A.perf_row[j];
            const bool shared = A.perf_shared[j] != 0;
            for (int a = 0; a < 3; ++a) {
                double bde = 0.0;
                for (int k = 0; k < 4; ++k) {
                    double bd = 0.0;
                    for (int c = 0; c < 4; ++c) bd += B[4 * a + c] * Di[4 * c + k];
                    Pj[7 * a + 3 + k] = -escale[a] * bd;
                    bde += bd * E[k];
                }
                for (int c = 0; c < 3; ++c) Pj[7 * a + c] = -escale[a] * M[3 * a + c];
                if (shared) A.bde[3 * long(j) + a] = bde; else rhs_extra[long(a) * A.nbp + row] = -(ew * bde);
            }
            // C_i rows 0..2 = -(F_i + Ms G_i); row 3 (control equation) = 0.  G_i is already in Q rows 0..2.
            double G[9];
            for (int k = 0; k < 9; ++k) G[k] = Qj[k];
            for (int a = 0; a < 3; ++a)
                for (int v = 0; v < 3; ++v) {
                    double s = 0.0;
                    for (int c = 0; c < 3; ++c) s += Ms[3 * a + c] * G[3 * c + v];
                    Qj[9 + 3 * a + v] = -(F[3 * a + v] + s);
                }
            Qj[18] = 0.0; Qj[19] = 0.0; Qj[20] = 0.0;
        }
    }
}

template <class MS, bool PRE>
__global__ __launch_bounds__(kBlock) void k_well_assemble(WellArgs A, const int32_t* __restrict__ slice_ptr, const int16_t* __restrict__ nlower,
                                                          double s0, double s1, double s2, double* __restrict__ R, MS* __restrict__ Amat,
                                                          double* __restrict__ rhs_extra, int32_t* __restrict__ flags)
{
    if (PRE && flags[WF_DONE]) return;
    well_assemble_dev<MS, PRE>(A, blockIdx.x, slice_ptr, nlower, s0, s1, s2, R, Amat, rhs_extra, flags, A.wellE + 4 * blockIdx.x, false);
}

// Rows perforated by several wells, one thread per such row: what k_well_assemble<MS, false> writes itself for a row with one perforation,
// applied for the row's perforations in ascending perforation index from the per-perforation data the wells' workgroups left (perf_rates =
// cq_s, Fsave = F, bde = B D^-1 E).  One thread owns the row, so the order -- that of np.add.at on the restatements' side -- is fixed and
// the result the same bits in every run; no atomics.
template <class MS>
__global__ __launch_bounds__(64) void k_well_shared_rows(int nshared, const int32_t* __restrict__ shared_rows, WellArgs A, const int32_t* __restrict__ slice_ptr,
                                                         const int16_t* __restrict__ nlower, double s0, double s1, double s2, double* __restrict__ R,
                                                         MS* __restrict__ Amat, double* __restrict__ rhs_extra)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nshared) return;
    const int row = shared_rows[i];
    MS* dptr = Amat + long(slice_ptr[row >> 6] + nlower[row]) * 576 + (row & 63);
    double rx[3] = { 0.0, 0.0, 0.0 };
    for (int j = A.perf_of_row[row]; j >= 0; j = A.perf_next[j]) {
        const double ew = A.eff[A.perf_well[j]];
        const double escale[3] = { ew * s0, ew * s1, ew * s2 };
        const double* F = A.Fsave + 21 * long(j);
        for (int a = 0; a < 3; ++a) {
            R[long(a) * A.nbp + row] -= ew * A.perf_rates[3 * long(j) + a];
            for (int v = 0; v < 3; ++v) dptr[(3 * a + v) * 64] = MS(double(dptr[(3 * a + v) * 64]) - escale[a] * F[3 * a + v]);
            rx[a] += -(ew * A.bde[3 * long(j) + a]);
        }
    }
    for (int a = 0; a < 3; ++a) rhs_extra[long(a) * A.nbp + row] = rx[a];
}

// ---- the explicit well pre-solve (solveWellEq, BlackoilModelBase_impl.hpp:1018-1133) -----------------------------------------------
// Three forms of one loop -- assemble every well with the reservoir frozen, ONE convergence decision from all wells' residuals, a Newton
// step of every well -- that share the pieces below and so give the same bits (tests/test_gpu_wells.py, tests/test_gpu_well_sizes.py).
// bsums = sums of 1/b per phase, ncells = their cell count (B_avg = bsums / ncells)
struct PresolveParams { const double* bsums; double ncells, tol_wells, tol_ctrl, max_resid, dbhp_max_rel; int max_it; };

struct LoadPlain { __device__ double operator()(const double* p) const { return *p; } };
// residuals published by other workgroups of a running grid
struct LoadAgent { __device__ double operator()(const double* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } };

// getWellConvergence (:1866-1950) over the residuals E[nw][4] of all wells: B_avg * max |flux eq| < tolerance_wells and max |control eq| <
// tolerance_well_control; NaN or above max_residual_allowed is a NumericalIssue (:1909-1923).  Called by ALL threads of a workgroup, reduced
// by its first wavefront (maxima are exact: the lane count does not show in the bits).  Returns 0 continue, 1 converged, 2 numerical failure.
template <class Load>
__device__ int presolve_verdict(int nw, const double* E, const PresolveParams& S, Load load)
{
    __shared__ int verdict;
    if (threadIdx.x < 64) {
        double mx[4] = { 0, 0, 0, 0 }; int bad = 0;
        for (int v = threadIdx.x; v < nw; v += 64) for (int k = 0; k < 4; ++k) { const double e = fabs(load(&E[4 * v + k])); if (!(e == e)) bad = 1; mx[k] = fmax(mx[k], e); }
        for (int k = 0; k < 4; ++k) mx[k] = wave_max(mx[k]);
        bad = __any(bad);
        if (threadIdx.x == 0) {
            bool conv = true, toolarge = false;
            for (int a = 0; a < 3; ++a) { const double wf = (S.bsums[a] / S.ncells) * mx[a]; conv = conv && wf < S.tol_wells; toolarge = toolarge || wf > S.max_resid || !(wf == wf); }
            conv = conv && mx[3] < S.tol_ctrl;
            verdict = (bad || toolarge) ? 2 : (conv ? 1 : 0);
        }
    }
    __syncthreads();
    return verdict;
}
// y = D^-1 r of well w
__device__ __forceinline__ void well_dinv_mul(const WellArgs& A, int w, const double r[4], double y[4])
{
    const double* Di = A.Dinv + 16 * w;
    for (int k = 0; k < 4; ++k) { double d = 0.0; for (int c = 0; c < 4; ++c) d += Di[4 * k + c] * r[c]; y[k] = d; }
}
// the Newton step of one well (:1063-1097; the well equations of different wells are independent while the reservoir is frozen):
// dy = D^-1 E, updateWellState, updateWellControls
__device__ void presolve_newton_step(const WellArgs& A, int w, const double* E, double dbhp_max_rel, int32_t* __restrict__ flags)
{
    const double r[4] = { E[0], E[1], E[2], E[3] };
    double dy[4];
    well_dinv_mul(A, w, r, dy);
    well_apply_increment(A, w, dy, dbhp_max_rel);
    if (!well_update_controls(A, w)) atomicOr(&flags[WF_ERR], WE_NO_CONTROL);
}
// the end of the pre-solve after `it` steps, by ONE thread: verdict 1 or 2 of presolve_verdict, or 0 = max_it steps taken without either
__device__ void presolve_finish(int32_t* __restrict__ flags, int verdict, int it)
{
    if (verdict == 2) atomicOr(&flags[WF_ERR], WE_BAD_RESIDUAL);
    flags[WF_CONV] = verdict == 1 ? 1 : 0; flags[WF_ITS] = it; flags[WF_DONE] = 1;
}

// The well state in one place: six arrays of doubles, in the order of AdaptiveTimeStepping's saved copy (wells_saved_state), and `current`.
// The pre-solve changes four of them: its snapshot ("if (!converged) well_state = well_state0", :1124-1126) is those four in the same order,
// wstate[4 nw] | thp[nw] | perf_rates[3 np] | perf_press[np], with `current` in isnap.
constexpr int kWellStateParts = 6;
struct WellStatePart { double* p; int len; bool presolve; };
struct WellStateLayout { WellStatePart part[kWellStateParts]; };
__host__ __device__ inline WellStateLayout well_state_layout(const WellArgs& A, int nw, int np)
{
    return { { { A.wstate, 4 * nw, true }, { A.thp, nw, true }, { A.cdp, np, false }, { A.perf_rates, 3 * np, true }, { A.perf_press, np, true },
               { A.perf_dens, np, false } } };
}
// snapshot (restore: put back) of element i of every part the pre-solve changes; i runs up to max(4 nw, 3 np)
__device__ __forceinline__ void presolve_snapshot(const WellArgs& A, int nw, int np, double* __restrict__ snap, int32_t* __restrict__ isnap, bool restore, int i)
{
    const WellStateLayout L = well_state_layout(A, nw, np);
    int off = 0;
    for (int k = 0; k < kWellStateParts; ++k) {
        if (!L.part[k].presolve) continue;
        if (i < L.part[k].len) { if (restore) L.part[k].p[i] = snap[off + i]; else snap[off + i] = L.part[k].p[i]; }
        off += L.part[k].len;
    }
    if (i < nw) { if (restore) A.current[i] = isnap[i]; else isnap[i] = A.current[i]; }
}

// The whole pre-solve loop in ONE launch when the wells fit one resident grid (one workgroup per well, nw <= kFusedWells): per
// iteration every workgroup assembles its well, publishes its four residuals, all meet at a counter barrier, every workgroup takes
// the SAME convergence decision from all wells' residuals and updates its own well.  The residual buffer alternates with the iteration
// parity, so one barrier per iteration suffices.  Replaces 32 dependent launches (~150 us) by one (~5 us + ~4 us per iteration).
// Spins are bounded: a workgroup that gives up raises error bit 16 and every workgroup leaves at its next poll.
constexpr int kFusedWells = 256;
__device__ __forceinline__ bool presolve_barrier(int32_t* counter, int target, int32_t* flags)
{
    __syncthreads();
    __shared__ int ok;
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        int good = 1;
        for (long spins = 0; __hip_atomic_load(counter, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < target; ++spins) {
            __builtin_amdgcn_s_sleep(4);
            if (spins > (1L << 22) || (__hip_atomic_load(&flags[WF_ERR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 16)) {
                __hip_atomic_fetch_or(&flags[WF_ERR], 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); good = 0; break;
            }
        }
        ok = good;
    }
    __syncthreads();
    return ok != 0;
}
__global__ __launch_bounds__(kBlock) void k_well_presolve_fused(int nw, WellArgs A, const int32_t* __restrict__ slice_ptr, const int16_t* __restrict__ nlower,
                                                                PresolveParams S, int32_t* __restrict__ flags, int32_t* __restrict__ counter,
                                                                double* __restrict__ Ebuf /* [2][nw][4] */)
{
    const int w = blockIdx.x, tid = threadIdx.x;
    const bool writer = w == 0 && tid == 0;         // every workgroup reaches the same end; one thread of the grid writes it down
    for (int it = 0;;) {
        double* Eall = Ebuf + size_t(it & 1) * nw * 4;
        double* Eme = Eall + 4 * size_t(w);
        well_assemble_dev<double, true>(A, w, slice_ptr, nlower, 1.0, 1.0, 1.0, nullptr, (double*)nullptr, nullptr, flags, Eme, true);
        if (!presolve_barrier(counter, nw * (it + 1), flags)) return;
        const int verdict = presolve_verdict(nw, Eall, S, LoadAgent());
        if (verdict != 0) { if (writer) presolve_finish(flags, verdict, it); return; }
        ++it;
        if (tid == 0) { presolve_newton_step(A, w, Eme, S.dbhp_max_rel, flags); __threadfence(); }
        __syncthreads();
        if (it >= S.max_it) { if (writer) presolve_finish(flags, 0, it); return; }
    }
}

__global__ void k_well_flag_or(int32_t* f, int bits) { atomicOr(f, bits); }
// Fallback of the fused pre-solve: its counter barrier needs all nw workgroups resident together, which the launch guarantees only against
// the kernel's own occupancy (fused_presolve_capacity) -- other streams' and other processes' kernels give their slots back, but slowly enough
// under co-tenancy (several ranks rehearsing on one GPU) for a workgroup's bounded spin to give up (error bit 16).  That is a SCHEDULING
// condition, not a numerical one: this kernel, launched right behind the fused one, does nothing unless bit 16 is up; then it clears the
// bit, restores the well state the pre-solve started from and runs the whole loop inside ONE workgroup, wells one after the other.  Slow,
// correct, and never a NumericalIssue.
__global__ __launch_bounds__(kBlock) void k_well_presolve_serial(int nw, int np, WellArgs A, const int32_t* __restrict__ slice_ptr, const int16_t* __restrict__ nlower,
                                                                 PresolveParams S, int32_t* __restrict__ flags, double* __restrict__ snap,
                                                                 int32_t* __restrict__ isnap, double* __restrict__ Ebuf /* [nw][4] */)
{
    const int tid = threadIdx.x;
    __shared__ int go;
    if (tid == 0) go = (flags[WF_ERR] & WE_BARRIER) ? 1 : 0;
    __syncthreads();
    if (!go) return;
    for (int i = tid; i < max(4 * nw, 3 * np); i += kBlock) presolve_snapshot(A, nw, np, snap, isnap, true, i);
    // the whole error word as snapshot before the fused attempt (isnap[nw]): a half-run attempt may have left control-switch / assembly bits
    // behind that are not the pre-solve's verdict
    if (tid == 0) { flags[WF_ERR] = isnap[nw] & ~WE_BARRIER; flags[WF_DONE] = 0; flags[WF_CONV] = 0; flags[WF_ITS] = 0; }
    __threadfence();
    __syncthreads();
    for (int it = 0;;) {
        for (int w = 0; w < nw; ++w) {
            well_assemble_dev<double, true>(A, w, slice_ptr, nlower, 1.0, 1.0, 1.0, nullptr, (double*)nullptr, nullptr, flags, Ebuf + 4 * size_t(w), false);
            __threadfence();
            __syncthreads();
        }
        const int verdict = presolve_verdict(nw, Ebuf, S, LoadPlain());
        if (verdict != 0) { if (tid == 0) presolve_finish(flags, verdict, it); return; }
        ++it;
        for (int w = tid; w < nw; w += kBlock) presolve_newton_step(A, w, Ebuf + 4 * size_t(w), S.dbhp_max_rel, flags);
        __threadfence();
        __syncthreads();
        for (int g = 0; g < A.ngroups; ++g) group_targets_dev(A, g);          // updateWellTargets (:1090-1093); ends with a barrier
        if (it >= S.max_it) { if (tid == 0) presolve_finish(flags, 0, it); return; }
    }
}
// how many workgroups of the fused pre-solve the device holds at once (occupancy query x compute units, halved as a margin for the side
// streams that run next to it): the fused path is taken only for nw up to this
static int fused_presolve_capacity()
{
    static int cap = -1;
    if (cap >= 0) return cap;
    int dev = 0, ncu = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(k_well_presolve_fused), kBlock, 0) != hipSuccess) return cap = 0;
    return cap = std::max(0, (ncu * per_cu) / 2);
}

// one step of the pre-solve loop behind k_well_assemble<double, true>, ONE workgroup for all wells; the iteration count lives in
// flags[WF_ITS] between the launches, and every launch is a no-op once flags[WF_DONE] is up
__global__ __launch_bounds__(kBlock) void k_well_presolve_step(int nw, WellArgs A, PresolveParams S, int32_t* __restrict__ flags)
{
    if (flags[WF_DONE]) return;
    const int tid = threadIdx.x;
    const int verdict = presolve_verdict(nw, A.wellE, S, LoadPlain());
    if (verdict != 0) { if (tid == 0) presolve_finish(flags, verdict, flags[WF_ITS]); return; }
    for (int w = tid; w < nw; w += kBlock) presolve_newton_step(A, w, A.wellE + 4 * size_t(w), S.dbhp_max_rel, flags);
    if (A.ngroups > 0) {          // updateWellTargets behind updateWellControls (BlackoilModelBase_impl.hpp:1090-1093)
        __syncthreads();
        for (int g = 0; g < A.ngroups; ++g) group_targets_dev(A, g);
    }
    if (tid == 0) { const int it = flags[WF_ITS] + 1; if (it >= S.max_it) presolve_finish(flags, 0, it); else flags[WF_ITS] = it; }
}

// snapshot of the well state before the pre-solve / restore after one that did not converge
__global__ __launch_bounds__(kBlock) void k_well_snapshot(int nw, int np, WellArgs A, double* __restrict__ snap, int32_t* __restrict__ isnap, int restore,
                                                          const int32_t* __restrict__ flags)
{
    if (restore && flags[WF_CONV]) return;          // a converged pre-solve keeps its solution
    const int i = blockIdx.x * kBlock + threadIdx.x;
    presolve_snapshot(A, nw, np, snap, isnap, restore != 0, i);
    // the error word as it stood before the pre-solve: the serial fallback puts it back WHOLE
    if (!restore && i == 0) isnap[nw] = flags[WF_ERR];
}

// recoverVariable (NewtonIterationUtilities.cpp:134-184): dy = D^-1 (E - sum_j C_j dx_j) -- the well part of the Newton increment,
// kept resident so that stabilizeNonlinearUpdate relaxes the WHOLE increment like the reference does (NonlinearSolver_impl.hpp:260-301)
__global__ __launch_bounds__(kBlock) void k_well_recover(WellArgs A, const double* __restrict__ dx)
{
    __shared__ double sm[16];
    const int w = blockIdx.x, tid = threadIdx.x;
    double acc[4] = { 0, 0, 0, 0 };
    for (int j = A.connpos[w] + tid; j < A.connpos[w + 1]; j += kBlock) {
        const int row = A.perf_row[j];
        const double x0 = dx[row], x1 = dx[A.nbp + row], x2 = dx[2 * long(A.nbp) + row];
        const double* C = A.Q + 21 * long(j) + 9;
        for (int k = 0; k < 4; ++k) acc[k] += C[3 * k] * x0 + C[3 * k + 1] * x1 + C[3 * k + 2] * x2;
    }
    block_sum<4>(acc, sm);
    if (tid == 0) {
        const double* E = A.wellE + 4 * w;
        const double r[4] = { E[0] - acc[0], E[1] - acc[1], E[2] - acc[2], E[3] - acc[3] };
        well_dinv_mul(A, w, r, A.wdy + 4 * w);
    }
}
// stabilizeNonlinearUpdate on the well part: dy_old <- dy; dy <- omega dy (+ (1 - omega) previous dy_old for SOR)
__global__ void k_well_stabilize(int n, int sor, double omega, double* __restrict__ dy, double* __restrict__ dy_old)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d = dy[i], o = dy_old[i];
    dy_old[i] = d;
    if (omega == 1.0) return;
    dy[i] = sor ? omega * d + (1.0 - omega) * o : omega * d;
}
// updateWellState (:611-700) from the resident increment
__global__ void k_well_update(int nw, WellArgs A, double relax, double dbhp_max_rel)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    double dy[4];
    for (int k = 0; k < 4; ++k) dy[k] = relax * A.wdy[4 * w + k];
    well_apply_increment(A, w, dy, dbhp_max_rel);
}

} // namespace

// ------------------------------------------------------------------------------------------ host side
struct BlackoilDevice::VfpDev {
    int ntab = 0;
    std::vector<int32_t> h_meta;        // [ntab][VM_COUNT]
    std::vector<int32_t> h_ids;
    DevArray<int32_t> meta;
    DevArray<double> datum, blob;
};

struct BlackoilDevice::WellsDev {
    int nw = 0, nctrl = 0;
    bool vfp_active = false;            // isVFPActive (BlackoilModelBase_impl.hpp:982-1008): some well has a THP control
    DevArray<int32_t> connpos, perf_row, perf_well, perf_of_row, type, allow_cf, ctrl_type, ctrl_ptr, ctrl_vfp, thp_ctrl, current, isnap, isaved;
    DevArray<double> WI, comp_frac, ctrl_target, ctrl_distr, ctrl_alq, depth_ref, z_perf, surf_dens_perf;
    DevArray<double> wstate, thp, cdp, perf_dens, perf_pvt, avgp, qout, perf_rates, perf_press, P, Q, Fsave, wellE, Dinv, t, wdy, wdy_old;
    DevArray<double> bsums, bscratch, snap, presolve_sync, ctrl_row;
    DevArray<double> eff;           // [nw] well efficiency factors (set_well_efficiency); no part of the well STATE: not saved, not restored
    std::vector<double> h_eff;
    // controlled groups (set_well_groups): no part of the well STATE either; indexed by well and control, never by row, so a re-plan
    // leaves them alone.  group_rate[ngroups] is written by every k_group_targets launch.
    int ngroups = 0;
    DevArray<int32_t> group_ptr, group_wells;
    DevArray<double> group_sign, group_target, group_distr, group_guide, group_rate;
    std::vector<int32_t> h_group_of;        // [nw] group of the well or -1
    std::vector<double> h_ctrl_target;      // [nctrl] the targets as the caller gave them: what a removal of the groups puts back into the slots
    // rows perforated by several wells (WellArgs): the chain, the rows' list (internal rows, ascending) and every perforated row ONCE
    DevArray<int32_t> perf_next, perf_shared, shared_rows, perf_rows_once;
    DevArray<double> bde;
    int nshared = 0, max_wells_per_cell = 0, nrows_once = 0;
    DevArray<double> saved;         // snapshot for AdaptiveTimeStepping: wstate | thp | cdp | perf_rates | perf_press | perf_dens
    DevArray<int32_t> flags;
    std::vector<int32_t> h_connpos, h_cells, h_ctrl_ptr;
    double* h_pinned = nullptr;
    bool dy_valid = false;
};

void BlackoilDevice::vfp_free() { delete vfp; vfp = nullptr; }
void BlackoilDevice::wells_free() { if (wd) { if (wd->h_pinned) (void)hipHostFree(wd->h_pinned); delete wd; wd = nullptr; } }

static WellArgs args_of(BlackoilDevice::WellsDev& W, BlackoilDevice::VfpDev* V, int nbp, const double* perf, double gravity)
{
    WellArgs A;
    A.nbp = nbp;
    A.connpos = W.connpos.p; A.perf_row = W.perf_row.p; A.type = W.type.p; A.allow_cf = W.allow_cf.p; A.ctrl_type = W.ctrl_type.p;
    A.WI = W.WI.p; A.comp_frac = W.comp_frac.p; A.ctrl_target = W.ctrl_target.p; A.ctrl_distr = W.ctrl_distr.p; A.depth_ref = W.depth_ref.p;
    A.ctrl_ptr = W.ctrl_ptr.p; A.ctrl_vfp = W.ctrl_vfp.p; A.thp_ctrl = W.thp_ctrl.p; A.ctrl_alq = W.ctrl_alq.p; A.current = W.current.p; A.thp = W.thp.p;
    A.perf_dens = W.perf_dens.p; A.perf_pvt = W.perf_pvt.p; A.wdy = W.wdy.p; A.gravity = gravity; A.ctrl_row = W.ctrl_row.p;
    A.V.ntab = V ? V->ntab : 0; A.V.meta = V ? V->meta.p : nullptr; A.V.datum = V ? V->datum.p : nullptr; A.V.blob = V ? V->blob.p : nullptr;
    A.z_perf = W.z_perf.p; A.surf_dens_perf = W.surf_dens_perf.p; A.perf = perf;
    A.wstate = W.wstate.p; A.cdp = W.cdp.p; A.perf_rates = W.perf_rates.p; A.perf_press = W.perf_press.p; A.P = W.P.p; A.Q = W.Q.p;
    A.Fsave = W.Fsave.p; A.wellE = W.wellE.p; A.Dinv = W.Dinv.p; A.eff = W.eff.p;
    A.perf_of_row = W.perf_of_row.p; A.perf_next = W.perf_next.p; A.perf_well = W.perf_well.p; A.perf_shared = W.perf_shared.p; A.bde = W.bde.p;
    A.ngroups = W.ngroups; A.group_ptr = W.group_ptr.p; A.group_wells = W.group_wells.p; A.group_sign = W.group_sign.p; A.group_target = W.group_target.p;
    A.group_distr = W.group_distr.p; A.group_guide = W.group_guide.p; A.group_rate = W.group_rate.p;
    return A;
}

int BlackoilDevice::set_vfp_tables(int n, const opmgpu_vfp_table* tabs)
{
    if (n < 0 || (n > 0 && !tabs)) return OPMGPU_EINVAL;
    delete vfp; vfp = nullptr;
    if (n == 0) return OPMGPU_OK;
    VfpDev* V = new VfpDev();
    V->ntab = n;
    std::vector<double> blob, datum;
    const double one_point[1] = { 0.0 };
    for (int t = 0; t < n; ++t) {
        const opmgpu_vfp_table& T = tabs[t];
        const int nwfr = T.is_injector ? 1 : T.nwfr, ngfr = T.is_injector ? 1 : T.ngfr, nalq = T.is_injector ? 1 : T.nalq;
        if (T.nflo < 1 || T.nthp < 1 || nwfr < 1 || ngfr < 1 || nalq < 1 || T.nthp > kVfpMaxThp || !T.flo || !T.thp || !T.data ||
            (!T.is_injector && (!T.wfr || !T.gfr || !T.alq))) { delete V; return OPMGPU_EINVAL; }
        int32_t m[VM_COUNT] = { T.id, T.is_injector ? 1 : 0, T.flo_type, T.wfr_type, T.gfr_type, T.nflo, T.nthp, nwfr, ngfr, nalq, int32_t(blob.size()), 0 };
        blob.insert(blob.end(), T.flo, T.flo + T.nflo); blob.insert(blob.end(), T.thp, T.thp + T.nthp);
        const double* aw = T.is_injector ? one_point : T.wfr; const double* ag = T.is_injector ? one_point : T.gfr; const double* aa = T.is_injector ? one_point : T.alq;
        blob.insert(blob.end(), aw, aw + nwfr); blob.insert(blob.end(), ag, ag + ngfr); blob.insert(blob.end(), aa, aa + nalq);
        m[VM_DATA] = int32_t(blob.size());
        const size_t nd = size_t(T.nthp) * nwfr * ngfr * nalq * T.nflo;
        blob.insert(blob.end(), T.data, T.data + nd);
        V->h_meta.insert(V->h_meta.end(), m, m + VM_COUNT);
        V->h_ids.push_back(T.id);
        datum.push_back(T.datum_depth);
    }
    V->meta.upload(V->h_meta, stream); V->datum.upload(datum, stream); V->blob.upload(blob, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    vfp = V;
    return OPMGPU_OK;
}

// diagnostic (opmgpu_vfp_evaluate): the evaluators the well kernels call, one thread per point, on table t of the resident tables
static __global__ void k_vfp_evaluate(VfpArgs V, int t, int n, const double* __restrict__ q, const double* __restrict__ thp, const double* __restrict__ alq,
                                      const double* __restrict__ bhp_in, double* __restrict__ bhp_out, double* __restrict__ dq_out, double* __restrict__ thp_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double qi[3] = { q[3 * i], q[3 * i + 1], q[3 * i + 2] };
    double dq[3];
    bhp_out[i] = vfp_bhp(V, t, qi, thp[i], alq[i], dq);
    for (int k = 0; k < 3; ++k) dq_out[3 * i + k] = dq[k];
    thp_out[i] = vfp_thp(V, t, qi, bhp_in[i], alq[i]);
}

int BlackoilDevice::vfp_evaluate(int t, int n, const double* q, const double* thp, const double* alq, const double* bhp_in,
                                 double* bhp_out, double* dbhp_dq, double* thp_out)
{
    if (!vfp || t < 0 || t >= vfp->ntab || n < 0) return OPMGPU_EINVAL;
    if (n == 0) return OPMGPU_OK;
    const size_t N = size_t(n);
    DevArray<double> in, out;           // own buffers: nothing a later solve reads is touched
    std::vector<double> h(6 * N);
    std::copy(q, q + 3 * N, h.begin()); std::copy(thp, thp + N, h.begin() + 3 * N);
    std::copy(alq, alq + N, h.begin() + 4 * N); std::copy(bhp_in, bhp_in + N, h.begin() + 5 * N);
    in.upload(h, stream); out.alloc(5 * N);
    VfpArgs V; V.ntab = vfp->ntab; V.meta = vfp->meta.p; V.datum = vfp->datum.p; V.blob = vfp->blob.p;
    hipLaunchKernelGGL(k_vfp_evaluate, dim3((n + 63) / 64), dim3(64), 0, stream, V, t, n, in.p, in.p + 3 * N, in.p + 4 * N, in.p + 5 * N,
                       out.p, out.p + N, out.p + 4 * N);
    OPMGPU_HIP(hipGetLastError());
    out.download(h.data(), 5 * N, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    std::copy(h.begin(), h.begin() + N, bhp_out); std::copy(h.begin() + N, h.begin() + 4 * N, dbhp_dq); std::copy(h.begin() + 4 * N, h.begin() + 5 * N, thp_out);
    return OPMGPU_OK;
}

int BlackoilDevice::set_device_wells(const opmgpu_wells* s)
{
    if (!s || s->nw < 0) return OPMGPU_EINVAL;
    if (s->nw == 0) { wells_free(); device_wells = false; ls.lowrank = LowRankOp(); ls.drop_hierarchies(); return set_wells(0, nullptr, nullptr); }
    if (!s->well_connpos || !s->well_cells || !s->WI || !s->type || !s->depth_ref || !s->comp_frac || !s->ctrl_type || !s->ctrl_target) return OPMGPU_EINVAL;
    const int nw = s->nw, np = s->well_connpos[nw];
    if (s->ctrl_ptr && s->ctrl_ptr[0] != 0) return OPMGPU_EINVAL;
    // any number of DIFFERENT wells may perforate a cell; one well naming a cell twice is refused (WellsManager never produces it: a
    // repeated COMPDAT entry replaces the earlier one)
    std::vector<int32_t> last_well(nc, -1), per_cell(nc, 0);
    int nshared_cells = 0, max_per_cell = 0;
    for (int w = 0; w < nw; ++w)
        for (int j = s->well_connpos[w]; j < s->well_connpos[w + 1]; ++j) {
            const int c = s->well_cells[j];
            if (c < 0 || c >= nc) return OPMGPU_EINVAL;
            if (last_well[c] == w) throw HipError(OPMGPU_EINVAL, "opmgpu_set_device_wells: well " + std::to_string(w) + " names cell " + std::to_string(c) + " twice (several wells may share a cell, one well may not repeat it)");
            last_well[c] = w;
            if (++per_cell[c] == 2) ++nshared_cells;
            if (per_cell[c] >= 2) max_per_cell = std::max(max_per_cell, int(per_cell[c]));
        }
    if (nshared_cells > 0) {
        // what sums a shared row's terms from one workgroup per well stays out of reach: the decomposed code and the subdomain coarse space
        if (ls.comm) throw HipError(OPMGPU_EINVAL, "opmgpu_set_device_wells: a cell is perforated by several wells; a decomposed run (a communicator is attached) does not support that");
        if (ls.coarse_mode == 2 || ls.emulate_ranks > 1) throw HipError(OPMGPU_EINVAL, "opmgpu_set_device_wells: a cell is perforated by several wells; the subdomain coarse space (OPMGPU_COARSE=2, OPMGPU_EMULATE_RANKS > 1) does not support that");
    }
    if (oil_water()) {
        // no gas phase: with the inactive phase's b_g = 1, mob_g = 0, rho_g = 0 the well kernels work as they are -- the gas well equation
        // reduces to q_g = 0 with unit derivative -- as long as nothing asks for gas (THP: the VFP tables' GFR axis, out of scope)
        const int nct_ = s->ctrl_ptr ? s->ctrl_ptr[nw] : nw;
        for (int w = 0; w < nw; ++w) if (s->comp_frac[3 * w + 2] != 0.0) throw HipError(OPMGPU_EINVAL, "a deck without a gas phase: a well's comp_frac has a gas entry");
        for (int c = 0; c < nct_; ++c) {
            if (s->ctrl_type[c] == OPMGPU_CTRL_THP) throw HipError(OPMGPU_EINVAL, "a deck without a gas phase: THP controls are not supported");
            if (s->ctrl_distr && s->ctrl_distr[3 * c + 2] != 0.0) throw HipError(OPMGPU_EINVAL, "a deck without a gas phase: a well control's distribution has a gas entry (gas rate control)");
        }
    }
    wells_free();
    wd = new WellsDev();
    WellsDev& W = *wd;
    W.nw = nw; W.nshared = nshared_cells; W.max_wells_per_cell = max_per_cell;
    W.h_connpos.assign(s->well_connpos, s->well_connpos + nw + 1);
    W.h_cells.assign(s->well_cells, s->well_cells + np);
    device_wells = true;
    // pattern: plain stencil (no cliques); the perforated cells are still registered for k_perf_props
    h_well_connpos = W.h_connpos; h_well_cells = W.h_cells;
    rebuild_structure();
    auto upi = [&](DevArray<int32_t>& d, const int32_t* src, size_t n, int32_t dflt) {
        std::vector<int32_t> h(n, dflt); if (src) h.assign(src, src + n); d.upload(h, stream);
    };
    auto upd = [&](DevArray<double>& d, const double* src, size_t n) {
        std::vector<double> h(n, 0.0); if (src) h.assign(src, src + n); d.upload(h, stream);
    };
    // WellControls: several controls per well, or (ctrl_ptr == NULL) exactly one
    W.h_ctrl_ptr.resize(nw + 1);
    for (int w = 0; w <= nw; ++w) W.h_ctrl_ptr[w] = s->ctrl_ptr ? s->ctrl_ptr[w] : w;
    const int nct = W.nctrl = W.h_ctrl_ptr[nw];
    std::vector<int32_t> vfp_idx(nct, -1), thp_ctrl(nw, -1);
    W.vfp_active = false;
    for (int w = 0; w < nw; ++w) {
        if (W.h_ctrl_ptr[w + 1] <= W.h_ctrl_ptr[w]) { wells_free(); device_wells = false; return OPMGPU_EINVAL; }        // "There should be at least one control"
        for (int c = W.h_ctrl_ptr[w]; c < W.h_ctrl_ptr[w + 1]; ++c) {
            if (s->ctrl_type[c] < 0 || s->ctrl_type[c] > OPMGPU_CTRL_RESERVOIR_RATE) { wells_free(); device_wells = false; return OPMGPU_EINVAL; }
            if (s->ctrl_type[c] != OPMGPU_CTRL_THP) continue;
            const int id = s->ctrl_vfp ? s->ctrl_vfp[c] : -1;
            int found = -1;
            if (vfp) for (int t = 0; t < vfp->ntab; ++t) if (vfp->h_ids[t] == id && (vfp->h_meta[VM_COUNT * t + VM_INJ] != 0) == (s->type[w] == 0)) found = t;
            if (found < 0) { wells_free(); device_wells = false; return OPMGPU_EINVAL; }      // the reference throws std::invalid_argument for a missing table
            vfp_idx[c] = found;
            if (thp_ctrl[w] < 0) thp_ctrl[w] = c;
            W.vfp_active = true;
        }
    }
    upi(W.connpos, s->well_connpos, nw + 1, 0); upi(W.type, s->type, nw, 1); upi(W.allow_cf, s->allow_cf, nw, 1); upi(W.ctrl_type, s->ctrl_type, nct, 0);
    W.ctrl_ptr.upload(W.h_ctrl_ptr, stream); W.ctrl_vfp.upload(vfp_idx, stream); W.thp_ctrl.upload(thp_ctrl, stream);
    upd(W.WI, s->WI, np); upd(W.comp_frac, s->comp_frac, 3 * size_t(nw)); upd(W.ctrl_target, s->ctrl_target, nct);
    upd(W.ctrl_distr, s->ctrl_distr, 3 * size_t(nct)); upd(W.ctrl_alq, s->ctrl_alq, nct); upd(W.depth_ref, s->depth_ref, nw);
    W.current.alloc(nw); W.current.zero(stream); W.isnap.alloc(nw + 1); W.isaved.alloc(nw);
    W.thp.alloc(nw); W.thp.zero(stream);
    W.perf_dens.alloc(np); W.perf_dens.zero(stream); W.perf_pvt.alloc(5 * size_t(np)); W.avgp.alloc(np); W.qout.alloc(3 * size_t(np));
    W.ctrl_row.alloc(4 * size_t(nw)); W.ctrl_row.zero(stream);
    W.h_eff.assign(nw, 1.0); W.eff.upload(W.h_eff, stream);          // a new well list: every factor is 1 again
    W.h_group_of.assign(nw, -1); W.h_ctrl_target.assign(s->ctrl_target, s->ctrl_target + nct);      // ... and no controlled groups
    W.wdy.alloc(4 * size_t(nw)); W.wdy.zero(stream); W.wdy_old.alloc(4 * size_t(nw)); W.wdy_old.zero(stream);
    W.bsums.alloc(16); W.bscratch.alloc(13 * size_t(kMaxRedBlocks)); W.snap.alloc(5 * size_t(nw) + 4 * size_t(np));
    std::vector<double> zp(np), sd(3 * size_t(np));
    std::vector<int32_t> pw(np);
    for (int w = 0; w < nw; ++w) for (int j = s->well_connpos[w]; j < s->well_connpos[w + 1]; ++j) pw[j] = w;
    for (int j = 0; j < np; ++j) {
        const int c = s->well_cells[j];
        zp[j] = h_z[c];
        for (int a = 0; a < 3; ++a) sd[3 * size_t(j) + a] = h_surface_density[3 * size_t(h_pvtnum[c]) + a];
    }
    W.z_perf.upload(zp, stream); W.surf_dens_perf.upload(sd, stream); W.perf_well.upload(pw, stream);
    W.wstate.alloc(4 * size_t(nw)); W.wstate.zero(stream);
    W.cdp.alloc(np); W.cdp.zero(stream); W.perf_rates.alloc(3 * size_t(np)); W.perf_rates.zero(stream); W.perf_press.alloc(np); W.perf_press.zero(stream);
    W.P.alloc(21 * size_t(np)); W.Q.alloc(21 * size_t(np)); W.Fsave.alloc(21 * size_t(np)); W.wellE.alloc(4 * size_t(nw)); W.Dinv.alloc(16 * size_t(nw));
    W.P.zero(stream); W.Q.zero(stream); W.wellE.zero(stream); W.Dinv.zero(stream);
    W.bde.alloc(3 * size_t(np)); W.bde.zero(stream);
    W.t.alloc(7 * size_t(nw)); W.t.zero(stream);
    W.flags.alloc(WF_COUNT); W.flags.zero(stream);
    OPMGPU_HIP(hipHostMalloc(reinterpret_cast<void**>(&W.h_pinned), (4 * size_t(nw) + 8) * sizeof(double)));
    wells_rebind();
    OPMGPU_HIP(hipStreamSynchronize(stream));
    return OPMGPU_OK;
}

// (re)derive the row-indexed maps after a (re)plan and hand the operator to the solver
void BlackoilDevice::wells_rebind()
{
    if (!wd) return;
    WellsDev& W = *wd;
    const Plan& P = ls.plan;
    const int np = int(W.h_cells.size());
    // por[row] = the FIRST perforation of the row, pnext[j] = the next one of the same row: chains in ascending perforation index
    std::vector<int32_t> pr(np), por(P.nbp, -1), pnext(std::max(np, 1), -1), shared, once;
    for (int j = np - 1; j >= 0; --j) { pr[j] = P.pos[W.h_cells[j]]; pnext[j] = por[pr[j]]; por[pr[j]] = j; }
    for (int j = 0; j < np; ++j) if (por[pr[j]] == j) { once.push_back(pr[j]); if (pnext[j] >= 0) shared.push_back(pr[j]); }
    std::vector<int32_t> pshared(std::max(np, 1), 0);
    for (int j = 0; j < np; ++j) pshared[j] = (pnext[j] >= 0 || por[pr[j]] != j) ? 1 : 0;
    W.perf_shared.upload(pshared, stream);
    std::sort(shared.begin(), shared.end());
    W.nshared = int(shared.size()); W.nrows_once = int(once.size());
    if (shared.empty()) shared.push_back(0);
    W.perf_row.upload(pr, stream); W.perf_of_row.upload(por, stream); W.perf_next.upload(pnext, stream);
    W.shared_rows.upload(shared, stream); W.perf_rows_once.upload(once, stream);
    // the opt-in Woodbury correction of stage 2 updates a perforated row from one workgroup per well: off while wells share a cell
    if (W.nshared > 0 && ls.well_woodbury) {
        static bool said = false;
        if (!said) { said = true; std::fprintf(stderr, "[opmgpu] OPMGPU_WELL_WOODBURY=1 is switched off for this well list: a cell is perforated by several wells\n"); }
        ls.well_woodbury = false; ls.wb_suspended = true;
    } else if (W.nshared == 0 && ls.wb_suspended) { ls.well_woodbury = true; ls.wb_suspended = false; }
    d_rhs_extra.alloc(3 * size_t(P.nbp));
    LowRankOp& L = ls.lowrank;
    L.nw = W.nw; L.nperf = np; L.connpos = W.connpos.p; L.perf_row = W.perf_row.p; L.perf_well = W.perf_well.p; L.perf_of_row = W.perf_of_row.p; L.perf_next = W.perf_next.p;
    L.P = W.P.p; L.Q = W.Q.p; L.t = W.t.p;
    L.Fsave = W.Fsave.p; L.ctrl_row = W.ctrl_row.p; L.eff = W.eff.p;
    for (int a = 0; a < 3; ++a) L.scale[a] = prm.matbalscale[a];
    ls.drop_hierarchies();
}

// WEFAC: one factor per well in the order of set_device_wells, NULL = all ones.  The array keeps its address, so the kernel arguments and
// the solver's LowRankOp stay valid; the next assembly reads the new values.
int BlackoilDevice::set_well_efficiency(const double* factors)
{
    if (!wd) throw HipError(OPMGPU_EINVAL, "opmgpu_set_well_efficiency: no device wells are set (opmgpu_set_device_wells comes first)");
    WellsDev& W = *wd;
    if (factors)
        for (int w = 0; w < W.nw; ++w) {
            if (!std::isfinite(factors[w])) throw HipError(OPMGPU_EINVAL, "opmgpu_set_well_efficiency: the factor of well " + std::to_string(w) + " is not finite");
            if (!(factors[w] > 0.0 && factors[w] <= 1.0)) throw HipError(OPMGPU_EINVAL, "opmgpu_set_well_efficiency: the factor of well " + std::to_string(w) + " is outside (0, 1]");
        }
    if (factors) W.h_eff.assign(factors, factors + W.nw); else W.h_eff.assign(W.nw, 1.0);
    OPMGPU_HIP(hipMemcpyAsync(W.eff.p, W.h_eff.data(), size_t(W.nw) * sizeof(double), hipMemcpyHostToDevice, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
    return OPMGPU_OK;
}
// Controlled groups (the rule: include/opmgpu.h).  Everything is checked against the host copies of the well list before anything is
// uploaded, so a refused call leaves the groups in force as they were.  ngroups == 0 removes them.
int BlackoilDevice::set_well_groups(int ngroups, const int32_t* group_ptr, const int32_t* group_wells, const double* sign, const double* target,
                                    const double* distr, const double* guide)
{
    const std::string who = "opmgpu_set_well_groups: ";
    if (!wd) throw HipError(OPMGPU_EINVAL, who + "no device wells are set (opmgpu_set_device_wells comes first)");
    if (ls.comm) throw HipError(OPMGPU_EINVAL, who + "a communicator is attached; group control in a decomposed run is not supported (a group's wells may sit on several ranks)");
    WellsDev& W = *wd;
    if (ngroups < 0) throw HipError(OPMGPU_EINVAL, who + "ngroups is negative");
    if (ngroups == 0) {
        if (W.ngroups > 0) { W.ctrl_target.upload(W.h_ctrl_target, stream); OPMGPU_HIP(hipStreamSynchronize(stream)); }      // the slots' targets as they were given
        W.ngroups = 0; W.h_group_of.assign(W.nw, -1);
        return OPMGPU_OK;
    }
    if (!group_ptr || !group_wells || !sign || !target || !distr || !guide) throw HipError(OPMGPU_EINVAL, who + "an array is NULL");
    if (group_ptr[0] != 0) throw HipError(OPMGPU_EINVAL, who + "group_ptr does not start at 0");
    // the controls as they were given: the slot's type and distr are checked against them
    std::vector<int32_t> h_type(W.nctrl);
    std::vector<double> h_distr(3 * size_t(W.nctrl));
    W.ctrl_type.download(h_type.data(), h_type.size(), stream); W.ctrl_distr.download(h_distr.data(), h_distr.size(), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    std::vector<int32_t> group_of(W.nw, -1);
    for (int g = 0; g < ngroups; ++g) {
        const std::string gs = "group " + std::to_string(g);
        if (group_ptr[g + 1] < group_ptr[g]) throw HipError(OPMGPU_EINVAL, who + "group_ptr decreases at " + gs);
        if (sign[g] != 1.0 && sign[g] != -1.0) throw HipError(OPMGPU_EINVAL, who + "the sign of " + gs + " is neither -1 (production) nor +1 (injection)");
        if (!std::isfinite(target[g])) throw HipError(OPMGPU_EINVAL, who + "the target of " + gs + " is not finite");
        if (target[g] < 0.0) throw HipError(OPMGPU_EINVAL, who + "the target of " + gs + " is negative");
        for (int a = 0; a < 3; ++a) if (!std::isfinite(distr[3 * g + a])) throw HipError(OPMGPU_EINVAL, who + "a phase weight of " + gs + " is not finite");
        for (int i = group_ptr[g]; i < group_ptr[g + 1]; ++i) {
            const int w = group_wells[i];
            if (w < 0 || w >= W.nw) throw HipError(OPMGPU_EINVAL, who + gs + " names well " + std::to_string(w) + ", which does not exist");
            const std::string wsn = "well " + std::to_string(w);
            if (group_of[w] >= 0) throw HipError(OPMGPU_EINVAL, who + wsn + " is in two groups (" + std::to_string(group_of[w]) + " and " + std::to_string(g) + ")");
            group_of[w] = g;
            if (!std::isfinite(guide[i])) throw HipError(OPMGPU_EINVAL, who + "the guide rate of " + wsn + " is not finite");
            if (!(guide[i] > 0.0)) throw HipError(OPMGPU_EINVAL, who + "the guide rate of " + wsn + " is not positive");
            const int c = W.h_ctrl_ptr[w + 1] - 1;
            bool same = h_type[c] == OPMGPU_CTRL_SURFACE_RATE;
            for (int a = 0; a < 3; ++a) same = same && h_distr[3 * size_t(c) + a] == distr[3 * g + a];
            if (!same) throw HipError(OPMGPU_EINVAL, who + "the last control of " + wsn + " is not a SURFACE_RATE slot with the distr of " + gs);
        }
    }
    const size_t nm = size_t(group_ptr[ngroups]);
    if (W.ngroups > 0) W.ctrl_target.upload(W.h_ctrl_target, stream);      // wells that were members and are no longer: their slots' targets as they were given
    W.group_ptr.upload(group_ptr, size_t(ngroups) + 1, stream); W.group_wells.upload(group_wells, nm, stream);
    W.group_sign.upload(sign, size_t(ngroups), stream); W.group_target.upload(target, size_t(ngroups), stream);
    W.group_distr.upload(distr, 3 * size_t(ngroups), stream); W.group_guide.upload(guide, nm, stream);
    W.group_rate.ensure(size_t(ngroups)); W.group_rate.zero(stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));          // the caller's arrays may go
    W.ngroups = ngroups; W.h_group_of = group_of;
    return OPMGPU_OK;
}
// the slot targets the rule gives for the well state and current controls as they stand (the kernel runs here too, so the call needs no
// assembly before it): slot_target[nw], NaN for a well in no group; group_rate[ngroups]
int BlackoilDevice::get_well_group_targets(double* slot_target, double* group_rate)
{
    if (!wd) throw HipError(OPMGPU_EINVAL, "opmgpu_get_well_group_targets: no device wells are set");
    WellsDev& W = *wd;
    std::vector<double> tg(W.nctrl);
    if (W.ngroups > 0) {
        hipLaunchKernelGGL(k_group_targets, dim3(W.ngroups), dim3(kBlock), 0, stream, args_of(W, vfp, ls.plan.nbp, d_perf.p, gravity));
        OPMGPU_HIP(hipGetLastError());
        W.ctrl_target.download(tg.data(), tg.size(), stream);
        if (group_rate) W.group_rate.download(group_rate, size_t(W.ngroups), stream);
        OPMGPU_HIP(hipStreamSynchronize(stream));
    }
    if (slot_target)
        for (int w = 0; w < W.nw; ++w) slot_target[w] = (W.ngroups > 0 && W.h_group_of[w] >= 0) ? tg[W.h_ctrl_ptr[w + 1] - 1] : std::nan("");
    return OPMGPU_OK;
}
int BlackoilDevice::well_group_count() const { return wd ? wd->ngroups : 0; }
// rows perforated by more than one well, and the largest number of wells in one cell (both 0 without shared cells)
int BlackoilDevice::well_shared_cells(int32_t* shared_rows, int32_t* max_wells_per_cell) const
{
    if (!wd) throw HipError(OPMGPU_EINVAL, "opmgpu_well_shared_cells: no device wells are set");
    if (shared_rows) *shared_rows = wd->nshared;
    if (max_wells_per_cell) *max_wells_per_cell = wd->max_wells_per_cell;
    return OPMGPU_OK;
}
int BlackoilDevice::shared_well_rows() const { return wd ? wd->nshared : 0; }
int BlackoilDevice::get_well_efficiency(double* factors) const
{
    if (!wd) throw HipError(OPMGPU_EINVAL, "opmgpu_get_well_efficiency: no device wells are set");
    std::copy(wd->h_eff.begin(), wd->h_eff.end(), factors);
    return OPMGPU_OK;
}

int BlackoilDevice::well_state_set(const double* bhp, const double* qs, const double* perf_press, const double* perf_rates)
{
    if (!wd || !bhp || !qs) return OPMGPU_EINVAL;
    WellsDev& W = *wd;
    std::vector<double> h(4 * size_t(W.nw));
    for (int w = 0; w < W.nw; ++w) { for (int a = 0; a < 3; ++a) h[4 * w + a] = qs[3 * w + a]; h[4 * w + 3] = bhp[w]; }
    W.wstate.upload(h, stream);
    if (perf_rates) W.perf_rates.upload(perf_rates, 3 * W.h_cells.size(), stream);
    if (perf_press) W.perf_press.upload(perf_press, W.h_cells.size(), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    return OPMGPU_OK;
}

int BlackoilDevice::well_state_get(double* bhp, double* qs, double* perf_press, double* perf_rates)
{
    if (!wd) return OPMGPU_EINVAL;
    WellsDev& W = *wd;
    std::vector<double> h(4 * size_t(W.nw));
    W.wstate.download(h.data(), h.size(), stream);
    if (perf_press) W.perf_press.download(perf_press, W.h_cells.size(), stream);
    if (perf_rates) W.perf_rates.download(perf_rates, 3 * W.h_cells.size(), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    for (int w = 0; w < W.nw; ++w) { if (qs) for (int a = 0; a < 3; ++a) qs[3 * w + a] = h[4 * w + a]; if (bhp) bhp[w] = h[4 * w + 3]; }
    return OPMGPU_OK;
}

// computeWellConnectionPressures (StandardWells_impl.hpp:336-358) from the resident reservoir + well state; gate: run only if *gate != 0
void BlackoilDevice::wells_connection_pressures(const int32_t* gate)
{
    WellsDev& W = *wd;
    WellArgs A = args_of(W, vfp, ls.plan.nbp, d_perf.p, gravity);
    const int g = (W.nw + 63) / 64;
    hipLaunchKernelGGL(k_well_avg_press, dim3(g), dim3(64), 0, stream, W.nw, A, gate, W.avgp.p);
    perf_pvt_device(W.avgp.p, W.perf_pvt.p, gate);
    hipLaunchKernelGGL(k_well_cdp, dim3(W.nw), dim3(64), 0, stream, W.nw, A, gravity, gate, W.qout.p);
}

// called by assemble() after the reservoir kernels; the well part of BlackoilModelBase::assemble in the reference's order (:757-840)
void BlackoilDevice::wells_prologue()
{
    WellsDev& W = *wd;
    perf_props_device();
    WellArgs A = args_of(W, vfp, ls.plan.nbp, d_perf.p, gravity);
    if (W.vfp_active) wells_connection_pressures(nullptr);        // VFP: densities for the hydrostatic correction, every assembly (:771-776)
    // group targets before the control update (applyGroupControls of setupGroupControl, :779-783: the rule is stateless, so every assembly
    // may do what the reference does at the first) and after it (updateWellTargets, :791)
    if (W.ngroups > 0) hipLaunchKernelGGL(k_group_targets, dim3(W.ngroups), dim3(kBlock), 0, stream, A);
    hipLaunchKernelGGL(k_well_controls, dim3((W.nw + 63) / 64), dim3(64), 0, stream, W.nw, A, W.flags.p);        // updateWellControls (:785)
    if (W.ngroups > 0) hipLaunchKernelGGL(k_group_targets, dim3(W.ngroups), dim3(kBlock), 0, stream, A);
}
// Newton iterations after the first of a time step: the prologue needs the state only, the reservoir assembly (0.36 ms) does not touch what
// it writes (d_perf, the wells' control state) -- so it runs beside it on its own stream instead of 35 us behind it.  Not on the first
// iteration (the pre-solve that follows needs the assembly's 1/b sums anyway) and not with THP controls (connection pressures in between).
bool BlackoilDevice::wells_prologue_async(bool initial)
{
    static const bool on = env_flag("OPMGPU_WELL_PROLOGUE_ASYNC", true);
    well_prologue_done = false;
    if (!on || !wd || initial || wd->vfp_active) return false;
    if (!well_stream) {
        OPMGPU_HIP(hipStreamCreateWithFlags(&well_stream, hipStreamNonBlocking));
        for (auto& e : ev_well) OPMGPU_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    OPMGPU_HIP(hipEventRecord(ev_well[0], stream));               // the state the previous update left
    OPMGPU_HIP(hipStreamWaitEvent(well_stream, ev_well[0], 0));
    {
        StreamSwapGuard g(stream, well_stream, ls.kt.on);          // (event brackets belong to the main stream); restored also if the prologue throws
        wells_prologue();
    }
    OPMGPU_HIP(hipEventRecord(ev_well[1], well_stream));
    well_prologue_done = true;
    return true;
}

void BlackoilDevice::wells_assemble(bool initial)
{
    if (!wd) {
        // multi-GPU run with wells on OTHER ranks: the pre-solve's B_avg is a global mean -- take part in its all-reduce
        if (initial && prm.solve_welleq_initially && ls.comm && ls.run_has_wells) binv_sums_device(d_red.p, d_red.p + kRedPart);
        return;
    }
    WellsDev& W = *wd;
    const Plan& P = ls.plan;
    if (!well_prologue_done) wells_prologue();
    well_prologue_done = false;
    WellArgs A = args_of(W, vfp, P.nbp, d_perf.p, gravity);
    const double* sc = prm.matbalscale;
    if (initial) {
        wells_connection_pressures(nullptr);      // once per time step from the explicit state (:797-805)
        W.wdy_old.zero(stream);
        if (prm.solve_welleq_initially) {
            // solveWellEq (:1018-1133): <= 15 Newton iterations on the well equations with the reservoir frozen.  Every launch is a
            // no-op once the device-side `done` flag is up, so the loop needs no host synchronisation.
            const int np = int(W.h_cells.size());
            const int gs = grid_for(std::max(4 * W.nw, 3 * np));
            hipLaunchKernelGGL(k_well_snapshot, dim3(gs), dim3(kBlock), 0, stream, W.nw, np, A, W.snap.p, W.isnap.p, 0, (const int32_t*)W.flags.p);
            OPMGPU_HIP(hipMemsetAsync(W.flags.p + WF_DONE, 0, 3 * sizeof(int32_t), stream));
            binv_sums_device(W.bsums.p, W.bscratch.p);
            const double ncg = ls.comm ? double(ls.comm->n_owned_global) : double(nc);
            const PresolveParams S = { W.bsums.p, ncg, prm.tolerance_wells, prm.tolerance_well_control, prm.max_residual_allowed, prm.dbhp_max_rel, 15 };
            // OPMGPU_WELL_PRESOLVE_FUSED: 1 (default) one launch with a counter barrier; 0 two launches per iteration; 2 (tests) the serial
            // fallback that takes over when the fused kernel's barrier gives up.  Read per call: once per time step.
            const char* fenv = std::getenv("OPMGPU_WELL_PRESOLVE_FUSED");
            const int fmode = fenv ? std::atoi(fenv) : 1;
            // With controlled groups every iteration's group targets need ALL wells' new rates and controls: the fused kernel has no
            // grid-wide meeting point behind its Newton step, so groups take the unfused pair below, whose one-workgroup step kernel
            // re-shares the targets behind its control update (the serial fallback, fmode 2, does the same and stays reachable).
            const bool fused_ok = W.ngroups == 0 || fmode == 2;
            if (fmode != 0 && fused_ok && W.nw <= std::min(kFusedWells, fused_presolve_capacity())) {
                // one launch: one workgroup per well, counter barrier per iteration -- all nw workgroups fit the device together
                // (fused_presolve_capacity: the kernel's occupancy x compute units, with a margin)
                W.presolve_sync.alloc(4 + 8 * size_t(W.nw)); W.presolve_sync.zero(stream);
                // (tests) the give-up bit AND a stray control bit of a half-run attempt: the fallback must wipe both
                if (fmode == 2) hipLaunchKernelGGL(k_well_flag_or, dim3(1), dim3(1), 0, stream, W.flags.p + WF_ERR, WE_BARRIER | WE_NO_CONTROL);
                else
                hipLaunchKernelGGL(k_well_presolve_fused, dim3(W.nw), dim3(kBlock), 0, stream, W.nw, A, ls.dp.slice_ptr.p, ls.dp.nlower.p, S, W.flags.p,
                                   reinterpret_cast<int32_t*>(W.presolve_sync.p), W.presolve_sync.p + 4);
                // does nothing unless the barrier gave up (error bit 16): then the loop once more from the snapshot, in one workgroup
                hipLaunchKernelGGL(k_well_presolve_serial, dim3(1), dim3(kBlock), 0, stream, W.nw, np, A, ls.dp.slice_ptr.p, ls.dp.nlower.p, S, W.flags.p,
                                   W.snap.p, W.isnap.p, W.presolve_sync.p + 4);
            } else
            for (int it = 0; it <= S.max_it; ++it) {
                hipLaunchKernelGGL((k_well_assemble<double, true>), dim3(W.nw), dim3(kBlock), 0, stream, A, ls.dp.slice_ptr.p, ls.dp.nlower.p, sc[0], sc[1], sc[2],
                                   (double*)nullptr, (double*)nullptr, (double*)nullptr, W.flags.p);
                hipLaunchKernelGGL(k_well_presolve_step, dim3(1), dim3(kBlock), 0, stream, W.nw, A, S, W.flags.p);
            }
            // converged: connection pressures from the new well state (:1122); otherwise the well state is restored (:1124-1126)
            wells_connection_pressures(W.flags.p + WF_CONV);
            hipLaunchKernelGGL(k_well_snapshot, dim3(gs), dim3(kBlock), 0, stream, W.nw, np, A, W.snap.p, W.isnap.p, 1, (const int32_t*)W.flags.p);
            // a pre-solve that did not converge has put wstate and current back: the slot targets follow the state they are a function of
            // (after a converged one the launch recomputes the bits that are there)
            if (W.ngroups > 0) hipLaunchKernelGGL(k_group_targets, dim3(W.ngroups), dim3(kBlock), 0, stream, A);
        }
    }
    d_rhs_extra.zero(stream);
    if (ls.matrix_is_float)
        hipLaunchKernelGGL((k_well_assemble<float, false>), dim3(W.nw), dim3(kBlock), 0, stream, A, ls.dp.slice_ptr.p, ls.dp.nlower.p, sc[0], sc[1], sc[2], d_R.p,
                           ls.matrix_f(), d_rhs_extra.p, W.flags.p);
    else
        hipLaunchKernelGGL((k_well_assemble<double, false>), dim3(W.nw), dim3(kBlock), 0, stream, A, ls.dp.slice_ptr.p, ls.dp.nlower.p, sc[0], sc[1], sc[2], d_R.p,
                           ls.matrix_d(), d_rhs_extra.p, W.flags.p);
    if (W.nshared > 0) {          // rows of several wells: their terms in ascending perforation index, behind the wells' workgroups
        const int gsh = (W.nshared + 63) / 64;
        if (ls.matrix_is_float)
            hipLaunchKernelGGL((k_well_shared_rows<float>), dim3(gsh), dim3(64), 0, stream, W.nshared, (const int32_t*)W.shared_rows.p, A, ls.dp.slice_ptr.p, ls.dp.nlower.p,
                               sc[0], sc[1], sc[2], d_R.p, ls.matrix_f(), d_rhs_extra.p);
        else
            hipLaunchKernelGGL((k_well_shared_rows<double>), dim3(gsh), dim3(64), 0, stream, W.nshared, (const int32_t*)W.shared_rows.p, A, ls.dp.slice_ptr.p, ls.dp.nlower.p,
                               sc[0], sc[1], sc[2], d_R.p, ls.matrix_d(), d_rhs_extra.p);
    }
    // every perforated row once (a row of several wells appears once)
    if (ls.matrix_is_float) ls.cpr_reweigh_rows<float>(W.perf_rows_once.p, W.nrows_once); else ls.cpr_reweigh_rows<double>(W.perf_rows_once.p, W.nrows_once);
    has_rhs_extra = true;
    W.dy_valid = false;
}

// well part of getConvergence (BlackoilModelBase_impl.hpp:1769-1779): max |flux equation| per phase, max |control equation|
bool BlackoilDevice::has_device_wells() const { return wd != nullptr || ls.run_has_wells; }

// max |flux equation| per phase, max |control equation|, NaN / failure mark, singular mark of this rank's wells (zeros without wells); the
// error word is consumed (reset) here, like well_convergence() does on the host path
__global__ __launch_bounds__(kBlock) void k_well_conv_pack(int nw, const double* __restrict__ wellE, int32_t* __restrict__ flags, double* __restrict__ out)
{
    __shared__ double sm[4][6];
    double m[6] = { 0, 0, 0, 0, 0, 0 };
    for (int w = threadIdx.x; w < nw; w += kBlock)
        for (int k = 0; k < 4; ++k) { const double e = fabs(wellE[4 * w + k]); if (!(e == e)) m[4] = 1.0; else m[k] = fmax(m[k], e); }
    for (int k = 0; k < 6; ++k) {
        double v = m[k];
        for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < 6; ++k) out[k] = fmax(fmax(sm[0][k], sm[1][k]), fmax(sm[2][k], sm[3][k]));
        const int32_t fl = flags ? flags[0] : 0;
        if (fl & WE_NUMERICAL) out[4] = 1.0;
        if (fl & WE_SINGULAR) out[5] = 1.0;
        if (fl) flags[0] = 0;
    }
}
void BlackoilDevice::well_conv_pack(double* d_out6)
{
    if (wd) hipLaunchKernelGGL(k_well_conv_pack, dim3(1), dim3(kBlock), 0, stream, wd->nw, (const double*)wd->wellE.p, wd->flags.p + WF_ERR, d_out6);
    else OPMGPU_HIP(hipMemsetAsync(d_out6, 0, 6 * sizeof(double), stream));
}

bool BlackoilDevice::well_words_sources(const void*& e, int& ne, const void*& f) const
{
    if (!wd) return false;
    e = wd->wellE.p; ne = 8 * wd->nw; f = wd->flags.p + WF_ERR;
    return true;
}

int BlackoilDevice::well_convergence(double* flux3, double* ctrl)
{
    if (!wd && !ls.comm) return OPMGPU_EINVAL;
    double f[3] = { 0, 0, 0 }, c = 0.0;
    bool bad = false, singular = false;
    if (ls.comm && well_red_valid) {            // all-reduced with the cells' maxima by convergence() after this assembly
        well_red_valid = false;
        for (int a = 0; a < 3; ++a) f[a] = h_red[13 + a];
        c = h_red[16]; bad = h_red[17] != 0.0; singular = h_red[18] != 0.0;
        if (flux3) for (int a = 0; a < 3; ++a) flux3[a] = f[a];
        if (ctrl) *ctrl = c;
        if (singular) return OPMGPU_ESINGULAR;
        return bad ? OPMGPU_ENUMERICAL : OPMGPU_OK;
    }
    if (wd) {
        WellsDev& W = *wd;
        int32_t fl = 0;
        if (well_words_valid && int(well_words.size()) == 8 * W.nw + 1) {            // read back by convergence() after this assembly
            std::memcpy(W.h_pinned, well_words.data(), 4 * size_t(W.nw) * sizeof(double));
            std::memcpy(&fl, well_words.data() + 8 * W.nw, sizeof(int32_t));
            well_words_valid = false;
        } else if (8 * W.nw + 1 <= LinSolver::kPubWords) {
            const uint32_t* h = ls.fetch_words(W.wellE.p, 8 * W.nw, W.flags.p + WF_ERR, 1);
            std::memcpy(W.h_pinned, h, 4 * size_t(W.nw) * sizeof(double));
            std::memcpy(&fl, h + 8 * W.nw, sizeof(int32_t));
        } else {
            OPMGPU_HIP(hipMemcpyAsync(W.h_pinned, W.wellE.p, 4 * size_t(W.nw) * sizeof(double), hipMemcpyDeviceToHost, stream));
            OPMGPU_HIP(hipMemcpyAsync(&fl, W.flags.p + WF_ERR, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
            OPMGPU_HIP(hipStreamSynchronize(stream));
        }
        for (int w = 0; w < W.nw; ++w) {
            for (int a = 0; a < 3; ++a) { const double e = std::fabs(W.h_pinned[4 * w + a]); if (!(e == e)) bad = true; f[a] = std::max(f[a], e); }
            const double e = std::fabs(W.h_pinned[4 * w + 3]); if (!(e == e)) bad = true; c = std::max(c, e);
        }
        if (fl) OPMGPU_HIP(hipMemsetAsync(W.flags.p + WF_ERR, 0, sizeof(int32_t), stream));
        if (fl & WE_SINGULAR) singular = true;
        if (fl & WE_NUMERICAL) bad = true;
    }
    if (ls.comm) {      // collective: every rank calls it, also the ones without wells
        double loc[6] = { f[0], f[1], f[2], c, bad ? 1.0 : 0.0, singular ? 1.0 : 0.0 };
        OPMGPU_HIP(hipMemcpyAsync(d_red.p, loc, sizeof(loc), hipMemcpyHostToDevice, stream));
        ls.comm->allreduce_max(d_red.p, 6, stream);
        OPMGPU_HIP(hipMemcpyAsync(h_red, d_red.p, sizeof(loc), hipMemcpyDeviceToHost, stream));
        OPMGPU_HIP(hipStreamSynchronize(stream));
        for (int a = 0; a < 3; ++a) f[a] = h_red[a];
        c = h_red[3]; bad = h_red[4] != 0.0; singular = h_red[5] != 0.0;
    }
    if (flux3) for (int a = 0; a < 3; ++a) flux3[a] = f[a];
    if (ctrl) *ctrl = c;
    if (singular) return OPMGPU_ESINGULAR;
    return bad ? OPMGPU_ENUMERICAL : OPMGPU_OK;
}

void BlackoilDevice::wells_recover()
{
    if (!wd) return;
    WellsDev& W = *wd;
    WellArgs A = args_of(W, vfp, ls.plan.nbp, d_perf.p, gravity);
    hipLaunchKernelGGL(k_well_recover, dim3(W.nw), dim3(kBlock), 0, stream, A, (const double*)d_dx.p);
    W.dy_valid = true;
}

void BlackoilDevice::wells_stabilize(int sor, double omega)
{
    if (!wd) return;
    WellsDev& W = *wd;
    if (!W.dy_valid) wells_recover();
    const int n = 4 * W.nw;
    hipLaunchKernelGGL(k_well_stabilize, dim3((n + 63) / 64), dim3(64), 0, stream, n, sor, omega, W.wdy.p, W.wdy_old.p);
}

void BlackoilDevice::wells_update(double relax, bool dx_from_host)
{
    if (!wd) return;
    WellsDev& W = *wd;
    if (!W.dy_valid || dx_from_host) wells_recover();
    WellArgs A = args_of(W, vfp, ls.plan.nbp, d_perf.p, gravity);
    hipLaunchKernelGGL(k_well_update, dim3((W.nw + 63) / 64), dim3(64), 0, stream, W.nw, A, relax, prm.dbhp_max_rel);
    W.dy_valid = false;
}

// device-side last_state of AdaptiveTimeStepping: every part of the well state and `current`, saved or (restore) put back
void BlackoilDevice::wells_saved_state(bool restore)
{
    if (!wd || (restore && !wd->saved.p)) return;
    WellsDev& W = *wd;
    const int nw = W.nw, np = int(W.h_cells.size());
    if (!restore) W.saved.alloc(5 * size_t(nw) + 6 * size_t(np));
    auto copy = [&](void* state, void* saved, size_t bytes) {
        OPMGPU_HIP(hipMemcpyAsync(restore ? state : saved, restore ? saved : state, bytes, hipMemcpyDeviceToDevice, stream));
    };
    const WellStateLayout L = well_state_layout(args_of(W, vfp, ls.plan.nbp, d_perf.p, gravity), nw, np);
    size_t off = 0;
    for (const WellStatePart& part : L.part) { copy(part.p, W.saved.p + off, part.len * sizeof(double)); off += part.len; }
    copy(W.current.p, W.isaved.p, nw * sizeof(int32_t));
}

int BlackoilDevice::well_controls_set(const int32_t* current, const double* thp)
{
    if (!wd) return OPMGPU_EINVAL;
    WellsDev& W = *wd;
    if (current) {
        for (int w = 0; w < W.nw; ++w) if (current[w] < 0 || current[w] >= W.h_ctrl_ptr[w + 1] - W.h_ctrl_ptr[w]) return OPMGPU_EINVAL;
        W.current.upload(current, size_t(W.nw), stream);
    }
    if (thp) W.thp.upload(thp, size_t(W.nw), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    return OPMGPU_OK;
}
// well_controls_iset_target / well_controls_iset_distr of every control at once (what SimulatorBase::computeRESV does to the RESERVOIR_RATE
// controls once per report step, SimulatorBase_impl.hpp:551-553): target[nctrl] and / or distr[nctrl][3] in the order of opmgpu_set_device_wells
int BlackoilDevice::well_controls_set_targets(const double* target, const double* distr)
{
    if (!wd) return OPMGPU_EINVAL;
    WellsDev& W = *wd;
    if (target) { W.ctrl_target.upload(target, size_t(W.nctrl), stream); W.h_ctrl_target.assign(target, target + W.nctrl); }
    if (distr) W.ctrl_distr.upload(distr, 3 * size_t(W.nctrl), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    return OPMGPU_OK;
}
int BlackoilDevice::well_controls_get(int32_t* current, double* thp, int32_t* pre_its, int32_t* pre_conv)
{
    if (!wd) return OPMGPU_EINVAL;
    WellsDev& W = *wd;
    int32_t fl[WF_COUNT];
    if (current) W.current.download(current, size_t(W.nw), stream);
    if (thp) W.thp.download(thp, size_t(W.nw), stream);
    W.flags.download(fl, WF_COUNT, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    if (pre_its) *pre_its = fl[WF_ITS];
    if (pre_conv) *pre_conv = fl[WF_CONV];
    return OPMGPU_OK;
}

} // namespace opmgpu
