// blackoil_output.hip -- what the black-oil model runs once per run or per report step, off every Newton iteration: fluid in place, the
// output record, computeMaxDp, SWATINIT, capPress, the voidage coefficients and region sums of the rate converter, the host well model's
// copies of the perforation properties, the residual's download and the assembly timer -- kernels and their BlackoilDevice methods.
// A translation unit of its own: these kernels share no inlining with the Newton path's (blackoil.hip), only the evaluators of
// fluid_eval.hpp.  Not tuned, not timed.
#include "fluid_eval.hpp"

#include <algorithm>
#include <cmath>

namespace opmgpu {

// computeFluidInPlace, the per-cell part (BlackoilModelBase_impl.hpp:2263-2296): fip[phase] = ((pv_mult * b_phase) * s_phase) * pv with b at the
// phase pressures and the cell's phase condition, dissolved gas = rs * fip[oil], vaporised oil = rv * fip[gas]; plus what the region
// loops need of the state (pore volume, pressure, so + sg).  Output in the CALLER's cell order: out[q * nc + nat[row]], q = 0..7.
template <int KM>
__global__ __launch_bounds__(kBlock) void k_fip_cells(int nc, DevTables T, const int32_t* __restrict__ nat, const double* __restrict__ pv, CellPlanes C,
                                                      double* __restrict__ out)
{
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    CellEval q;
    eval_row<KM>(T, c, C, q);
    const long n = nat[c];
    const double so = C.so[c], sgv = C.sg[c], swv = C.sw[c];          // the state's saturations, as the reference takes them
    const double fw = ((q.pvm.v * q.b[0].v) * swv) * pv[c];
    const double fo = ((q.pvm.v * q.b[1].v) * so) * pv[c];
    const double fg = ((q.pvm.v * q.b[2].v) * sgv) * pv[c];
    out[0 * long(nc) + n] = fw; out[1 * long(nc) + n] = fo; out[2 * long(nc) + n] = fg;
    out[3 * long(nc) + n] = C.rs[c] * fo; out[4 * long(nc) + n] = C.rv[c] * fg;
    out[5 * long(nc) + n] = pv[c]; out[6 * long(nc) + n] = C.p[c]; out[7 * long(nc) + n] = so + sgv;
}

// BlackoilModelBase's SimulatorData, the per-cell output record of a report step (BlackoilModelBase_impl.hpp:662-683 and rq_[].b / rho /
// mu / kr of the assembly; named in SimulatorFullyImplicitBlackoilOutput.hpp:512-567): eval_row of the RESIDENT state, so end-point and
// vertical scaling, hysteresis, VAPPARS and ROCKTAB act as in the assembly.  kr is the relative permeability itself (no transmissibility
// multiplier, not divided by the viscosity); RsSat / RvSat are the saturated values (VAPPARS factor included) of EVERY cell whatever its
// phase state; Pb / Pd invert the plain curves at the solution state's rs / rv (sat_pressure).  OPMGPU_SIMDATA_K planes in the CALLER's
// cell order: out[q * nc + nat[row]], slots OPMGPU_SD_* of opmgpu.h.  An output path: once per report step.
template <int KM>
__global__ __launch_bounds__(kBlock) void k_simulator_data(int nc, DevTables T, const int32_t* __restrict__ nat, CellPlanes C, double* __restrict__ out)
{
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    CellEval q;
    CellOutput x;
    eval_row<KM, true>(T, c, C, q, &x);
    const int preg = C.pvtnum[c];
    double* o = out + nat[c];
    const long n = nc;
#pragma unroll
    for (int ph = 0; ph < 3; ++ph) {
        o[(OPMGPU_SD_BW + ph) * n] = q.b[ph].v; o[(OPMGPU_SD_WAT_DEN + ph) * n] = q.rho[ph].v;
        o[(OPMGPU_SD_WAT_VISC + ph) * n] = x.mu[ph]; o[(OPMGPU_SD_WATKR + ph) * n] = x.kr[ph];
    }
    o[OPMGPU_SD_RSSAT * n] = x.rsSat; o[OPMGPU_SD_RVSAT * n] = x.rvSat;
    o[OPMGPU_SD_PBUB * n] = bubble_point_d(T, preg, q.rs.v); o[OPMGPU_SD_PDEW * n] = dew_point_d(T, preg, q.rv.v);
}

// computeMaxDp, the per-cell part (opm/simulators/thresholdPressures.hpp:109-248): the pressure, density and saturation of every active
// phase of cell `row` (water, oil, gas) by the rules of THAT function, which are not the Newton path's:
//   p_o = the state's pressure, p_w = p_o - pcow(Sw), p_g = p_o + pcgo(Sg) with the STATE's saturations (not those implied by the phase
//   condition) through the cell's end-point and vertical scaling (hysteresis is KR-only here: no capillary-pressure history);
//   rho_w = rhoS_w b_w(p_w);
//   rho_o = rhoS_o b_o + rhoS_g Rs b_o with the state's Rs, b_o from the saturated curve at p_o when Rs >= RsSat(p_o), else the
//   undersaturated value at (p_o, Rs); RsSat is the plain curve (no VAPPARS factor); without DISGAS RsSat = 0: the saturated curve;
//   rho_g = rhoS_g b_g + rhoS_o Rv b_g the same way by Rv >= RvSat(p_g) at p_g.
// KM_OW: water and oil only, the dead-oil curve, no gas table and no gas density read; the gas slots come back as p_o, 0, 0.
template <int KM>
__device__ void max_dp_cell(const DevTables& D, int row, const CellPlanes& C, double (&pp)[3], double (&rho)[3], double (&s)[3])
{
    const opmgpu_tables& T = D.t; const TabX& X = D.x;
    const int preg = C.pvtnum[row], sreg = C.satnum[row];
    const double p = C.p[row];
    EpsD E;
    eps_load(C.eps, C.eps_u0, C.nbp, row, sreg, E);
    s[0] = C.sw[row]; s[1] = C.so[row]; s[2] = km_model(KM) == KM_OW ? 0.0 : C.sg[row];
    double f, df;
    const int wa = T.swof_ptr[sreg], nw = T.swof_ptr[sreg + 1] - wa;
    sat_curve_s<false>(T.swof_sw + wa, T.swof_pcow + wa, X.swof_dpcow + wa, nw, s[0], E, EC_PCOW, f, df);
    pp[0] = p - f; pp[1] = p; pp[2] = p;
    const double* rhos = T.surface_density + 3 * preg;
    rho[0] = rhos[0] * water_invb_value(T.pvtw + 5 * preg, pp[0]);
    const int oa = T.oil_node_ptr[preg], on = T.oil_node_ptr[preg + 1] - oa;
    if constexpr (km_model(KM) == KM_OW) {
        if (X.oil_pvcdo) f = oil_pvcdo_invb_value(X.oil_pvcdo + 5 * preg, p);
        else lin_at(T.oil_psat + oa, T.oil_invb_sat + oa, X.oil_dinvb_sat + oa, pvt_seg(T.oil_psat + oa, on, p), p, f, df);
        rho[1] = rhos[1] * f; rho[2] = 0.0;
    } else {
        const int ga = T.sgof_ptr[sreg], ng = T.sgof_ptr[sreg + 1] - ga;
        sat_curve_s<true>(T.sgof_sg + ga, T.sgof_pcgo + ga, X.sgof_dpcgo + ga, ng, s[2], E, EC_PCGO, f, df);
        pp[2] = p + f;
        const double rs = C.rs[row], rv = C.rv[row];
        double b;
        if (X.oil_pvcdo) b = oil_pvcdo_invb_value(X.oil_pvcdo + 5 * preg, p);
        else if (rs >= rs_sat_d(D, preg, p)) lin_at(T.oil_psat + oa, T.oil_invb_sat + oa, X.oil_dinvb_sat + oa, pvt_seg(T.oil_psat + oa, on, p), p, b, df);
        else b = pvt2_value(T.oil_rs + oa, on, T.oil_col_ptr + oa, T.oil_col_p, T.oil_col_invb, X.oil_col_dinvb, rs, p);
        rho[1] = rhos[1] * b + rhos[2] * rs * b;
        const int gna = T.gas_node_ptr[preg], gn = T.gas_node_ptr[preg + 1] - gna;
        if (rv >= rv_sat_d(D, preg, pp[2])) lin_at(T.gas_pg + gna, T.gas_invb_sat + gna, X.gas_dinvb_sat + gna, pvt_seg(T.gas_pg + gna, gn, pp[2]), pp[2], b, df);
        else b = pvt2_value(T.gas_pg + gna, gn, T.gas_col_ptr + gna, T.gas_col_rv, T.gas_col_invb, X.gas_col_dinvb, pp[2], rv);
        rho[2] = rhos[2] * b + rhos[1] * rv * b;
    }
}

// computeMaxDp, the per-connection part (thresholdPressures.hpp:252-297): one thread per connection; conn = the connections' two cells in
// internal numbering, eql = the cells' equilibration regions (internal numbering), sres = the residual saturations of satRange [3][nbp].
// A thread whose cells share a region -- almost every one -- leaves at once; the others evaluate BOTH end cells (each barrier face
// is a handful of threads: nothing is exchanged or accumulated).  For every active phase p1 = p(c1), p2 = p(c2) + (rho(c1) + rho(c2))/2 g
// (z1 - z2); the phase counts when (p1 > p2 && s1 > sres1) || (p2 > p1 && s2 > sres2), strict; out[f] = the largest |p1 - p2| of the
// phases that count, 0 when none does, on a connection within one region and on f >= nface (NNCs: the reference scans grid faces only).
// Off every timed path (once per run, before the first step): not tuned, not timed.
template <int KM>
__global__ __launch_bounds__(kBlock) void k_max_dp(int nconn, int nface, DevTables T, const int32_t* __restrict__ conn, const int32_t* __restrict__ eql,
                                                   CellPlanes C, const double* __restrict__ sres, const double* __restrict__ zc, double gravity,
                                                   double* __restrict__ out)
{
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= nconn) return;
    double dp = 0.0;
    const int c1 = conn[2 * long(f)], c2 = conn[2 * long(f) + 1];
    if (f < nface && eql[c1] != eql[c2]) {
        double p1[3], p2[3], r1[3], r2[3], s1[3], s2[3];
        max_dp_cell<KM>(T, c1, C, p1, r1, s1);
        max_dp_cell<KM>(T, c2, C, p2, r2, s2);
        const double dz = zc[c1] - zc[c2];
        constexpr int np = km_model(KM) == KM_OW ? 2 : 3;
#pragma unroll
        for (int ph = 0; ph < np; ++ph) {
            const double rho_avg = (r1[ph] + r2[ph]) / 2;
            const double pa = p1[ph], pb = p2[ph] + rho_avg * gravity * dz;
            if ((pa > pb && s1[ph] > sres[ph * C.nbp + c1]) || (pb > pa && s2[ph] > sres[ph * C.nbp + c2])) dp = fmax(dp, fabs(pa - pb));
        }
    }
    out[f] = dp;
}

// SWATINIT, the per-cell part of BlackoilPropsAdFromDeck::setSwatInitScaling (BlackoilPropsAdFromDeck.cpp:1009-1019): one thread per cell of
// the plan (row r, caller cell nat[r]; sw_in / pcow_in / the two outputs are in CALLER numbering, everything else internal).  The rule is
// stated in include/opmgpu.h (opmgpu_set_swatinit_scaling): pcow < 0 -> sw_out = Swu, nothing scaled; else sw_out = the imposed saturation
// clamped to [Swl, Swu], pc_at = the cell's pcow there under its current scaling (the evaluator every other kernel uses), and where
// pc_at > 0 the cell's PCW is to be multiplied by ratio = pcow / pc_at.  ratio_out = -1 marks a cell whose PCW stays (a ratio is never
// negative).  swl / swu: the cell's scaled end points, else its table's first / last Sw node (the host holds them).
// Off every timed path (once per run, before the first step): not tuned, not timed.
__global__ __launch_bounds__(kBlock) void k_swatinit(int nb, DevTables D, const int32_t* __restrict__ nat, CellPlanes C,
                                                     const double* __restrict__ swl, const double* __restrict__ swu, const double* __restrict__ sw_in,
                                                     const double* __restrict__ pcow_in, double* __restrict__ sw_out, double* __restrict__ ratio_out)
{
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nb) return;
    const opmgpu_tables& T = D.t;
    const int c = nat[r], sreg = C.satnum[r];
    const double pcow = pcow_in[c];
    double sw = swu[r], ratio = -1.0;
    if (!(pcow < 0.0)) {
        sw = fmin(fmax(sw_in[c], swl[r]), swu[r]);
        EpsD E;
        eps_load(C.eps, C.eps_u0, C.nbp, r, sreg, E);
        const int wa = T.swof_ptr[sreg], nw = T.swof_ptr[sreg + 1] - wa;
        double f, df;
        sat_curve_s<false>(T.swof_sw + wa, T.swof_pcow + wa, D.x.swof_dpcow + wa, nw, sw, E, EC_PCOW, f, df);
        if (f > 0.0) ratio = pcow / f;
    }
    sw_out[c] = sw; ratio_out[c] = ratio;
}

// capPress of the properties object (BlackoilPropsAdFromDeck::capPress): pcow = p_o - p_w at sw[r] and pcgo = p_g - p_o at sg[r] (internal
// planes) through the cell's end-point and vertical scaling, the curves the Newton path evaluates (eval_cell; hysteresis is KR-only: no
// capillary-pressure history); C.sw / C.sg are the saturations asked for, the resident planes or the caller's.  out (caller numbering): [pcow | pcgo] x nc.  No gas phase: pcgo = 0, no gas table read.  Not timed.
__global__ __launch_bounds__(kBlock) void k_cap_press(int nb, DevTables D, const int32_t* __restrict__ nat, CellPlanes C, double* __restrict__ out)
{
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nb) return;
    const opmgpu_tables& T = D.t;
    const int c = nat[r], sreg = C.satnum[r];
    EpsD E;
    eps_load(C.eps, C.eps_u0, C.nbp, r, sreg, E);
    const int wa = T.swof_ptr[sreg], nw = T.swof_ptr[sreg + 1] - wa;
    double f, df;
    sat_curve_s<false>(T.swof_sw + wa, T.swof_pcow + wa, D.x.swof_dpcow + wa, nw, C.sw[r], E, EC_PCOW, f, df);
    out[c] = f;
    f = 0.0;
    if (T.active_phases != OPMGPU_PHASES_OIL_WATER) {
        const int ga = T.sgof_ptr[sreg], ng = T.sgof_ptr[sreg + 1] - ga;
        sat_curve_s<true>(T.sgof_sg + ga, T.sgof_pcgo + ga, D.x.sgof_dpcgo + ga, ng, C.sg[r], E, EC_PCGO, f, df);
    }
    out[long(nb) + c] = f;
}

// RateConverter::SurfaceToReservoirVoidage::calcCoeff (RateConverterLegacy.hpp:495-548): coefficients c with q_rT = sum_p c[p] q_s[p] at a
// region's average state (p, rs, rv) -- b_w(p), the UNDERSATURATED b_o(p, rs) and b_g(p, rv) (FluidSystem::oilPvt().inverseFormationVolumeFactor(
// region, T, p, Rs): the tables are evaluated at the given ratios whatever the saturated curve says), detR = 1 - rs rv.
__global__ __launch_bounds__(kBlock) void k_voidage_coeff(int n, DevTables D, const double* __restrict__ press, const double* __restrict__ rs_,
                                                          const double* __restrict__ rv_, const int32_t* __restrict__ pvtreg, double* __restrict__ coeff)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double rs = rs_[i], rv = rv_[i];
    double bw, bo, bg;
    b_values(D, pvtreg ? pvtreg[i] : 0, press[i], rs, rv, !D.t.has_disgas, !D.t.has_vapoil, bw, bo, bg);
    const double detR = 1.0 - (rs * rv);
    double cw = 0.0, co = 0.0, cg = 0.0;
    cw = 1.0 / bw;                                  // q[w]_r = q[w]_s / bw
    {
        const double den = bo * detR;               // q[o]_r = 1/(bo (1 - rs rv)) (q[o]_s - rv q[g]_s)
        co += 1.0 / den;
        cg -= rv / den;
    }
    {
        const double den = bg * detR;               // q[g]_r = 1/(bg (1 - rs rv)) (q[g]_s - rs q[o]_s)
        cg += 1.0 / den;
        co -= rs / den;
    }
    if (D.t.active_phases == OPMGPU_PHASES_OIL_WATER) cg = 0.0;      // no gas phase: no gas voidage
    coeff[3 * long(i) + 0] = cw; coeff[3 * long(i) + 1] = co; coeff[3 * long(i) + 2] = cg;
}

// setSwatInitScaling (BlackoilPropsAdFromDeck.cpp:1009-1019; the rule: include/opmgpu.h).  The kernel evaluates the curve and returns the
// ratio per cell; the new PCW goes into the host copy h_eps_v[3] and from there through build_eps_planes like a PCW array given at
// creation, so a later re-plan keeps it.  A context without any scaling gets identity planes (use_eps: e.on is a run-time pointer).
void BlackoilDevice::set_swatinit_scaling(const double* sw, const double* pcow, double* sw_out)
{
    for (int c = 0; c < nc; ++c) {
        if (!std::isfinite(sw[c]) || !std::isfinite(pcow[c]))
            throw HipError(OPMGPU_EINVAL, "setSwatInitScaling: the saturation or capillary pressure of cell " + std::to_string(c) + " is not finite");
        if (sw[c] < 0.0 || sw[c] > 1.0)
            throw HipError(OPMGPU_EINVAL, "setSwatInitScaling: the water saturation of cell " + std::to_string(c) + " is outside [0, 1]");
    }
    const Plan& P = ls.plan;
    const int nbp = P.nbp;
    OPMGPU_HIP(hipStreamSynchronize(stream));
    std::vector<double> lim(2 * size_t(nbp), 0.0), in(2 * size_t(nc)), out(2 * size_t(nc));
    for (int r = 0; r < nc; ++r) {
        const int c = P.nat[r];
        const double* u = &h_unscaled[8 * size_t(h_satnum[c])];
        lim[r] = has_endpoints ? h_eps[0][c] : u[0];
        lim[size_t(nbp) + r] = has_endpoints ? h_eps[2][c] : u[2];
    }
    std::copy(sw, sw + nc, in.begin()); std::copy(pcow, pcow + nc, in.begin() + nc);
    DevArray<double> d_lim, d_in, d_out;
    d_lim.upload(lim, stream); d_in.upload(in, stream); d_out.alloc(out.size());
    hipLaunchKernelGGL(k_swatinit, dim3(grid_for(nc)), dim3(kBlock), 0, stream, nc, dtp_, ls.dp.nat.p, cell_planes(),
                       (const double*)d_lim.p, (const double*)d_lim.p + nbp, (const double*)d_in.p, (const double*)d_in.p + nc, d_out.p, d_out.p + nc);
    OPMGPU_HIP(hipGetLastError());
    d_out.download(out.data(), out.size(), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    std::vector<double> pcw(nc);
    get_pcw(pcw.data());
    for (int c = 0; c < nc; ++c) if (out[size_t(nc) + c] >= 0.0) pcw[c] *= out[size_t(nc) + c];
    h_eps_v[3] = pcw;
    use_eps = true;
    upload_drainage_eps();
    if (sw_out) std::copy(out.begin(), out.begin() + nc, sw_out);
}

// capPress for given saturations ([nc][3] water, oil, gas; caller numbering) or, sat == nullptr, the resident state's: pc = [pcow | pcgo] x nc
void BlackoilDevice::cap_press(const double* sat, double* pc)
{
    const Plan& P = ls.plan;
    const int nbp = P.nbp;
    DevArray<double> d_s, d_out;
    CellPlanes C = cell_planes();
    if (sat) {
        std::vector<double> s(2 * size_t(nbp), 0.0);
        for (int r = 0; r < nc; ++r) { s[r] = sat[3 * size_t(P.nat[r])]; s[size_t(nbp) + r] = sat[3 * size_t(P.nat[r]) + 2]; }
        d_s.upload(s, stream);
        OPMGPU_HIP(hipStreamSynchronize(stream));
        C.sw = d_s.p; C.sg = d_s.p + nbp;
    }
    d_out.alloc(2 * size_t(nc));
    hipLaunchKernelGGL(k_cap_press, dim3(grid_for(nc)), dim3(kBlock), 0, stream, nc, dtp_, ls.dp.nat.p, C, d_out.p);
    OPMGPU_HIP(hipGetLastError());
    d_out.download(pc, 2 * size_t(nc), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

double BlackoilDevice::time_assemble(int reps, int props_only)
{
    const double dt = last_dt > 0 ? last_dt : 86400.0;
    hipEvent_t e0, e1;
    OPMGPU_HIP(hipEventCreate(&e0)); OPMGPU_HIP(hipEventCreate(&e1));
    auto launch = [&]() {
        if (props_only) launch_cell_values();
        else assemble(dt, false);
    };
    launch();
    OPMGPU_HIP(hipEventRecord(e0, stream));
    for (int i = 0; i < reps; ++i) launch();
    OPMGPU_HIP(hipEventRecord(e1, stream));
    OPMGPU_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    OPMGPU_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return double(ms) / reps;
}

void BlackoilDevice::perf_pvt(const double* press, double* out)
{
    if (nperf == 0) return;
    DevArray<double> dp_, dout; dp_.upload(press, size_t(nperf), stream); dout.alloc(5 * size_t(nperf));
    perf_pvt_device(dp_.p, dout.p, nullptr);
    OPMGPU_HIP(hipMemcpyAsync(out, dout.p, 5 * size_t(nperf) * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

void BlackoilDevice::perf_props(double* out)
{
    if (nperf == 0) return;
    perf_props_device();
    OPMGPU_HIP(hipMemcpyAsync(out, d_perf.p, size_t(nperf) * OPMGPU_PERF_K * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

// decomposed runs: v[0..n) summed (or maximised) over the ranks, in place: upload, all-reduce, download, synchronise
void BlackoilDevice::host_allreduce(double* v, int n, bool max)
{
    if (!ls.comm || n <= 0) return;
    DevArray<double> d;
    d.upload(v, size_t(n), stream);
    if (max) ls.comm->allreduce_max(d.p, n, stream);
    else ls.comm->allreduce_sum(d.p, n, stream);
    d.download(v, size_t(n), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
}
// the region loops of a decomposed run size their buffers by the caller's n: it must be the global number on every rank
void BlackoilDevice::check_global_region_count(int n, const char* who)
{
    double nmax = double(n);
    host_allreduce(&nmax, 1, true);
    if (int(nmax + 0.5) != n) throw HipError(OPMGPU_EINVAL, std::string(who) + ": pass the GLOBAL number of regions on every rank of a decomposed run");
}

// Rock regions (the rule: include/opmgpu.h at opmgpu_set_rock_regions).  The history, one thread per cell: the smallest pressure the cell
// has seen.  fmin of two finite doubles (or +inf) is exact, so a float64 restatement matches bit for bit.
__global__ __launch_bounds__(kBlock) void k_rock_history(int nb, const double* __restrict__ p, double* __restrict__ p_min)
{
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c < nb) p_min[c] = fmin(p_min[c], p[c]);
}
// The two multipliers of every cell at the resident state, in the CALLER's cell order (either output may be null): what the evaluators
// form (rock_region_eval) with rock regions, else the one rock of the tables as eval_cell reads it.
template <bool ROCK>
__global__ __launch_bounds__(kBlock) void k_rock_multipliers(int nc, DevTables D, const int32_t* __restrict__ nat, CellPlanes C, double* __restrict__ pv_mult,
                                                             double* __restrict__ trans_mult)
{
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    const double p = C.p[c];
    double pvm = 1.0, trm = 1.0, d0, d1;
    if constexpr (ROCK) {
        bool table;
        rock_region_eval(D.t, rocknum_of<KM_ROCK>(C.satnum, C.nbp, c), p, rock_pmin_of<KM_ROCK>(C.somax, C.nbp, c), table, pvm, d0, trm, d1);
    } else {
        const opmgpu_tables& T = D.t;
        if (T.rocktab_n > 0) {
            rocktab_eval(T.rocktab_p, T.rocktab_pvmult, T.rocktab_n, p, pvm, d0);
            rocktab_eval(T.rocktab_p, T.rocktab_transmult, T.rocktab_n, p, trm, d1);
        } else if (T.rock_comp != 0.0) {
            const double cp = T.rock_comp * (p - T.rock_pref);
            pvm = 1.0 + cp + 0.5 * cp * cp;
        }
    }
    if (pv_mult) pv_mult[nat[c]] = pvm;
    if (trans_mult) trans_mult[nat[c]] = trm;
}
void BlackoilDevice::update_rock_history()
{
    if (!rock_on()) throw HipError(OPMGPU_EINVAL, "opmgpu_update_rock_history: no rock regions are set (opmgpu_set_rock_regions)");
    if (!has_state) throw HipError(OPMGPU_EINVAL, "opmgpu_update_rock_history: no state is resident (opmgpu_set_state)");
    hipLaunchKernelGGL(k_rock_history, dim3(grid_for(nc)), dim3(kBlock), 0, stream, nc, (const double*)d_p.p, d_somax.p + size_t(ls.plan.nbp));
    OPMGPU_HIP(hipGetLastError());
}
void BlackoilDevice::get_rock_multipliers(double* pv_mult, double* trans_mult)
{
    if (!has_state) throw HipError(OPMGPU_EINVAL, "opmgpu_get_rock_multipliers: no state is resident (opmgpu_set_state)");
    DevArray<double> dout; dout.alloc(2 * size_t(nc));
    auto kern = rock_on() ? k_rock_multipliers<true> : k_rock_multipliers<false>;
    hipLaunchKernelGGL(kern, dim3(grid_for(nc)), dim3(kBlock), 0, stream, nc, dtp_, ls.dp.nat.p, cell_planes(), pv_mult ? dout.p : (double*)nullptr,
                       trans_mult ? dout.p + nc : (double*)nullptr);
    OPMGPU_HIP(hipGetLastError());
    if (pv_mult) dout.download(pv_mult, size_t(nc), stream);
    if (trans_mult) OPMGPU_HIP(hipMemcpyAsync(trans_mult, dout.p + nc, size_t(nc) * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

// the output record of the resident state: one launch, one copy; reads the state and writes a buffer of its own, nothing else
void BlackoilDevice::simulator_data(double* out)
{
    DevArray<double> dout; dout.alloc(size_t(OPMGPU_SIMDATA_K) * nc);
    hipLaunchKernelGGL(OPMGPU_BY_MODEL(k_simulator_data), dim3(grid_for(nc)), dim3(kBlock), 0, stream, nc, dtp_, ls.dp.nat.p, cell_planes(), dout.p);
    dout.download(out, size_t(OPMGPU_SIMDATA_K) * nc, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

// computeFluidInPlace (BlackoilModelBase_impl.hpp:2263-2445, serial and parallel branch): per-cell volumes on the device, the region sums on the host
// in cell order like the reference's loops (an output path: once per sub-step / report step).  fipnum: region per cell in the caller's
// order, 0 = in no region, nullptr = one region of all cells; values: [dims][7]; fip_cells (optional): [7][nc] like SimulatorData::fip.
void BlackoilDevice::fluid_in_place(const int32_t* fipnum, int dims, double* fip_cells, double* values)
{
    DevArray<double> dout; dout.alloc(size_t(8) * nc);
    hipLaunchKernelGGL(OPMGPU_BY_MODEL(k_fip_cells), dim3(grid_for(nc)), dim3(kBlock), 0, stream, nc, dtp_, ls.dp.nat.p, d_pv.p, cell_planes(), dout.p);
    std::vector<double> h(size_t(8) * nc);
    dout.download(h.data(), h.size(), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    const double *pvol = h.data() + size_t(5) * nc, *pres_c = h.data() + size_t(6) * nc, *hyd = h.data() + size_t(7) * nc;
    // decomposed runs (the reference's parallel branch, :2369-2446): every rank sums over the cells it OWNS (caller cells [0, n_owned)),
    // the regions' hydrocarbon pore volumes / pressure sums and finally the region values are summed over the ranks; `dims` must be the
    // GLOBAL number of regions on every rank (the reference takes comm.max of the local maxima; here the buffer is the caller's)
    const int n_own = ls.comm ? n_owned_cells : nc;
    check_global_region_count(dims, "computeFluidInPlace");
    for (int i = 0; i < dims * 7; ++i) values[i] = 0.0;
    auto region = [&](int c) { return fipnum ? fipnum[c] - 1 : 0; };
    for (int ph = 0; ph < 5; ++ph)                       // phases, then the rs / rv volumes (:2312-2332)
        for (int c = 0; c < n_own; ++c) { const int r = region(c); if (r != -1) values[r * 7 + ph] += h[size_t(ph) * nc + c]; }
    std::vector<double> hp(2 * size_t(dims), 0.0);       // hydrocarbon pore volume | pv-weighted pressure sum, per region
    double* hcpv = hp.data(); double* pres = hp.data() + dims;
    for (int c = 0; c < n_own; ++c) { const int r = region(c); if (r != -1) { hcpv[r] += pvol[c] * hyd[c]; pres[r] += pvol[c] * pres_c[c]; } }
    host_allreduce(hp.data(), 2 * dims, false);                       // comm.sum(hcpv), comm.sum(pres)
    std::vector<double> fpv(nc, 0.0), fwp(nc, 0.0);
    for (int c = 0; c < n_own; ++c) {
        const int r = region(c);
        if (r == -1) continue;
        fpv[c] = pvol[c];
        // hydrocarbon-pore-volume weighted average pressure; a region without hydrocarbons: as the reference writes it (:2356-2360)
        if (hcpv[r] != 0) fwp[c] = pvol[c] * pres_c[c] * hyd[c] / hcpv[r];
        else fwp[c] = pres[r] / pvol[c];
        values[r * 7 + 5] += fpv[c];
        values[r * 7 + 6] += fwp[c];
    }
    host_allreduce(values, dims * 7, false);                       // one sum for all regions (the reference loops comm.sum over the regions)
    if (fip_cells) {
        std::copy(h.begin(), h.begin() + size_t(5) * nc, fip_cells);
        std::copy(fpv.begin(), fpv.end(), fip_cells + size_t(5) * nc);
        std::copy(fwp.begin(), fwp.end(), fip_cells + size_t(6) * nc);
    }
}

// computeMaxDp (opm/simulators/thresholdPressures.hpp:46-298) for the resident state: the per-connection potential differences on the
// device (k_max_dp), the maxima per pair of regions on the host over the downloaded plane, in connection order like the reference's face
// loop.  eqlnum: 1-based region per cell, caller order; max_dp: [nregions][nregions], symmetric, -1 = no face connection joins the pair
// (the reference's "pair absent from the map"), 0 = joined, but no phase ever counts.  The residual saturations are satRange's
// (SaturationPropsFromDeck.cpp:212-250) from the end points the host holds: SWL, SGL, max(0, 1 - SWU - SGU) -- the cell's scaled values,
// else its region's table's; with two phases max(0, 1 - SWU).  Decomposed runs: collective; every rank scans its local face connections
// (one seen from both sides is harmless to a max) and passes the GLOBAL number of regions; the maxima are max-reduced over the ranks.
void BlackoilDevice::compute_max_dp(const int32_t* eqlnum, int nregions, int n_face_conn, double* dp_conn, double* max_dp)
{
    const Plan& P = ls.plan;
    const int nbp = P.nbp;
    check_global_region_count(nregions, "computeMaxDp");
    std::vector<double> dp(std::max(nconn, 1), 0.0);
    if (nconn > 0) {
        std::vector<int32_t> hc(2 * size_t(nconn)), he(nbp, 0);
        for (size_t i = 0; i < hc.size(); ++i) hc[i] = P.pos[h_conn[i]];
        std::vector<double> sres(3 * size_t(nbp), 0.0);
        for (int r = 0; r < nc; ++r) {
            const int c = P.nat[r];
            he[r] = eqlnum[c];
            const double* u = &h_unscaled[8 * size_t(h_satnum[c])];
            auto end_point = [&](int k) { return has_endpoints ? h_eps[k][c] : u[k]; };
            sres[r] = end_point(0);
            sres[size_t(2) * nbp + r] = oil_water() ? 0.0 : end_point(4);
            double so_min = 1.0;
            so_min -= end_point(2);
            if (!oil_water()) so_min -= end_point(6);
            sres[size_t(nbp) + r] = std::max(0.0, so_min);
        }
        DevArray<int32_t> d_conn, d_eql;
        DevArray<double> d_sres, d_out;
        d_conn.upload(hc, stream); d_eql.upload(he, stream); d_sres.upload(sres, stream);
        d_out.alloc(size_t(nconn));
        hipLaunchKernelGGL(OPMGPU_BY_MODEL_PLAIN(k_max_dp), dim3(grid_for(nconn)), dim3(kBlock), 0, stream, nconn, n_face_conn, dtp_, d_conn.p, d_eql.p,
                           cell_planes(), d_sres.p, (const double*)d_zc.p, gravity, d_out.p);
        OPMGPU_HIP(hipGetLastError());
        d_out.download(dp.data(), size_t(nconn), stream);
        OPMGPU_HIP(hipStreamSynchronize(stream));
    }
    const size_t nn = size_t(nregions) * nregions;
    for (size_t i = 0; i < nn; ++i) max_dp[i] = -1.0;
    for (int f = 0; f < n_face_conn; ++f) {
        const int a = eqlnum[h_conn[2 * size_t(f)]] - 1, b = eqlnum[h_conn[2 * size_t(f) + 1]] - 1;
        if (a == b) continue;
        double& m = max_dp[size_t(a) * nregions + b];
        m = std::max(std::max(m, 0.0), dp[f]);
        max_dp[size_t(b) * nregions + a] = m;
    }
    host_allreduce(max_dp, int(nn), true);
    if (dp_conn) std::copy(dp.begin(), dp.begin() + nconn, dp_conn);
}

// RateConverter::SurfaceToReservoirVoidage::calcAverages (RateConverterLegacy.hpp:718-768), the sums only: per region sum of p, rs, rv over the
// cells and their number, in cell order like the reference's loop; decomposed runs: over the OWNED cells, then summed over the ranks (its
// is_parallel branch).  region: per cell in the caller's order, values 0 .. nregions-1 (nullptr = one region: what SimulatorBase builds,
// SimulatorBase_impl.hpp:66).  sums: [nregions][4] = sum p, sum rs, sum rv, n.  An output-cadence path (once per report step).
void BlackoilDevice::region_state_sums(const int32_t* region, int nregions, double* sums)
{
    std::vector<double> p(nc), sat(3 * size_t(nc)), rs(nc), rv(nc);
    std::vector<int8_t> hc(nc);
    get_state(p.data(), sat.data(), rs.data(), rv.data(), hc.data());
    const int n_own = ls.comm ? n_owned_cells : nc;
    for (int i = 0; i < 4 * nregions; ++i) sums[i] = 0.0;
    for (int c = 0; c < n_own; ++c) {
        const int r = region ? region[c] : 0;
        if (r < 0 || r >= nregions) throw HipError(OPMGPU_EINVAL, "region_state_sums: region index out of range");
        sums[4 * r + 0] += p[c]; sums[4 * r + 1] += rs[c]; sums[4 * r + 2] += rv[c]; sums[4 * r + 3] += 1.0;
    }
    host_allreduce(sums, 4 * nregions, false);
}

void BlackoilDevice::voidage_coefficients(int n, const double* p, const double* rs, const double* rv, const int32_t* pvtreg, double* coeff)
{
    if (n <= 0) return;
    if (pvtreg) for (int i = 0; i < n; ++i) if (pvtreg[i] < 0 || pvtreg[i] >= dto_.t.n_pvt_regions) throw HipError(OPMGPU_EINVAL, "voidage_coefficients: PVT region out of range");
    DevArray<double> din, dout; DevArray<int32_t> dreg;
    std::vector<double> h(3 * size_t(n));
    std::copy(p, p + n, h.begin()); std::copy(rs, rs + n, h.begin() + n); std::copy(rv, rv + n, h.begin() + 2 * size_t(n));
    din.upload(h.data(), h.size(), stream);
    if (pvtreg) dreg.upload(pvtreg, size_t(n), stream);
    dout.alloc(3 * size_t(n));
    hipLaunchKernelGGL(k_voidage_coeff, dim3(grid_for(n)), dim3(kBlock), 0, stream, n, dtp_, din.p, din.p + n, din.p + 2 * size_t(n),
                       pvtreg ? (const int32_t*)dreg.p : (const int32_t*)nullptr, dout.p);
    dout.download(coeff, 3 * size_t(n), stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

void BlackoilDevice::get_residual(double* r)
{
    ls.vec_to_host<double>(d_R.p, VEC_EQUATION_MAJOR, r);
}

} // namespace opmgpu
