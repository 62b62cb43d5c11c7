// fluid_eval.hpp -- everything device-side that evaluates a fluid table or a cell: the V4 chain-rule type, the table lookups (PVT,
// saturation functions with end-point scaling and hysteresis, ROCKTAB, VAPPARS, Stone), the forms of the tables (for_each_table / rebase /
// resolve_tables, which upload_tables uses on the host too), eval_cell / eval_cell_ow, and eval_row over the CellPlanes bundle.
// Written independently of oracle/ (explicit chain rule, branch-free linear scans over the small tables instead of bisection).
// Included by blackoil.hip (the Newton path) and blackoil_output.hip (everything else): __forceinline__ functions and templates only.
#ifndef OPMGPU_FLUID_EVAL_HPP
#define OPMGPU_FLUID_EVAL_HPP

#include "blackoil.hpp"

namespace opmgpu {

// the instantiation of a cell-evaluating kernel template <int KM> for this deck's model (inside a BlackoilDevice method)
#define OPMGPU_BY_MODEL_(kernel, oil) (km_model(kmodel()) == KM_OW ? kernel<KM_OW | oil> : (km_model(kmodel()) == KM_STONE ? kernel<KM_STONE | oil> : (km_model(kmodel()) == KM_KILLOUGH ? kernel<KM_KILLOUGH | oil> : kernel<KM_DEFAULT | oil>)))
#define OPMGPU_BY_MODEL_PLAIN(kernel) (km_pvcdo(kmodel()) ? OPMGPU_BY_MODEL_(kernel, KM_PVCDO) : OPMGPU_BY_MODEL_(kernel, 0))      // for a kernel that evaluates no cell: KM_DRDT and KM_ROCK ignored
// with dissolution limits (KM_DRDT: never KM_OW, never KM_PVCDO) the three instantiations that carry the caps, else the ones above
// with rock regions (KM_ROCK: any of the four models, never KM_PVCDO, never KM_DRDT) the four instantiations that read the regions
#define OPMGPU_BY_MODEL(kernel) (km_rock(kmodel()) ? OPMGPU_BY_MODEL_(kernel, KM_ROCK) : (km_drdt(kmodel()) ? (km_model(kmodel()) == KM_STONE ? kernel<KM_STONE | KM_DRDT> : (km_model(kmodel()) == KM_KILLOUGH ? kernel<KM_KILLOUGH | KM_DRDT> : kernel<KM_DEFAULT | KM_DRDT>)) : OPMGPU_BY_MODEL_PLAIN(kernel)))

struct V4 { double v, p, w, x; };      // value, d/dP, d/dSw, d/dXvar

__device__ __forceinline__ V4 mk(double v, double p, double w, double x) { V4 r; r.v = v; r.p = p; r.w = w; r.x = x; return r; }
__device__ __forceinline__ V4 vmul(const V4& a, const V4& b) { return mk(a.v * b.v, a.p * b.v + a.v * b.p, a.w * b.v + a.v * b.w, a.x * b.v + a.v * b.x); }
__device__ __forceinline__ V4 vadd(const V4& a, const V4& b) { return mk(a.v + b.v, a.p + b.p, a.w + b.w, a.x + b.x); }
__device__ __forceinline__ V4 vscale(double s, const V4& a) { return mk(s * a.v, s * a.p, s * a.w, s * a.x); }
__device__ __forceinline__ V4 vdiv(const V4& a, const V4& b)
{
    const double q = a.v / b.v, ib = 1.0 / b.v;
    return mk(q, (a.p - q * b.p) * ib, (a.w - q * b.w) * ib, (a.x - q * b.x) * ib);
}
// f(g): f value, df = f'(g.v)
__device__ __forceinline__ V4 vchain(double f, double df, const V4& g) { return mk(f, df * g.p, df * g.w, df * g.x); }
__device__ __forceinline__ V4 vchain2(double f, double dfa, const V4& a, double dfb, const V4& b)
{
    return mk(f, dfa * a.p + dfb * b.p, dfa * a.w + dfb * b.w, dfa * a.x + dfb * b.x);
}

// PVT tables: linear extrapolation, opm-material Tabulated1DFunction segment rule
__device__ __forceinline__ int pvt_seg(const double* __restrict__ x, int n, double xv)
{
    int i = 0;
    if (n > 2) i = (x[1] < xv) ? 1 : 0;
    for (int k = 2; k <= n - 2; ++k) i += (x[k] <= xv) ? 1 : 0;
    return i;
}

// ENDSCALE: per curve S_unscaled = u0 + (S - s0) * k (two-point, k = (u2 - u0) / (s2 - s0)); with SCALECRS the relative-permeability
// curves go through a middle point: S >= s1 -> u1 + (S - s1) * k1 (scaledToUnscaledSatThreePoint_).  Vertical scaling (KRW / KRO / KRG /
// PCW / PCG): the table value times v = cell maximum / table maximum.  All precomputed on the host (BlackoilDevice::rebuild_structure).
// Curve order: krw, krow, pcow, krg, krog (in oil saturation), pcgo.
enum { EC_KRW = 0, EC_KROW, EC_PCOW, EC_KRG, EC_KROG, EC_PCGO, EC_COUNT };
constexpr int kEpsPlanes = 5 * EC_COUNT;       // [s0 | k | s1 | k1 | v] x 6 curves, stride nbp
constexpr int kEpsRegion = 2 * EC_COUNT;       // [u0 | u1] x 6 curves per saturation region
struct EpsD {
    bool on;
    double u0[EC_COUNT], s0[EC_COUNT], k[EC_COUNT], u1[EC_COUNT], s1[EC_COUNT], k1[EC_COUNT], v[EC_COUNT];
};
__device__ __forceinline__ void eps_load(const double* __restrict__ eps, const double* __restrict__ ureg, long nbp, int row, int sreg, EpsD& e)
{
    e.on = eps != nullptr;
    if (!e.on) return;
#pragma unroll
    for (int c = 0; c < EC_COUNT; ++c) {
        e.u0[c] = ureg[kEpsRegion * sreg + c]; e.u1[c] = ureg[kEpsRegion * sreg + EC_COUNT + c];
        e.s0[c] = eps[long(c) * nbp + row];
        e.k[c] = eps[long(EC_COUNT + c) * nbp + row];
        e.s1[c] = eps[long(2 * EC_COUNT + c) * nbp + row];
        e.k1[c] = eps[long(3 * EC_COUNT + c) * nbp + row];
        e.v[c] = eps[long(4 * EC_COUNT + c) * nbp + row];
    }
}
// scaled -> unscaled saturation of curve c and the slope of the map there
__device__ __forceinline__ double eps_map(const EpsD& e, int c, double sv, double& slope)
{
    if (sv >= e.s1[c]) { slope = e.k1[c]; return e.u1[c] + (sv - e.s1[c]) * e.k1[c]; }
    slope = e.k[c];
    return e.u0[c] + (sv - e.s0[c]) * e.k[c];
}
__device__ __forceinline__ double eps_unmap(const EpsD& e, int c, double su)       // unscaled -> scaled (inverse map)
{
    return su >= e.u1[c] && e.s1[c] < 1e30 ? e.s1[c] + (su - e.u1[c]) / e.k1[c] : e.s0[c] + (su - e.u0[c]) / e.k[c];
}
// Relative-permeability hysteresis of a cell (EclHysteresisTwoPhaseLaw, Carlson for the non-wetting phases, KR only): the history
// planes hold the smallest wetting saturation each two-phase system has seen (2.0 = none) and the shift of the imbibition curve.
// Killough's model (KM_KILLOUGH; the rule is stated in include/opmgpu.h at opmgpu_set_hysteresis_model) takes the scanning curve in ONE
// affine form, krn = R krn_imb(A0 + m S) over the abscissa S the Carlson branch shifts (Sw_ow resp. Sg): the shift planes then hold A0
// with Carlson's signs (+d_ow, -d_go) and the m / R planes are loaded by that model's kernels alone.  The trapped saturations Sncrt are
// kept for the caller (opmgpu_get_hysteresis_scanning); no evaluator reads them.
enum { HP_MDC_OW = 0, HP_MDC_GO, HP_D_OW, HP_D_GO, HP_M_OW, HP_M_GO, HP_R_OW, HP_R_GO, HP_SNCRT_OW, HP_SNCRT_GO, HP_COUNT };
struct HystD { bool on; int ireg; double mdc_ow, mdc_go, d_ow, d_go, m_ow, m_go, r_ow, r_go; };
struct HystArgs { const int32_t* imbnum; const double* hist; const double* ieps; const double* iureg; };      // kernel argument: imbnum == nullptr = no hysteresis
// The resident state as a cell evaluator reads it: the region numbers, the state planes, the end-point scaling (eps == nullptr: none), the
// VAPPARS history and the hysteresis arguments, all in internal numbering with stride nbp.  Passed to kernels by value;
// BlackoilDevice::cell_planes() is the one function that fills it.
struct CellPlanes {
    const int32_t *pvtnum, *satnum;         // satnum: with rock regions satnum | rocknum (rocknum_of)
    const double *p, *sw, *so, *sg, *rs, *rv;
    const int8_t* hc;
    const double *eps, *eps_u0, *somax;     // somax: with dissolution limits so_max | rs_cap | rv_cap (rs_cap_of / rv_cap_of), with rock regions so_max | p_min (rock_pmin_of)
    long nbp;
    HystArgs hy;
};
// DRSDT / DRVDT (KM_DRDT): the caps of a row ride behind so_max, as planes 1 and 2 of the array whose plane 0 is so_max (stride nbp; the
// array has those planes only in a context with limits, and only a KM_DRDT instantiation reads them).  +inf without.
template <int KM> __device__ __forceinline__ double rs_cap_of(const double* __restrict__ somax, long nbp, int row)
{
    if constexpr (km_drdt(KM)) return somax[nbp + row];
    else return __builtin_inf();
}
template <int KM> __device__ __forceinline__ double rv_cap_of(const double* __restrict__ somax, long nbp, int row)
{
    if constexpr (km_drdt(KM)) return somax[2 * nbp + row];
    else return __builtin_inf();
}
// Rock regions (KM_ROCK; never together with KM_DRDT): the smallest pressure a row has seen rides behind so_max as plane 1 of that array,
// the row's rock region behind satnum as plane 1 of that one (stride nbp; the arrays have those planes only in a context with rock
// regions, and only a KM_ROCK instantiation reads them).
template <int KM> __device__ __forceinline__ double rock_pmin_of(const double* __restrict__ somax, long nbp, int row)
{
    if constexpr (km_rock(KM)) return somax[nbp + row];
    else return __builtin_inf();
}
template <int KM> __device__ __forceinline__ int rocknum_of(const int32_t* __restrict__ satnum, long nbp, int row)
{
    if constexpr (km_rock(KM)) return satnum[nbp + row];
    else return 0;
}
template <int KM = KM_DEFAULT>
__device__ __forceinline__ void hyst_load(const int32_t* __restrict__ imbnum, const double* __restrict__ hist, long nbp, int row, HystD& h)
{
    h.on = imbnum != nullptr;
    if (!h.on) return;
    h.ireg = imbnum[row];
    h.mdc_ow = hist[row]; h.mdc_go = hist[nbp + row]; h.d_ow = hist[2 * nbp + row]; h.d_go = hist[3 * nbp + row];
    if constexpr (km_model(KM) == KM_KILLOUGH) {
        h.m_ow = hist[HP_M_OW * nbp + row]; h.m_go = hist[HP_M_GO * nbp + row]; h.r_ow = hist[HP_R_OW * nbp + row]; h.r_go = hist[HP_R_GO * nbp + row];
    }
}

// VAPPARS (applyVap, BlackoilPropsAdFromDeck.cpp:1052-1078): factor (so/soMax)^vap and its so-derivative
__device__ __forceinline__ void vap_factor(double vap, double so, double so_max, double& f, double& df)
{
    f = 1.0; df = 0.0;
    if (vap > 0.0 && so_max > 0.01 && so < so_max) {
        const double so_i = fmax(so, 1.4901161193847656e-08);
        f = pow(so_i / so_max, vap);
        df = vap * pow(so_i / so_max, vap - 1.0) / so_max;
    }
}
// ROCKTAB (RockCompressibility.cpp:86-125 -> Opm::linearInterpolation): left segment at a breakpoint, linear extrapolation
__device__ __forceinline__ void rocktab_eval(const double* __restrict__ x, const double* __restrict__ y, int n, double xv, double& f, double& df)
{
    int i = 0;
    for (int k = 1; k <= n - 2; ++k) i += (x[k] < xv) ? 1 : 0;
    df = (y[i + 1] - y[i]) / (x[i + 1] - x[i]);
    f = y[i] + df * (xv - x[i]);
}

// The pore-volume and the transmissibility multiplier of a cell in rock region r (the rule: include/opmgpu.h at opmgpu_set_rock_regions).
// A table region is evaluated at x = p on the curve -- REVERSIBLE, or p <= p_min: a tie is on the curve -- and at x = p_min with slope
// exactly 0 off it; the two tables share the segment (rocktab_eval's rule: the left segment at a breakpoint, the end segments
// extrapolated) and take their slopes from the blob.  A ROCK-form region (0 rows) is elastic whatever the mode: the quadratic form of
// its pair, transmissibility multiplier 1.  `table` tells the caller whether the mobilities carry a multiplier at all.
// In a context with regions the rock fields of the device form of opmgpu_tables, which nobody reads then, carry them (upload_rock_tables):
//   rocktab_p         five planes of rocktab_n words: p | pv_mult | its slopes | trans_mult | its slopes, all regions' tables end to end
//   rocktab_pvmult    [nregions][2] the pairs (p_ref, compressibility) of the ROCK form
//   rocktab_transmult [nregions + 1] int32 words: the rows of every region's table (0 rows: the ROCK form)
//   rock_comp         the mode, OPMGPU_ROCK_REVERSIBLE / _IRREVERSIBLE as a double
struct RockView { const int32_t* rock_ptr; const double *rock_ref, *rock_tab; long rock_rows; int rock_mode; };
__device__ __forceinline__ RockView rock_view(const opmgpu_tables& T)
{
    RockView X;
    X.rock_ptr = reinterpret_cast<const int32_t*>(T.rocktab_transmult); X.rock_ref = T.rocktab_pvmult; X.rock_tab = T.rocktab_p;
    X.rock_rows = T.rocktab_n; X.rock_mode = T.rock_comp != 0.0 ? OPMGPU_ROCK_IRREVERSIBLE : OPMGPU_ROCK_REVERSIBLE;
    return X;
}
__device__ __forceinline__ void rock_region_eval(const opmgpu_tables& T, int r, double p, double p_min, bool& table, double& pvm, double& dpvm, double& trm, double& dtrm)
{
    const RockView X = rock_view(T);
    const int a = X.rock_ptr[r], n = X.rock_ptr[r + 1] - a;
    table = n > 0;
    trm = 1.0; dtrm = 0.0;
    if (table) {
        const bool on_curve = X.rock_mode == OPMGPU_ROCK_REVERSIBLE || p <= p_min;
        const double xv = on_curve ? p : p_min;
        const double* __restrict__ x = X.rock_tab + a;
        const long m = X.rock_rows;
        int i = 0;
        for (int k = 1; k <= n - 2; ++k) i += (x[k] < xv) ? 1 : 0;
        const double h = xv - x[i];
        dpvm = x[2 * m + i]; pvm = x[m + i] + dpvm * h;
        dtrm = x[4 * m + i]; trm = x[3 * m + i] + dtrm * h;
        if (!on_curve) { dpvm = 0.0; dtrm = 0.0; }
    } else {
        const double pref = X.rock_ref[2 * r], comp = X.rock_ref[2 * r + 1];
        const double cp = comp * (p - pref);
        pvm = 1.0; dpvm = 0.0;
        if (comp != 0.0) { pvm = 1.0 + cp + 0.5 * cp * cp; dpvm = comp + cp * comp; }
    }
}

// Device form of the tables (struct DevTables, blackoil.hpp): the caller's arrays and, as their device-internal companions, the slope
// (y[i+1] - y[i]) / (x[i+1] - x[i]) of every segment of every 1-D table, formed once on the host by the same IEEE division a kernel
// would repeat per cell and per table (an f64 division is ~12 quarter-rate-class instructions on gfx950 and eval_cell made ~50 of them;
// it runs twice per cell and assembly, and it is VALU-bound: 3 800 static instructions in its value-only form).  Slope arrays are as
// long as their table (the last entry of a table is unused).  Every evaluator below reads the slopes: there is one family of them.

// THE list of the pointer fields of a DevTables: fd sees every `const double*&`, fi every `const int32_t*&`.  Whatever turns one form of
// the tables into another (word offsets -> device pointers on the host, -> pointers into LDS or the blob in a kernel) goes through here;
// upload_tables() is the only other place that names every array, because it alone knows their lengths.
template <class FD, class FI>
__host__ __device__ __forceinline__ void for_each_table(DevTables& D, FD&& fd, FI&& fi)
{
    opmgpu_tables& T = D.t; TabX& X = D.x;
    fd(T.surface_density); fd(T.pvtw);
    fi(T.oil_node_ptr); fd(T.oil_rs); fd(T.oil_psat); fd(T.oil_invb_sat); fd(T.oil_invbmu_sat);
    fi(T.oil_col_ptr); fd(T.oil_col_p); fd(T.oil_col_invb); fd(T.oil_col_invbmu);
    fi(T.gas_node_ptr); fd(T.gas_pg); fd(T.gas_rvsat); fd(T.gas_invb_sat); fd(T.gas_invbmu_sat);
    fi(T.gas_col_ptr); fd(T.gas_col_rv); fd(T.gas_col_invb); fd(T.gas_col_invbmu);
    fi(T.swof_ptr); fd(T.swof_sw); fd(T.swof_krw); fd(T.swof_krow); fd(T.swof_pcow);
    fi(T.sgof_ptr); fd(T.sgof_sg); fd(T.sgof_krg); fd(T.sgof_krog); fd(T.sgof_pcgo);
    fd(T.rocktab_p); fd(T.rocktab_pvmult); fd(T.rocktab_transmult);
    fd(T.stone1_exponent);
    fd(X.swof_dkrw); fd(X.swof_dkrow); fd(X.swof_dpcow); fd(X.sgof_dkrg); fd(X.sgof_dkrog); fd(X.sgof_dpcgo);
    fd(X.oil_drs); fd(X.oil_dinvb_sat); fd(X.oil_dinvbmu_sat); fd(X.oil_col_dinvb); fd(X.oil_col_dinvbmu);
    fd(X.gas_drvsat); fd(X.gas_dinvb_sat); fd(X.gas_dinvbmu_sat); fd(X.gas_col_dinvb); fd(X.gas_col_dinvbmu);
    fd(X.oil_pvcdo);
}
// the table word at offset `off` of `base` (pointer fields of the offset form hold the offset itself)
template <class P>
__host__ __device__ __forceinline__ void rebase(P*& p, const double* base) { p = reinterpret_cast<P*>(base + reinterpret_cast<size_t>(p)); }

// Tables in LDS: every table function is two dependent memory round trips (find the segment, read its end points) and a cell evaluates
// ~14 of them; from L1/L2 that chain is ~10 us of pure latency per wave, from LDS a tenth of it.  The kernels on the Newton path take the
// tables with every pointer field holding a WORD OFFSET into the blob and resolve them here against the blob's copy in LDS (LDS = true:
// the workgroup stages it first; the host chooses it when the blob fits) or against the blob itself.  With the base a compile-time choice
// every table access of the LDS instantiation is a ds_read at a 32-bit offset (rebasing generic pointers at run time, the round-2 form,
// gave flat loads with 64-bit address arithmetic: 284 v_lshl_add_u64 in the value-only kernel).
template <bool LDS>
__device__ __forceinline__ void resolve_tables(DevTables& D, const double* __restrict__ blob, int words, double* lds)
{
    const double* base = blob;
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < words; i += blockDim.x) lds[i] = blob[i];
        __syncthreads();
        base = lds;
    }
    auto rb = [&](auto*& p) { rebase(p, base); };
    for_each_table(D, rb, rb);
}

// saturation tables: LEFT = segment x[i] < xv <= x[i+1] (SWOF by Sw), RIGHT = x[i] <= xv < x[i+1] (SGOF by Sg: opm-material tabulates
// those against So).  The segment search and the evaluation are separate so that curves over the same abscissa share one search.
// clamp: -1 / +1 = constant extrapolation below / above the table.
template <bool RIGHT>
__device__ __forceinline__ int sat_seg(const double* __restrict__ x, int n, double xv, int& clamp)
{
    clamp = (xv <= x[0]) ? -1 : ((xv >= x[n - 1]) ? 1 : 0);
    int i = 0;
    for (int k = 1; k < n - 1; ++k) i += (RIGHT ? (x[k] <= xv) : (x[k] < xv)) ? 1 : 0;
    return i;
}
__device__ __forceinline__ void sat_at(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ dy, int n, int i, int clamp, double xv,
                                       double& f, double& df)
{
    if (clamp < 0) { f = y[0]; df = 0.0; return; }
    if (clamp > 0) { f = y[n - 1]; df = 0.0; return; }
    df = dy[i];
    f = y[i] + df * (xv - x[i]);
}
template <bool RIGHT>
__device__ __forceinline__ void sat_curve_s(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ dy, int n, double sv, const EpsD& e, int c,
                                            double& f, double& df)
{
    int cl;
    if (!e.on) { const int i = sat_seg<RIGHT>(x, n, sv, cl); sat_at(x, y, dy, n, i, cl, sv, f, df); return; }
    double slope;
    const double su = eps_map(e, c, sv, slope);
    const int i = sat_seg<RIGHT>(x, n, su, cl);
    sat_at(x, y, dy, n, i, cl, su, f, df);
    f *= e.v[c]; df *= slope * e.v[c];
}
__device__ __forceinline__ void lin_at(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ dy, int i, double xv, double& f, double& df)
{
    df = dy[i];
    f = y[i] + df * (xv - x[i]);
}
// UniformXTabulated2DFunction::eval for TWO functions over the same columns (1/B and 1/(B mu)): node segment i given, column searches shared
__device__ __forceinline__ void pvt2_pair(const double* __restrict__ xs, int i, const int32_t* __restrict__ cp, const double* __restrict__ cy,
                                          const double* __restrict__ cv1, const double* __restrict__ dcv1, const double* __restrict__ cv2, const double* __restrict__ dcv2,
                                          double xv, double yv, double& f1, double& dfx1, double& dfy1, double& f2, double& dfx2, double& dfy2)
{
    const double ih = 1.0 / (xs[i + 1] - xs[i]);
    const double alpha = (xv - xs[i]) * ih, oma = 1.0 - alpha;
    const int c0 = cp[i], c1 = cp[i + 1];
    const int j0 = pvt_seg(cy + c0, c1 - c0, yv), j1 = pvt_seg(cy + c1, cp[i + 2] - c1, yv);
    double s1, d1, s2, d2;
    lin_at(cy + c0, cv1 + c0, dcv1 + c0, j0, yv, s1, d1); lin_at(cy + c1, cv1 + c1, dcv1 + c1, j1, yv, s2, d2);
    f1 = s1 * oma + s2 * alpha; dfx1 = (s2 - s1) * ih; dfy1 = d1 * oma + d2 * alpha;
    lin_at(cy + c0, cv2 + c0, dcv2 + c0, j0, yv, s1, d1); lin_at(cy + c1, cv2 + c1, dcv2 + c1, j1, yv, s2, d2);
    f2 = s1 * oma + s2 * alpha; dfx2 = (s2 - s1) * ih; dfy2 = d1 * oma + d2 * alpha;
}
// the same for ONE function, value only (perforation and voidage PVT).  alpha keeps its division: pvt2_pair's reciprocal rounds differently
__device__ __forceinline__ double pvt2_value(const double* __restrict__ xs, int nn, const int32_t* __restrict__ cp, const double* __restrict__ cy,
                                             const double* __restrict__ cv, const double* __restrict__ dcv, double xv, double yv)
{
    const int i = pvt_seg(xs, nn, xv);
    const double alpha = (xv - xs[i]) / (xs[i + 1] - xs[i]);
    const int c0 = cp[i], c1 = cp[i + 1];
    double s1, s2, d;
    lin_at(cy + c0, cv + c0, dcv + c0, pvt_seg(cy + c0, c1 - c0, yv), yv, s1, d);
    lin_at(cy + c1, cv + c1, dcv + c1, pvt_seg(cy + c1, cp[i + 2] - c1, yv), yv, s2, d);
    return s1 * (1.0 - alpha) + s2 * alpha;
}
// saturated rs(p) / rv(p_g) of a PVT region's curve (0 without DISGAS / VAPOIL)
__device__ __forceinline__ double rs_sat_d(const DevTables& D, int reg, double p)
{
    if (!D.t.has_disgas) return 0.0;
    const int a = D.t.oil_node_ptr[reg];
    double f, df;
    lin_at(D.t.oil_psat + a, D.t.oil_rs + a, D.x.oil_drs + a, pvt_seg(D.t.oil_psat + a, D.t.oil_node_ptr[reg + 1] - a, p), p, f, df);
    return f;
}
__device__ __forceinline__ double rv_sat_d(const DevTables& D, int reg, double p)
{
    if (!D.t.has_vapoil) return 0.0;
    const int a = D.t.gas_node_ptr[reg];
    double f, df;
    lin_at(D.t.gas_pg + a, D.t.gas_rvsat + a, D.x.gas_drvsat + a, pvt_seg(D.t.gas_pg + a, D.t.gas_node_ptr[reg + 1] - a, p), p, f, df);
    return f;
}
// Bubble- / dew-point pressure (BlackoilPropsAdFromDeck::bubblePointPressure / dewPointPressure, BlackoilPropsAdFromDeck.cpp:959-1004).  The
// reference calls oilPvt() / gasPvt().saturationPressure of opm-material, which is not part of its tree, so the rule here is OURS: the
// pressure at which the region's plain tabulated saturated curve y(x) (oil_rs over oil_psat, gas_rvsat over gas_pg; piecewise linear, the
// end segments extrapolated, exactly what lin_at evaluates; no VAPPARS factor, which the reference applies outside the PVT object) takes
// the value v.  The segments are scanned from the lowest pressure upwards, the first and the last unbounded on their outer side; the
// first whose value range contains v gives x_i + (v - y_i) / slope_i.  0 -- the reference's "NumericalIssue: leave 0" -- when no
// segment contains v, when that segment is flat, or when the result is not finite.
__device__ __forceinline__ double sat_pressure(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ dy, int n, double v)
{
    for (int i = 0; i + 1 < n; ++i) {
        const double y0 = y[i], y1 = y[i + 1];
        const bool first = i == 0, last = i == n - 2;
        bool in;
        if (y1 > y0) in = (first || v >= y0) && (last || v <= y1);
        else if (y1 < y0) in = (first || v <= y0) && (last || v >= y1);
        else in = v == y0;
        if (!in) continue;
        if (y1 == y0 || dy[i] == 0.0) return 0.0;
        const double r = x[i] + (v - y0) / dy[i];
        return isfinite(r) ? r : 0.0;
    }
    return 0.0;
}
__device__ __forceinline__ double bubble_point_d(const DevTables& D, int reg, double rs)
{
    if (!D.t.has_disgas) return 0.0;        // dead oil has no saturation pressure
    const int a = D.t.oil_node_ptr[reg];
    return sat_pressure(D.t.oil_psat + a, D.t.oil_rs + a, D.x.oil_drs + a, D.t.oil_node_ptr[reg + 1] - a, rs);
}
__device__ __forceinline__ double dew_point_d(const DevTables& D, int reg, double rv)
{
    if (!D.t.has_vapoil) return 0.0;        // dry gas neither
    const int a = D.t.gas_node_ptr[reg];
    return sat_pressure(D.t.gas_pg + a, D.t.gas_rvsat + a, D.x.gas_drvsat + a, D.t.gas_node_ptr[reg + 1] - a, rv);
}
// 1 / B_w at pressure p (ConstantCompressibilityWaterPvt::inverseFormationVolumeFactor; w = the region's PVTW row), value only.  It DIVIDES
// by w[1]; the Newton evaluators (water_pvt) multiply by the reciprocal, which rounds differently: the two forms stay apart.
__device__ __forceinline__ double water_invb_value(const double* __restrict__ w, double p)
{
    const double Xc = w[2] * (p - w[0]);
    return (1.0 + Xc * (1.0 + Xc / 2.0)) / w[1];
}
// 1 / B_o at pressure p of the dead oil of constant compressibility (PVCDO; o = the region's row p_ref, B_ref, C_o, mu_ref, C_v; the rule is
// ours and stated in include/opmgpu.h at opmgpu_set_pvcdo), value only.  It DIVIDES by o[1], as water_invb_value does; the Newton
// evaluators (oil_pvcdo_pair) multiply by the reciprocal.
__device__ __forceinline__ double oil_pvcdo_invb_value(const double* __restrict__ o, double p)
{
    const double Xc = o[2] * (p - o[0]);
    return (1.0 + Xc * (1.0 + Xc / 2.0)) / o[1];
}
// b_w, b_o, b_g of a PVT region at (p, rs, rv), all phases at the SAME pressure; sat_o / sat_g: oil / gas from its saturated curve
// (ConstantCompressibilityWaterPvt, LiveOilPvt, WetGasPvt: inverseFormationVolumeFactor / saturatedInverseFormationVolumeFactor)
__device__ __forceinline__ void b_values(const DevTables& D, int preg, double p, double rs, double rv, bool sat_o, bool sat_g, double& bw, double& bo, double& bg)
{
    const opmgpu_tables& T = D.t; const TabX& X = D.x;
    bw = water_invb_value(T.pvtw + 5 * preg, p);
    double df;
    const int oa = T.oil_node_ptr[preg], on = T.oil_node_ptr[preg + 1] - oa;
    if (X.oil_pvcdo) bo = oil_pvcdo_invb_value(X.oil_pvcdo + 5 * preg, p);
    else if (sat_o) lin_at(T.oil_psat + oa, T.oil_invb_sat + oa, X.oil_dinvb_sat + oa, pvt_seg(T.oil_psat + oa, on, p), p, bo, df);
    else bo = pvt2_value(T.oil_rs + oa, on, T.oil_col_ptr + oa, T.oil_col_p, T.oil_col_invb, X.oil_col_dinvb, rs, p);
    if (T.active_phases == OPMGPU_PHASES_OIL_WATER) { bg = 1.0; return; }       // the inactive phase's b (no gas table is read)
    const int ga = T.gas_node_ptr[preg], gn = T.gas_node_ptr[preg + 1] - ga;
    if (sat_g) lin_at(T.gas_pg + ga, T.gas_invb_sat + ga, X.gas_dinvb_sat + ga, pvt_seg(T.gas_pg + ga, gn, p), p, bg, df);
    else bg = pvt2_value(T.gas_pg + ga, gn, T.gas_col_ptr + ga, T.gas_col_rv, T.gas_col_invb, X.gas_col_dinvb, p, rv);
}
// a / b with ONE division (the reciprocal), value and derivatives
__device__ __forceinline__ V4 vdiv1(const V4& a, const V4& b)
{
    const double ib = 1.0 / b.v, q = a.v * ib;
    return mk(q, (a.p - q * b.p) * ib, (a.w - q * b.w) * ib, (a.x - q * b.x) * ib);
}

// Stone I / II three-phase oil relative permeability (the rule is stated in include/opmgpu.h at opmgpu_tables::threephase_model; it is
// ours, opm-material's is not in the reference tree).  krw / krg are the cell's two-phase values eval_cell has already; the two curve
// evaluations at the arguments only these laws use -- krow at Sw* alone, krog at Sg alone -- are made here, through the same scaling as
// the default model's.  The model is uniform over the deck: the caller's branch is wave-uniform.
__device__ __forceinline__ V4 stone_kro(const DevTables& DT, const EpsD& E, int sreg, int row, double sw_, const V4& W, const V4& sg, const V4& krw, const V4& krg)
{
    const opmgpu_tables& T = DT.t; const TabX& X = DT.x;
    const int wa = T.swof_ptr[sreg], nw = T.swof_ptr[sreg + 1] - wa;
    const int ga = T.sgof_ptr[sreg], ng = T.sgof_ptr[sreg + 1] - ga;
    const double* xsw = T.swof_sw + wa; const double* xsg = T.sgof_sg + ga;
    const V4 zero = mk(0, 0, 0, 0);
    const double krocw = T.swof_krow[wa] * (E.on ? E.v[EC_KROW] : 1.0);
    if (!(krocw > 0.0)) return zero;
    const bool hscaled = E.on && (E.k[EC_PCOW] != 1.0 || E.s0[EC_PCOW] != 0.0 || E.u0[EC_PCOW] != 0.0);
    const double swco = hscaled ? E.s0[EC_PCOW] : xsw[0];
    const V4 swp = (sw_ > swco) ? W : mk(swco, 0, 0, 0);
    double f, df;
    sat_curve_s<false>(xsw, T.swof_krow + wa, X.swof_dkrow + wa, nw, swp.v, E, EC_KROW, f, df);
    const V4 kow = vchain(f, df, swp);
    int cl;
    if (E.on) {     // krog is tabulated against the oil saturation 1 - Swco_table - Sg; the scaling acts on that axis (as in eval_cell)
        double slope;
        const double so_u = eps_map(E, EC_KROG, 1.0 - (swco + sg.v), slope);
        const double sgu = 1.0 - xsw[0] - so_u;
        const int i = sat_seg<true>(xsg, ng, sgu, cl);
        sat_at(xsg, T.sgof_krog + ga, X.sgof_dkrog + ga, ng, i, cl, sgu, f, df);
        f *= E.v[EC_KROG]; df *= slope * E.v[EC_KROG];
    } else { const int i = sat_seg<true>(xsg, ng, sg.v, cl); sat_at(xsg, T.sgof_krog + ga, X.sgof_dkrog + ga, ng, i, cl, sg.v, f, df); }
    const V4 kgo = vchain(f, df, sg);
    const double ik = 1.0 / krocw;
    V4 kro;
    if (T.threephase_model == OPMGPU_KRO_STONE2) {
        const V4 ab = vmul(vadd(vscale(ik, kow), krw), vadd(vscale(ik, kgo), krg));
        kro = vscale(krocw, mk(ab.v - krw.v - krg.v, ab.p - krw.p - krg.p, ab.w - krw.w - krg.w, ab.x - krw.x - krg.x));
    } else {
        const double som = DT.stone_som[row], D = 1.0 - swco - som;
        const V4 sos = mk(1.0 - swp.v - sg.v, 0, -swp.w - sg.w, -sg.x);          // So* = 1 - Sw* - Sg
        if (!(D > 0.0) || !(sos.v > som)) return zero;
        const double iD = 1.0 / D;
        const V4 sso = mk((sos.v - som) * iD, 0, sos.w * iD, sos.x * iD);
        const V4 omw = mk(1.0 - (swp.v - swco) * iD, 0, -swp.w * iD, 0);          // 1 - SSw
        const V4 omg = mk(1.0 - sg.v * iD, 0, -sg.w * iD, -sg.x * iD);            // 1 - SSg
        const V4 r = vdiv1(sso, vmul(omw, omg));
        const double eta = T.stone1_exponent[sreg], beta = pow(r.v, eta);
        kro = vscale(ik, vmul(vchain(beta, eta * beta / r.v, r), vmul(kow, kgo)));        // d r^eta = eta r^eta / r dr  (r > 0 here)
    }
    return kro.v > 0.0 ? kro : zero;
}

// ---- what eval_cell and eval_cell_ow share, each written once (the Newton path's arithmetic: reciprocals, not divisions) ----
// water PVT with derivatives (ConstantCompressibilityWaterPvt; w = the region's PVTW row) at the water pressure pw: 1 / B_w and the viscosity
__device__ __forceinline__ void water_pvt(const double* __restrict__ w, const V4& pw, V4& b, V4& mu)
{
    const double iw1 = 1.0 / w[1];
    const double Xc = w[2] * (pw.v - w[0]);
    const double bw = (1.0 + Xc * (1.0 + Xc / 2.0)) * iw1;
    const double dbw = w[2] * (1.0 + Xc) * iw1;
    b = vchain(bw, dbw, pw);
    const double c = w[2] - w[4];
    const double Y = c * (pw.v - w[0]);
    const double den = 1.0 + Y * (1.0 + Y / 2.0), iden = 1.0 / den;
    const double BM = w[3] * w[1];
    mu = vchain(BM * bw * iden, BM * (dbw * den - bw * c * (1.0 + Y)) * (iden * iden), pw);
}
// 1 / b and 1 / (b mu) of the saturated oil curve at p with their slopes (oa: the region's first node, ip: the node segment of p)
__device__ __forceinline__ void oil_sat_pair(const opmgpu_tables& T, const TabX& X, int oa, int ip, double p, double& ib, double& dibp, double& ibm, double& dibmp)
{
    lin_at(T.oil_psat + oa, T.oil_invb_sat + oa, X.oil_dinvb_sat + oa, ip, p, ib, dibp);
    lin_at(T.oil_psat + oa, T.oil_invbmu_sat + oa, X.oil_dinvbmu_sat + oa, ip, p, ibm, dibmp);
}
// the same four numbers of the dead oil of constant compressibility (PVCDO, opmgpu_set_pvcdo; o = the region's row): water_pvt's
// arithmetic with oil's row at the oil pressure, 1 / (b mu) taken directly instead of the viscosity
__device__ __forceinline__ void oil_pvcdo_pair(const double* __restrict__ o, double p, double& ib, double& dibp, double& ibm, double& dibmp)
{
    const double io1 = 1.0 / o[1], iBM = 1.0 / (o[1] * o[3]);
    const double Xc = o[2] * (p - o[0]);
    ib = (1.0 + Xc * (1.0 + Xc / 2.0)) * io1;
    dibp = o[2] * (1.0 + Xc) * io1;
    const double c = o[2] - o[4];
    const double Y = c * (p - o[0]);
    ibm = (1.0 + Y * (1.0 + Y / 2.0)) * iBM;
    dibmp = c * (1.0 + Y) * iBM;
}

struct CellEval {
    V4 pw, pg, rs, rv, sw, so, sg;
    V4 b[3], mob[3], rho[3], accum[3];
    V4 pvm;              // pore-volume multiplier (poroMult)
};
// What the output record (k_simulator_data) takes of a cell beyond CellEval: values that are locals of eval_cell.  Only the OUTPUT
// instantiation hands them out; the one on the Newton path neither computes nor carries anything for them.
struct CellOutput { double mu[3], kr[3], rsSat, rvSat; };

// SolutionState + ReservoirResidualQuant of one cell (BlackoilModelBase_impl.hpp:614-751, 1484-1497, 2009-2027)
// KM: the saturation-function model of the deck -- KM_DEFAULT the default three-phase law, KM_STONE Stone I or II (T.threephase_model says
// which), KM_OW a deck without a gas phase (T.active_phases == OPMGPU_PHASES_OIL_WATER: eval_cell_ow).  A template parameter and not a
// branch on the fields, chosen on the host for every kernel that evaluates cells: with the branch k_assemble_rows' default instantiation went from 7 to 20 spilled VGPRs.
// KM_PVCDO or-ed to it: the oil is the analytic dead oil (oil_pvcdo_pair) instead of the tabulated one -- a template parameter too: as a branch
// on DT.x.oil_pvcdo it moved the spills and the scratch of ten k_assemble_rows shapes a deck without it runs.
// KM_DRDT or-ed to a three-phase model: DRSDT / DRVDT (the rule is stated in include/opmgpu.h at opmgpu_set_dissolution_limits).  After the
// VAPPARS factor a saturated ratio above the cell's cap (strictly: a tie is not capped) is replaced by the cap, a constant; a capped cell
// with the other phase free then holds UNDERSATURATED oil (gas) at (p, cap), so its PVT takes the 2-D table.  Without the flag rs_cap /
// rv_cap are not read and every expression below folds to what it was.
// KM_ROCK or-ed to any model: rock regions (the rule is stated in include/opmgpu.h at opmgpu_set_rock_regions).  The multipliers of the
// cell come from rock_region_eval instead of the one rock of opmgpu_tables, whose fields are then not read.  Nothing else changes.
template <bool OUTPUT, bool PVCDO, bool ROCK> __device__ void eval_cell_ow(const DevTables& DT, const EpsD& E, int preg, int sreg, double p, double sw_, CellEval& q, CellOutput* out, int rreg, double p_min);
template <bool OUTPUT = false, int KM = KM_DEFAULT>
__device__ void eval_cell(const DevTables& DT, const EpsD& E, double so_max, int preg, int sreg, double p, double sw_, double sg_, double rs_, double rv_, int hc,
                          int row, CellEval& q, const HystD& H = HystD{ false, 0, 2.0, 2.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0 }, const EpsD* EI = nullptr, CellOutput* out = nullptr,
                          double rs_cap = __builtin_inf(), double rv_cap = __builtin_inf(), int rreg = 0, double p_min = __builtin_inf())
{
    if constexpr (km_model(KM) == KM_OW) { eval_cell_ow<OUTPUT, km_pvcdo(KM), km_rock(KM)>(DT, E, preg, sreg, p, sw_, q, out, rreg, p_min); return; }
    const opmgpu_tables& T = DT.t; const TabX& X = DT.x;
    const bool isSg = hc == OPMGPU_HC_GAS_AND_OIL, isRs = hc == OPMGPU_HC_OIL_ONLY, isRv = hc == OPMGPU_HC_GAS_ONLY;
    const bool freeOil = isSg || isRs, freeGas = isSg || isRv;
    const V4 P = mk(p, 1, 0, 0), W = mk(sw_, 0, 1, 0);
    const V4 Xv = mk(isRs ? rs_ : (isRv ? rv_ : sg_), 0, 0, 1);
    // sg = isSg*X + isRv*(1 - W);  so = 1 - W - sg
    V4 sg = mk(0, 0, 0, 0);
    if (isSg) sg = Xv;
    else if (isRv) sg = mk(1.0 - sw_, 0, -1, 0);
    const V4 so = mk((1.0 - sw_) - sg.v, 0, -1.0 - sg.w, -sg.x);
    q.sw = W; q.so = so; q.sg = sg;
    // saturation functions
    const int wa = T.swof_ptr[sreg], nw = T.swof_ptr[sreg + 1] - wa;
    const int ga = T.sgof_ptr[sreg], ng = T.sgof_ptr[sreg + 1] - ga;
    const double* xsw = T.swof_sw + wa; const double* xsg = T.sgof_sg + ga;
    double f, df;
    V4 krw, krg;
    const bool gas_imb = H.on && (1.0 - sg.v) > H.mdc_go;        // gas on its (shifted) imbibition curve: krn_imb(Sw + delta) = krg_imb(Sg - delta)
    if (!E.on) {
        // no end-point scaling: pcow and krw share the segment of Sw, pcgo and krg the segment of Sg
        int cw, cg;
        const int iw = sat_seg<false>(xsw, nw, sw_, cw);
        sat_at(xsw, T.swof_pcow + wa, X.swof_dpcow + wa, nw, iw, cw, sw_, f, df);
        q.pw = mk(p - f, 1, -df, 0);
        sat_at(xsw, T.swof_krw + wa, X.swof_dkrw + wa, nw, iw, cw, sw_, f, df);
        krw = mk(f, 0, df, 0);
        const int ig = sat_seg<true>(xsg, ng, sg.v, cg);
        sat_at(xsg, T.sgof_pcgo + ga, X.sgof_dpcgo + ga, ng, ig, cg, sg.v, f, df);
        q.pg = mk(p + f, 1, df * sg.w, df * sg.x);
        if (!gas_imb) { sat_at(xsg, T.sgof_krg + ga, X.sgof_dkrg + ga, ng, ig, cg, sg.v, f, df); krg = vchain(f, df, sg); }
    } else {
        sat_curve_s<false>(xsw, T.swof_pcow + wa, X.swof_dpcow + wa, nw, sw_, E, EC_PCOW, f, df);
        q.pw = mk(p - f, 1, -df, 0);
        sat_curve_s<true>(xsg, T.sgof_pcgo + ga, X.sgof_dpcgo + ga, ng, sg.v, E, EC_PCGO, f, df);
        q.pg = mk(p + f, 1, df * sg.w, df * sg.x);
        sat_curve_s<false>(xsw, T.swof_krw + wa, X.swof_dkrw + wa, nw, sw_, E, EC_KRW, f, df);
        krw = mk(f, 0, df, 0);
        if (!gas_imb) { sat_curve_s<true>(xsg, T.sgof_krg + ga, X.sgof_dkrg + ga, ng, sg.v, E, EC_KRG, f, df); krg = vchain(f, df, sg); }
    }
    if (gas_imb) {
        const int gi = T.sgof_ptr[H.ireg];
        if constexpr (km_model(KM) == KM_KILLOUGH) {      // Killough's scanning curve R krg_imb(A0 + m Sg), A0 = -d_go
            sat_curve_s<true>(T.sgof_sg + gi, T.sgof_krg + gi, X.sgof_dkrg + gi, T.sgof_ptr[H.ireg + 1] - gi, fma(H.m_go, sg.v, -H.d_go), *EI, EC_KRG, f, df);
            f *= H.r_go; df *= H.r_go * H.m_go;
        } else sat_curve_s<true>(T.sgof_sg + gi, T.sgof_krg + gi, X.sgof_dkrg + gi, T.sgof_ptr[H.ireg + 1] - gi, sg.v - H.d_go, *EI, EC_KRG, f, df);
        krg = vchain(f, df, sg);
    }
    V4 kro;
    if constexpr (km_model(KM) == KM_STONE) kro = stone_kro(DT, E, sreg, row, sw_, W, sg, krw, krg);      // (never with hysteresis: refused at creation)
    else {   // EclDefaultMaterial::krn
        // connate water of the three-phase law: the cell's scaled SWL; a set without horizontal scaling (s0 = u0 = 0, k = 1) has the table's
        const bool hscaled = E.on && (E.k[EC_PCOW] != 1.0 || E.s0[EC_PCOW] != 0.0 || E.u0[EC_PCOW] != 0.0);
        const double swco = hscaled ? E.s0[EC_PCOW] : xsw[0];
        const V4 swp = (sw_ > swco) ? W : mk(swco, 0, 0, 0);
        const V4 swow = vadd(sg, swp);
        if (H.on && swow.v > H.mdc_ow) {         // oil against water on its (shifted) imbibition curve
            const int wi = T.swof_ptr[H.ireg];
            if constexpr (km_model(KM) == KM_KILLOUGH) {  // Killough's scanning curve R krow_imb(A0 + m Sw_ow), A0 = d_ow
                sat_curve_s<false>(T.swof_sw + wi, T.swof_krow + wi, X.swof_dkrow + wi, T.swof_ptr[H.ireg + 1] - wi, fma(H.m_ow, swow.v, H.d_ow), *EI, EC_KROW, f, df);
                f *= H.r_ow; df *= H.r_ow * H.m_ow;
            } else sat_curve_s<false>(T.swof_sw + wi, T.swof_krow + wi, X.swof_dkrow + wi, T.swof_ptr[H.ireg + 1] - wi, swow.v + H.d_ow, *EI, EC_KROW, f, df);
        } else sat_curve_s<false>(xsw, T.swof_krow + wa, X.swof_dkrow + wa, nw, swow.v, E, EC_KROW, f, df);
        const V4 kow = vchain(f, df, swow);
        const V4 sgeq = mk(swow.v - swco, swow.p, swow.w, swow.x);
        int cl;
        if (E.on) {     // krog is tabulated against the oil saturation 1 - Swco_table - Sg; the scaling acts on that axis
            double slope;
            const double so_u = eps_map(E, EC_KROG, 1.0 - swow.v, slope);
            const double sgu = 1.0 - xsw[0] - so_u;
            const int i = sat_seg<true>(xsg, ng, sgu, cl);
            sat_at(xsg, T.sgof_krog + ga, X.sgof_dkrog + ga, ng, i, cl, sgu, f, df);
            f *= E.v[EC_KROG]; df *= slope * E.v[EC_KROG];
        } else { const int i = sat_seg<true>(xsg, ng, sgeq.v, cl); sat_at(xsg, T.sgof_krog + ga, X.sgof_dkrog + ga, ng, i, cl, sgeq.v, f, df); }
        const V4 kgo = vchain(f, df, sgeq);
        const double eps = 1e-5;
        const V4 den = sgeq;                                    // Sw_ow - Swco
        const V4 num = vadd(vmul(sg, kgo), vmul(mk(swp.v - swco, swp.p, swp.w, swp.x), kow));
        if (swow.v - swco < eps) {
            const V4 k2 = vscale(0.5, vadd(kow, kgo));
            if (swow.v - swco > eps / 2) {
                const V4 k1 = vdiv(num, den);
                const V4 al = mk((eps - den.v) / (eps / 2), -den.p / (eps / 2), -den.w / (eps / 2), -den.x / (eps / 2));
                const V4 oma = mk(1.0 - al.v, -al.p, -al.w, -al.x);
                kro = vadd(vmul(k2, al), vmul(k1, oma));
            } else kro = k2;
        } else kro = vdiv1(num, den);
    }
    // rs / rv (saturated curves over the nodes' pressures: the node segment of p is shared with the saturated oil PVT below, that of
    // p_g with the saturated gas PVT)
    const int oa = T.oil_node_ptr[preg], on = T.oil_node_ptr[preg + 1] - oa;
    const int gna = T.gas_node_ptr[preg], gn = T.gas_node_ptr[preg + 1] - gna;
    const int ip = pvt_seg(T.oil_psat + oa, on, p);
    const int ipg = pvt_seg(T.gas_pg + gna, gn, q.pg.v);
    V4 rsSat = mk(0, 0, 0, 0), rvSat = mk(0, 0, 0, 0);
    if (T.has_disgas) { lin_at(T.oil_psat + oa, T.oil_rs + oa, X.oil_drs + oa, ip, p, f, df); rsSat = mk(f, df, 0, 0); }
    if (T.vap2 > 0.0) { vap_factor(T.vap2, so.v, so_max, f, df); rsSat = vmul(vchain(f, df, so), rsSat); }
    bool capped_s = false, capped_v = false;
    if constexpr (km_drdt(KM)) { capped_s = rs_cap < rsSat.v; if (capped_s) rsSat = mk(rs_cap, 0, 0, 0); }
    q.rs = (T.has_disgas && isRs) ? Xv : rsSat;
    if (T.has_vapoil) { lin_at(T.gas_pg + gna, T.gas_rvsat + gna, X.gas_drvsat + gna, ipg, q.pg.v, f, df); rvSat = vchain(f, df, q.pg); }
    if (T.vap1 > 0.0) { vap_factor(T.vap1, so.v, so_max, f, df); rvSat = vmul(vchain(f, df, so), rvSat); }
    if constexpr (km_drdt(KM)) { capped_v = rv_cap < rvSat.v; if (capped_v) rvSat = mk(rv_cap, 0, 0, 0); }
    q.rv = (T.has_vapoil && isRv) ? Xv : rvSat;
    // water PVT (ConstantCompressibilityWaterPvt)
    V4 mu[3];
    water_pvt(T.pvtw + 5 * preg, q.pw, q.b[0], mu[0]);
    // oil PVT (LiveOilPvt; saturated branch when free gas is present -- and the cap does not hold rs below the curve -- or no DISGAS)
    {
        double ib, dibp, dibr = 0.0, ibm, dibmp, dibmr = 0.0;
        if constexpr (km_pvcdo(KM)) oil_pvcdo_pair(X.oil_pvcdo + 5 * preg, p, ib, dibp, ibm, dibmp);
        else if ((freeGas && !capped_s) || !T.has_disgas) oil_sat_pair(T, X, oa, ip, p, ib, dibp, ibm, dibmp);
        else {
            const int ir = pvt_seg(T.oil_rs + oa, on, q.rs.v);
            pvt2_pair(T.oil_rs + oa, ir, T.oil_col_ptr + oa, T.oil_col_p, T.oil_col_invb, X.oil_col_dinvb, T.oil_col_invbmu, X.oil_col_dinvbmu,
                      q.rs.v, p, ib, dibr, dibp, ibm, dibmr, dibmp);
        }
        q.b[1] = vchain2(ib, dibp, P, dibr, q.rs);
        const double r = 1.0 / ibm, m = ib * r;
        mu[1] = vchain2(m, (dibp - m * dibmp) * r, P, (dibr - m * dibmr) * r, q.rs);
    }
    // gas PVT (WetGasPvt; saturated branch when free oil is present or no VAPOIL)
    {
        double ib, dibp, dibr = 0.0, ibm, dibmp, dibmr = 0.0;
        if ((freeOil && !capped_v) || !T.has_vapoil) {
            lin_at(T.gas_pg + gna, T.gas_invb_sat + gna, X.gas_dinvb_sat + gna, ipg, q.pg.v, ib, dibp);
            lin_at(T.gas_pg + gna, T.gas_invbmu_sat + gna, X.gas_dinvbmu_sat + gna, ipg, q.pg.v, ibm, dibmp);
        } else {
            pvt2_pair(T.gas_pg + gna, ipg, T.gas_col_ptr + gna, T.gas_col_rv, T.gas_col_invb, X.gas_col_dinvb, T.gas_col_invbmu, X.gas_col_dinvbmu,
                      q.pg.v, q.rv.v, ib, dibp, dibr, ibm, dibmp, dibmr);
        }
        q.b[2] = vchain2(ib, dibp, q.pg, dibr, q.rv);
        const double r = 1.0 / ibm, m = ib * r;
        mu[2] = vchain2(m, (dibp - m * dibmp) * r, q.pg, (dibr - m * dibmr) * r, q.rv);
    }
    // densities, mobilities (tr_mult == 1: no ROCKTAB)
    const double* rhos = T.surface_density + 3 * preg;
    q.rho[0] = vscale(rhos[0], q.b[0]);
    q.rho[1] = vadd(vscale(rhos[1], q.b[1]), vscale(rhos[2], vmul(q.rs, q.b[1])));
    q.rho[2] = vadd(vscale(rhos[2], q.b[2]), vscale(rhos[1], vmul(q.rv, q.b[2])));
    // accumulation with rock compressibility, transmissibility multiplier (RockCompressibility.cpp:86-125).  (This block and its two-phase
    // twin in eval_cell_ow stay inline: as a shared helper it changed k_assemble_rows' register allocation in ten shapes.)
    V4 pvm = mk(1, 0, 0, 0);
    if constexpr (km_rock(KM)) {
        bool table; double dpv, tr, dtr;
        rock_region_eval(T, rreg, p, p_min, table, f, dpv, tr, dtr); pvm = mk(f, dpv, 0, 0);
        if (table) {
            const V4 trm = mk(tr, dtr, 0, 0);
            q.mob[0] = vdiv1(vmul(trm, krw), mu[0]); q.mob[1] = vdiv1(vmul(trm, kro), mu[1]); q.mob[2] = vdiv1(vmul(trm, krg), mu[2]);
        } else {
            q.mob[0] = vdiv1(krw, mu[0]); q.mob[1] = vdiv1(kro, mu[1]); q.mob[2] = vdiv1(krg, mu[2]);
        }
    } else {
    if (T.rocktab_n > 0) {
        rocktab_eval(T.rocktab_p, T.rocktab_pvmult, T.rocktab_n, p, f, df); pvm = mk(f, df, 0, 0);
        rocktab_eval(T.rocktab_p, T.rocktab_transmult, T.rocktab_n, p, f, df);
        const V4 trm = mk(f, df, 0, 0);
        q.mob[0] = vdiv1(vmul(trm, krw), mu[0]); q.mob[1] = vdiv1(vmul(trm, kro), mu[1]); q.mob[2] = vdiv1(vmul(trm, krg), mu[2]);
    } else {
        q.mob[0] = vdiv1(krw, mu[0]); q.mob[1] = vdiv1(kro, mu[1]); q.mob[2] = vdiv1(krg, mu[2]);
    }
    if (T.rocktab_n == 0 && T.rock_comp != 0.0) {
        const double cp = T.rock_comp * (p - T.rock_pref);
        pvm = mk(1.0 + cp + 0.5 * cp * cp, T.rock_comp + cp * T.rock_comp, 0, 0);
    }
    }
    q.pvm = pvm;
    const V4 aw = vmul(vmul(pvm, q.b[0]), W);
    const V4 ao = vmul(vmul(pvm, q.b[1]), so);
    const V4 ag = vmul(vmul(pvm, q.b[2]), sg);
    q.accum[0] = aw;
    q.accum[1] = vadd(ao, vmul(q.rv, ag));
    q.accum[2] = vadd(ag, vmul(q.rs, ao));
    if constexpr (OUTPUT) {
        out->mu[0] = mu[0].v; out->mu[1] = mu[1].v; out->mu[2] = mu[2].v;
        out->kr[0] = krw.v; out->kr[1] = kro.v; out->kr[2] = krg.v;
        out->rsSat = rsSat.v; out->rvSat = rvSat.v;
    }
}
// eval_cell of a deck WITHOUT a gas phase (oil and water active; the law is stated in include/opmgpu.h at opmgpu_tables::active_phases):
// krw(Sw) and pcow(Sw) as with three phases, kro = krow(Sw) with the EC_KROW scaling -- no connate-water clamp, no blend --, the dead-oil
// PVT, So = 1 - Sw.  No gas table is touched.  The inactive gas phase presents b_g = 1, mu_g = 1, mob_g = 0, rho_g = 0, p_g = p_o,
// Sg = rs = rv = 0 with all derivatives 0, so that what still indexes three phases needs no guard; d/dXvar of everything is 0.
template <bool OUTPUT, bool PVCDO, bool ROCK>
__device__ void eval_cell_ow(const DevTables& DT, const EpsD& E, int preg, int sreg, double p, double sw_, CellEval& q, CellOutput* out, int rreg, double p_min)
{
    const opmgpu_tables& T = DT.t; const TabX& X = DT.x;
    const V4 P = mk(p, 1, 0, 0), W = mk(sw_, 0, 1, 0), zero = mk(0, 0, 0, 0), one = mk(1, 0, 0, 0);
    const V4 so = mk(1.0 - sw_, 0, -1, 0);
    q.sw = W; q.so = so; q.sg = zero; q.rs = zero; q.rv = zero; q.pg = P;
    const int wa = T.swof_ptr[sreg], nw = T.swof_ptr[sreg + 1] - wa;
    const double* xsw = T.swof_sw + wa;
    double f, df;
    V4 krw, kro;
    if (!E.on) {      // the three curves share the segment of Sw
        int cw;
        const int iw = sat_seg<false>(xsw, nw, sw_, cw);
        sat_at(xsw, T.swof_pcow + wa, X.swof_dpcow + wa, nw, iw, cw, sw_, f, df);
        q.pw = mk(p - f, 1, -df, 0);
        sat_at(xsw, T.swof_krw + wa, X.swof_dkrw + wa, nw, iw, cw, sw_, f, df);
        krw = mk(f, 0, df, 0);
        sat_at(xsw, T.swof_krow + wa, X.swof_dkrow + wa, nw, iw, cw, sw_, f, df);
        kro = mk(f, 0, df, 0);
    } else {
        sat_curve_s<false>(xsw, T.swof_pcow + wa, X.swof_dpcow + wa, nw, sw_, E, EC_PCOW, f, df);
        q.pw = mk(p - f, 1, -df, 0);
        sat_curve_s<false>(xsw, T.swof_krw + wa, X.swof_dkrw + wa, nw, sw_, E, EC_KRW, f, df);
        krw = mk(f, 0, df, 0);
        sat_curve_s<false>(xsw, T.swof_krow + wa, X.swof_dkrow + wa, nw, sw_, E, EC_KROW, f, df);
        kro = mk(f, 0, df, 0);
    }
    // water PVT (ConstantCompressibilityWaterPvt), dead-oil PVT (the saturated curve): the arithmetic of eval_cell
    V4 mu[2];
    water_pvt(T.pvtw + 5 * preg, q.pw, q.b[0], mu[0]);
    {
        const int oa = T.oil_node_ptr[preg], on = T.oil_node_ptr[preg + 1] - oa;
        double ib, dibp, ibm, dibmp;
        if constexpr (PVCDO) oil_pvcdo_pair(X.oil_pvcdo + 5 * preg, p, ib, dibp, ibm, dibmp);
        else oil_sat_pair(T, X, oa, pvt_seg(T.oil_psat + oa, on, p), p, ib, dibp, ibm, dibmp);
        q.b[1] = mk(ib, dibp, 0, 0);
        const double r = 1.0 / ibm, m = ib * r;
        mu[1] = mk(m, (dibp - m * dibmp) * r, 0, 0);
    }
    q.b[2] = one;
    const double* rhos = T.surface_density + 3 * preg;
    q.rho[0] = vscale(rhos[0], q.b[0]);
    q.rho[1] = vscale(rhos[1], q.b[1]);
    q.rho[2] = zero;
    V4 pvm = one;
    if constexpr (ROCK) {
        bool table; double dpv, tr, dtr;
        rock_region_eval(T, rreg, p, p_min, table, f, dpv, tr, dtr); pvm = mk(f, dpv, 0, 0);
        if (table) {
            const V4 trm = mk(tr, dtr, 0, 0);
            q.mob[0] = vdiv1(vmul(trm, krw), mu[0]); q.mob[1] = vdiv1(vmul(trm, kro), mu[1]);
        } else {
            q.mob[0] = vdiv1(krw, mu[0]); q.mob[1] = vdiv1(kro, mu[1]);
        }
        q.mob[2] = zero;
    } else {
    if (T.rocktab_n > 0) {
        rocktab_eval(T.rocktab_p, T.rocktab_pvmult, T.rocktab_n, p, f, df); pvm = mk(f, df, 0, 0);
        rocktab_eval(T.rocktab_p, T.rocktab_transmult, T.rocktab_n, p, f, df);
        const V4 trm = mk(f, df, 0, 0);
        q.mob[0] = vdiv1(vmul(trm, krw), mu[0]); q.mob[1] = vdiv1(vmul(trm, kro), mu[1]);
    } else {
        q.mob[0] = vdiv1(krw, mu[0]); q.mob[1] = vdiv1(kro, mu[1]);
    }
    q.mob[2] = zero;
    if (T.rocktab_n == 0 && T.rock_comp != 0.0) {
        const double cp = T.rock_comp * (p - T.rock_pref);
        pvm = mk(1.0 + cp + 0.5 * cp * cp, T.rock_comp + cp * T.rock_comp, 0, 0);
    }
    }
    q.pvm = pvm;
    q.accum[0] = vmul(vmul(pvm, q.b[0]), W);
    q.accum[1] = vmul(vmul(pvm, q.b[1]), so);
    q.accum[2] = zero;
    if constexpr (OUTPUT) {
        out->mu[0] = mu[0].v; out->mu[1] = mu[1].v; out->mu[2] = 1.0;
        out->kr[0] = krw.v; out->kr[1] = kro.v; out->kr[2] = 0.0;
        out->rsSat = 0.0; out->rvSat = 0.0;
    }
}
// eval_cell of a row's cell with what surrounds it: the cell's end-point scaling, its hysteresis history and, with one, the end points of
// its imbibition curves
template <int KM, bool OUTPUT = false>
__device__ __forceinline__ void eval_row(const DevTables& DT, int row, const CellPlanes& C, CellEval& q, CellOutput* out = nullptr)
{
    EpsD E, EI;
    HystD H;
    eps_load(C.eps, C.eps_u0, C.nbp, row, C.satnum[row], E);
    hyst_load<KM>(C.hy.imbnum, C.hy.hist, C.nbp, row, H);
    if (H.on) eps_load(C.hy.ieps, C.hy.iureg, C.nbp, row, H.ireg, EI);
    eval_cell<OUTPUT, KM>(DT, E, C.somax[row], C.pvtnum[row], C.satnum[row], C.p[row], C.sw[row], C.sg[row], C.rs[row], C.rv[row], C.hc[row], row, q, H, &EI, out,
                          rs_cap_of<KM>(C.somax, C.nbp, row), rv_cap_of<KM>(C.somax, C.nbp, row), rocknum_of<KM>(C.satnum, C.nbp, row), rock_pmin_of<KM>(C.somax, C.nbp, row));
}

} // namespace opmgpu
#endif
