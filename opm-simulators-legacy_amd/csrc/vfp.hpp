// vfp.hpp -- VFP tables for THP well control: ONE evaluator for the device (csrc/wells.hip) and for a plain C++ host build
// (tests/support/vfp_host.cpp compiles this header with g++ and compares it with the restatement opmgpu/vfp.py, axis by axis).
//
// Restates VFPProd/InjPropertiesLegacy::bhp / thp (opm/autodiff/VFPProdPropertiesLegacy.cpp:36-154, VFPInjPropertiesLegacy.cpp:36-130)
// over opm-simulators' VFPHelpers.hpp (detail::findInterpData / interpolate / getFlo / getWFR / getGFR / findTHP).
//
// meta[t][12]: id, is_injector, flo_type, wfr_type, gfr_type, nflo, nthp, nwfr, ngfr, nalq, axis offset, data offset (into blob);
// axes are stored flo | thp | wfr | gfr | alq, data [thp][wfr][gfr][alq][flo] (VFPProdTable) -- an injector table has one-point
// wfr / gfr / alq axes, so the same five-dimensional code serves both kinds.
//
// Non-finite arguments: the reference throws where it finds no interval; a kernel cannot.  Every search here is bounded by its axis, and
// a NaN flo / thp / alq / bhp comes back as NaN, which the callers' WE_BAD_RESIDUAL / NumericalIssue path reports.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define OPMGPU_VFP_HD __host__ __device__ inline
#else
#define OPMGPU_VFP_HD inline
#endif

namespace opmgpu {

struct VfpArgs { int ntab; const int32_t* meta; const double* datum; const double* blob; };
enum { VM_ID = 0, VM_INJ, VM_FLO_T, VM_WFR_T, VM_GFR_T, VM_NFLO, VM_NTHP, VM_NWFR, VM_NGFR, VM_NALQ, VM_AXIS, VM_DATA, VM_COUNT };
constexpr int kVfpMaxThp = 64;

struct VfpInterp { int i0, i1; double inv, f; };
// detail::findInterpData (opm-simulators VFPHelpers.hpp, pinned by tests/test_vfp.py on the host restatement).  The search stops at the
// last interval whatever v is: a NaN compares false everywhere and must not walk off the axis.
OPMGPU_VFP_HD VfpInterp vfp_find(double v, const double* __restrict__ ax, int n)
{
    VfpInterp r; r.i0 = 0; r.i1 = 0; r.inv = 0.0; r.f = 0.0;
    if (n == 1) return r;
    if (v < ax[0]) { r.i0 = 0; r.i1 = 1; }
    else if (v >= ax[n - 1]) { r.i0 = n - 2; r.i1 = n - 1; }
    else { int i = 1; while (i < n - 1 && !(ax[i] >= v)) ++i; r.i0 = i - 1; r.i1 = i; }
    const double a = ax[r.i0], b = ax[r.i1];
    if (b > a) { r.inv = 1.0 / (b - a); r.f = (v - a) * r.inv; }
    return r;
}
// detail::interpolate: multilinear value on the cell it[] = (thp, wfr, gfr, alq, flo) and the partial derivative along each axis
OPMGPU_VFP_HD double vfp_interp5(const double* __restrict__ data, const int32_t* __restrict__ m, const VfpInterp it[5], double d[5])
{
    const int n[5] = { m[VM_NTHP], m[VM_NWFR], m[VM_NGFR], m[VM_NALQ], m[VM_NFLO] };
    double val = 0.0;
    for (int k = 0; k < 5; ++k) d[k] = 0.0;
    for (int c = 0; c < 32; ++c) {
        long idx = 0;
        double w[5];
        for (int k = 0; k < 5; ++k) {
            const int bit = (c >> (4 - k)) & 1;
            idx = idx * n[k] + (bit ? it[k].i1 : it[k].i0);
            w[k] = bit ? it[k].f : 1.0 - it[k].f;
        }
        const double v = data[idx];
        val += w[0] * w[1] * w[2] * w[3] * w[4] * v;
        for (int k = 0; k < 5; ++k) {
            double pw = ((c >> (4 - k)) & 1) ? it[k].inv : -it[k].inv;
            for (int j = 0; j < 5; ++j) if (j != k) pw *= w[j];
            d[k] += pw * v;
        }
    }
    return val;
}
OPMGPU_VFP_HD double vfp_ratio(double num, double den) { if (den == 0.0) return 0.0; const double r = num / den; return std::isfinite(r) ? r : 0.0; }
// the table variables flo / wfr / gfr of the rates q = (aqua, liquid, vapour) and their gradients (getFlo / getWFR / getGFR + zeroIfNanInf)
OPMGPU_VFP_HD void vfp_vars(const int32_t* __restrict__ m, const double q[3], double& flo, double& wfr, double& gfr, double dflo[3], double dwfr[3], double dgfr[3])
{
    for (int k = 0; k < 3; ++k) { dflo[k] = 0.0; dwfr[k] = 0.0; dgfr[k] = 0.0; }
    const double a = q[0], l = q[1], v = q[2];
    switch (m[VM_FLO_T]) { case 0: flo = l; dflo[1] = 1.0; break; case 1: flo = a + l; dflo[0] = 1.0; dflo[1] = 1.0; break; default: flo = v; dflo[2] = 1.0; }
    double num, den, dn[3] = { 0, 0, 0 }, dd[3] = { 0, 0, 0 };
    switch (m[VM_WFR_T]) { case 0: num = a; den = l; dn[0] = 1; dd[1] = 1; break; case 1: num = a; den = a + l; dn[0] = 1; dd[0] = 1; dd[1] = 1; break; default: num = a; den = v; dn[0] = 1; dd[2] = 1; }
    wfr = vfp_ratio(num, den);
    if (den != 0.0 && std::isfinite(num / den)) for (int k = 0; k < 3; ++k) dwfr[k] = (dn[k] - wfr * dd[k]) / den;
    for (int k = 0; k < 3; ++k) { dn[k] = 0.0; dd[k] = 0.0; }
    switch (m[VM_GFR_T]) { case 0: num = v; den = l; dn[2] = 1; dd[1] = 1; break; case 1: num = v; den = l + a; dn[2] = 1; dd[0] = 1; dd[1] = 1; break; default: num = l; den = v; dn[1] = 1; dd[2] = 1; }
    gfr = vfp_ratio(num, den);
    if (den != 0.0 && std::isfinite(num / den)) for (int k = 0; k < 3; ++k) dgfr[k] = (dn[k] - gfr * dd[k]) / den;
}
// VFPProd/InjPropertiesLegacy::bhp: value and d bhp / d (aqua, liquid, vapour).  Producer rates are negative: the lookup negates flo
// and the flo term of the gradient carries a minus (VFPProdPropertiesLegacy.cpp:100, :146); injectors plus (VFPInjPropertiesLegacy.cpp:92, :119).
OPMGPU_VFP_HD double vfp_bhp(const VfpArgs& V, int t, const double q[3], double thp, double alq, double dq[3])
{
    const int32_t* m = V.meta + VM_COUNT * t;
    const double* ax = V.blob + m[VM_AXIS];
    const double* a_flo = ax; const double* a_thp = a_flo + m[VM_NFLO]; const double* a_wfr = a_thp + m[VM_NTHP];
    const double* a_gfr = a_wfr + m[VM_NWFR]; const double* a_alq = a_gfr + m[VM_NGFR];
    double flo, wfr, gfr, dflo[3], dwfr[3], dgfr[3];
    vfp_vars(m, q, flo, wfr, gfr, dflo, dwfr, dgfr);
    const double sgn = m[VM_INJ] ? 1.0 : -1.0;
    VfpInterp it[5] = { vfp_find(thp, a_thp, m[VM_NTHP]), vfp_find(wfr, a_wfr, m[VM_NWFR]), vfp_find(gfr, a_gfr, m[VM_NGFR]),
                        vfp_find(alq, a_alq, m[VM_NALQ]), vfp_find(sgn * flo, a_flo, m[VM_NFLO]) };
    double d[5];
    const double v = vfp_interp5(V.blob + m[VM_DATA], m, it, d);
    if (dq) for (int k = 0; k < 3; ++k) dq[k] = d[1] * dwfr[k] + d[2] * dgfr[k] + sgn * d[4] * dflo[k];
    return v;
}
OPMGPU_VFP_HD double vfp_find_x(double x0, double x1, double y0, double y1, double y) { return x0 + ((x1 - x0) / (y1 - y0)) * (y - y0); }
// VFPProd/InjPropertiesLegacy::thp -> detail::findTHP: invert the piecewise-linear bhp(thp axis) at the given rates.  Where no interval
// holds bhp -- a NaN bhp, or NaN table values after a NaN rate -- the end interval is taken, sorted or not, and the NaN comes back.
OPMGPU_VFP_HD double vfp_thp(const VfpArgs& V, int t, const double q[3], double bhp, double alq)
{
    const int32_t* m = V.meta + VM_COUNT * t;
    const int n = m[VM_NTHP];
    const double* ta = V.blob + m[VM_AXIS] + m[VM_NFLO];
    double b[kVfpMaxThp];
    bool sorted = true;
    for (int i = 0; i < n; ++i) { b[i] = vfp_bhp(V, t, q, ta[i], alq, nullptr); if (i > 0 && b[i - 1] > b[i]) sorted = false; }
    if (n < 2) return ta[0];
    int found = -1;
    for (int i = 0; i < n - 1; ++i) if (b[i] < bhp && bhp <= b[i + 1]) { found = i; break; }
    if (sorted) {
        if (bhp <= b[0]) return vfp_find_x(ta[0], ta[1], b[0], b[1], bhp);
        if (bhp > b[n - 1]) return vfp_find_x(ta[n - 2], ta[n - 1], b[n - 2], b[n - 1], bhp);
    }
    if (found >= 0) return vfp_find_x(ta[found], ta[found + 1], b[found], b[found + 1], bhp);
    if (bhp <= b[0]) return vfp_find_x(ta[0], ta[1], b[0], b[1], bhp);
    return vfp_find_x(ta[n - 2], ta[n - 1], b[n - 2], b[n - 1], bhp);
}

} // namespace opmgpu
