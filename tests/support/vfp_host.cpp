// Host twin of the device's VFP evaluators: csrc/vfp.hpp compiled by plain g++, behind the call opmgpu_vfp_evaluate makes on the device.
// tests/test_vfp_twin.py compares it with the restatement opmgpu/vfp.py on a machine without a GPU; vfp_host_check.cpp runs the same
// code under the address and undefined-behaviour sanitizers.  Test infrastructure: nothing of the product links against it.
#include "../../opm-simulators-legacy_amd/csrc/vfp.hpp"
#include "../../include/opmgpu.h"

#include <vector>

namespace {

// the layout BlackoilDevice::set_vfp_tables (csrc/wells.hip) uploads: per table axes flo | thp | wfr | gfr | alq, then the data
struct Packed { std::vector<int32_t> meta; std::vector<double> blob, datum; };

bool pack(int ntab, const opmgpu_vfp_table* tabs, Packed& P)
{
    using namespace opmgpu;
    const double one_point[1] = { 0.0 };
    for (int t = 0; t < ntab; ++t) {
        const opmgpu_vfp_table& T = tabs[t];
        const int nwfr = T.is_injector ? 1 : T.nwfr, ngfr = T.is_injector ? 1 : T.ngfr, nalq = T.is_injector ? 1 : T.nalq;
        if (T.nflo < 1 || T.nthp < 1 || nwfr < 1 || ngfr < 1 || nalq < 1 || T.nthp > kVfpMaxThp || !T.flo || !T.thp || !T.data ||
            (!T.is_injector && (!T.wfr || !T.gfr || !T.alq))) return false;
        int32_t m[VM_COUNT] = { T.id, T.is_injector ? 1 : 0, T.flo_type, T.wfr_type, T.gfr_type, T.nflo, T.nthp, nwfr, ngfr, nalq, int32_t(P.blob.size()), 0 };
        P.blob.insert(P.blob.end(), T.flo, T.flo + T.nflo); P.blob.insert(P.blob.end(), T.thp, T.thp + T.nthp);
        const double* aw = T.is_injector ? one_point : T.wfr; const double* ag = T.is_injector ? one_point : T.gfr; const double* aa = T.is_injector ? one_point : T.alq;
        P.blob.insert(P.blob.end(), aw, aw + nwfr); P.blob.insert(P.blob.end(), ag, ag + ngfr); P.blob.insert(P.blob.end(), aa, aa + nalq);
        m[VM_DATA] = int32_t(P.blob.size());
        P.blob.insert(P.blob.end(), T.data, T.data + size_t(T.nthp) * nwfr * ngfr * nalq * T.nflo);
        P.meta.insert(P.meta.end(), m, m + VM_COUNT);
        P.datum.push_back(T.datum_depth);
    }
    return true;
}

opmgpu::VfpArgs args_of(int ntab, const Packed& P)
{
    opmgpu::VfpArgs V; V.ntab = ntab; V.meta = P.meta.data(); V.datum = P.datum.data(); V.blob = P.blob.data();
    return V;
}

} // namespace

extern "C" {

// opmgpu_vfp_evaluate on host arrays, the tables given as to opmgpu_set_vfp_tables
int vfp_host_evaluate(int ntab, const opmgpu_vfp_table* tabs, int table, int n, const double* q, const double* thp, const double* alq,
                      const double* bhp_in, double* bhp_out, double* dbhp_dq, double* thp_out)
{
    Packed P;
    if (ntab < 1 || !tabs || table < 0 || table >= ntab || n < 0 || !pack(ntab, tabs, P)) return OPMGPU_EINVAL;
    const opmgpu::VfpArgs V = args_of(ntab, P);
    for (int i = 0; i < n; ++i) {
        bhp_out[i] = opmgpu::vfp_bhp(V, table, q + 3 * i, thp[i], alq[i], dbhp_dq + 3 * i);
        thp_out[i] = opmgpu::vfp_thp(V, table, q + 3 * i, bhp_in[i], alq[i]);
    }
    return OPMGPU_OK;
}

// what vfp_bhp sees before the chain rule: vars[3i..] = flo, wfr, gfr of the rates; value[i] and partials[5i..] = d / d (thp, wfr, gfr, alq, flo)
// of the 32-corner interpolation (the flo entry along the table's own, positive axis)
int vfp_host_partials(int ntab, const opmgpu_vfp_table* tabs, int table, int n, const double* q, const double* thp, const double* alq,
                      double* vars, double* value, double* partials)
{
    using namespace opmgpu;
    Packed P;
    if (ntab < 1 || !tabs || table < 0 || table >= ntab || n < 0 || !pack(ntab, tabs, P)) return OPMGPU_EINVAL;
    const int32_t* m = P.meta.data() + VM_COUNT * table;
    const double* a_flo = P.blob.data() + m[VM_AXIS]; const double* a_thp = a_flo + m[VM_NFLO]; const double* a_wfr = a_thp + m[VM_NTHP];
    const double* a_gfr = a_wfr + m[VM_NWFR]; const double* a_alq = a_gfr + m[VM_NGFR];
    for (int i = 0; i < n; ++i) {
        double flo, wfr, gfr, dflo[3], dwfr[3], dgfr[3];
        vfp_vars(m, q + 3 * i, flo, wfr, gfr, dflo, dwfr, dgfr);
        const double sgn = m[VM_INJ] ? 1.0 : -1.0;
        const VfpInterp it[5] = { vfp_find(thp[i], a_thp, m[VM_NTHP]), vfp_find(wfr, a_wfr, m[VM_NWFR]), vfp_find(gfr, a_gfr, m[VM_NGFR]),
                                  vfp_find(alq[i], a_alq, m[VM_NALQ]), vfp_find(sgn * flo, a_flo, m[VM_NFLO]) };
        vars[3 * i] = flo; vars[3 * i + 1] = wfr; vars[3 * i + 2] = gfr;
        value[i] = vfp_interp5(P.blob.data() + m[VM_DATA], m, it, partials + 5 * i);
    }
    return OPMGPU_OK;
}

}
