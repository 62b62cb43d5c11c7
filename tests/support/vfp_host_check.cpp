// Stand-alone check of the VFP evaluators of csrc/vfp.hpp on a fixed edge list, built with -fsanitize=address,undefined (see the Makefile):
// every axis below its first node, on its first, an inner and its last node, between nodes and above the last; rates that make every
// ratio's denominator zero; zero rates; producer and injector tables; one-point axes, a two-point and a one-point THP axis, a table whose
// bhp(thp) is not sorted -- and NaN / Inf in every argument, which must terminate inside the table and come back as NaN where the argument
// is looked up on an axis of more than one point.  Exit status 0 = every check held and the sanitizers saw nothing.
#include "../../include/opmgpu.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

extern "C" int vfp_host_evaluate(int ntab, const opmgpu_vfp_table* tabs, int table, int n, const double* q, const double* thp, const double* alq,
                                 const double* bhp_in, double* bhp_out, double* dbhp_dq, double* thp_out);

namespace {

struct Table {
    std::vector<double> flo, thp, wfr, gfr, alq, data;
    opmgpu_vfp_table c;
};

// dip: the THP profile goes down between its second and third node, so bhp(thp) is not sorted
Table make(int id, bool inj, int flo_t, int wfr_t, int gfr_t, int nthp, int nwfr, int ngfr, int nalq, int nflo, bool dip)
{
    Table T;
    for (int i = 0; i < nflo; ++i) T.flo.push_back(0.001 + 0.004 * i * (1.0 + 0.5 * i));
    for (int i = 0; i < nthp; ++i) T.thp.push_back(1e6 * (1.0 + 1.5 * i + 0.25 * i * i));
    for (int i = 0; i < nwfr; ++i) T.wfr.push_back(nwfr == 1 ? 0.0 : 0.125 * i * (1.0 + i));
    for (int i = 0; i < ngfr; ++i) T.gfr.push_back(ngfr == 1 ? 0.0 : 50.0 + 64.0 * i * (1.0 + i));
    for (int i = 0; i < nalq; ++i) T.alq.push_back(nalq == 1 ? 0.0 : 100.0 * i * (1.0 + 0.5 * i));
    for (int t = 0; t < nthp; ++t) for (int w = 0; w < nwfr; ++w) for (int g = 0; g < ngfr; ++g) for (int a = 0; a < nalq; ++a) for (int f = 0; f < nflo; ++f) {
        double tp = T.thp[t] * (1.0 + 0.02 * t);
        if (dip && t == 2) tp = 0.5 * (T.thp[0] + T.thp[1]);
        T.data.push_back(8e6 + tp + 4e8 * T.flo[f] * std::sqrt(T.flo[f]) * (1.0 + T.wfr[w]) + 2e6 * T.wfr[w] * T.wfr[w] - 3e4 * std::sqrt(T.gfr[g])
                         - 2e3 * T.alq[a] * (1.0 + 0.5 * T.wfr[w]));
    }
    T.c.id = id; T.c.is_injector = inj; T.c.flo_type = flo_t; T.c.wfr_type = wfr_t; T.c.gfr_type = gfr_t; T.c.datum_depth = 2500.0;
    T.c.nflo = nflo; T.c.nthp = nthp; T.c.nwfr = nwfr; T.c.ngfr = ngfr; T.c.nalq = nalq;
    return T;
}

int failures = 0;
void check(bool ok, const char* what, int table, double a, double b, double c, double thp, double alq, double bhp)
{
    if (ok) return;
    ++failures;
    if (failures <= 20) std::printf("FAILED %s: table %d q = (%g, %g, %g) thp = %g alq = %g bhp = %g\n", what, table, a, b, c, thp, alq, bhp);
}

// below, first node, between, inner node, last node, above
std::vector<double> positions(const std::vector<double>& ax)
{
    const size_t n = ax.size();
    if (n == 1) return { ax[0] - 1.0, ax[0], ax[0] + 1.0 };
    const double span = ax[n - 1] - ax[0];
    return { ax[0] - 0.3 * span, ax[0], 0.5 * (ax[0] + ax[1]), ax[n / 2], ax[n - 1], ax[n - 1] + 0.3 * span };
}

} // namespace

int main()
{
    std::vector<Table> tabs;
    tabs.push_back(make(1, false, OPMGPU_VFP_FLO_LIQ, OPMGPU_VFP_WFR_WCT, OPMGPU_VFP_GFR_GLR, 4, 4, 4, 3, 5, false));
    tabs.push_back(make(2, false, OPMGPU_VFP_FLO_OIL, OPMGPU_VFP_WFR_WOR, OPMGPU_VFP_GFR_GOR, 3, 2, 4, 2, 6, false));
    tabs.push_back(make(3, false, OPMGPU_VFP_FLO_GAS, OPMGPU_VFP_WFR_WGR, OPMGPU_VFP_GFR_OGR, 5, 3, 2, 4, 3, false));
    tabs.push_back(make(4, true, OPMGPU_VFP_FLO_LIQ, 0, 0, 4, 1, 1, 1, 5, false));
    tabs.push_back(make(5, false, OPMGPU_VFP_FLO_OIL, OPMGPU_VFP_WFR_WOR, OPMGPU_VFP_GFR_GOR, 3, 1, 1, 1, 4, false));
    tabs.push_back(make(6, false, OPMGPU_VFP_FLO_LIQ, OPMGPU_VFP_WFR_WCT, OPMGPU_VFP_GFR_GLR, 2, 2, 2, 2, 3, false));
    tabs.push_back(make(7, false, OPMGPU_VFP_FLO_LIQ, OPMGPU_VFP_WFR_WCT, OPMGPU_VFP_GFR_GLR, 1, 2, 3, 2, 3, false));
    tabs.push_back(make(8, false, OPMGPU_VFP_FLO_LIQ, OPMGPU_VFP_WFR_WCT, OPMGPU_VFP_GFR_GLR, 5, 3, 3, 2, 4, true));
    tabs.push_back(make(9, false, OPMGPU_VFP_FLO_LIQ, OPMGPU_VFP_WFR_WCT, OPMGPU_VFP_GFR_GLR, 64, 2, 2, 2, 3, false));         // the most THP values a table may have
    std::vector<opmgpu_vfp_table> c;
    for (Table& T : tabs) {
        T.c.flo = T.flo.data(); T.c.thp = T.thp.data(); T.c.wfr = T.wfr.data(); T.c.gfr = T.gfr.data(); T.c.alq = T.alq.data(); T.c.data = T.data.data();
        if (T.c.is_injector) { T.c.wfr = T.c.gfr = T.c.alq = nullptr; }
        c.push_back(T.c);
    }
    const int ntab = int(c.size());
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    long evaluated = 0;

    for (int t = 0; t < ntab; ++t) {
        const Table& T = tabs[t];
        const double sgn = T.c.is_injector ? 1.0 : -1.0;
        // rates: zero, and magnitudes that put flo below, inside and above its axis; every combination, so each ratio meets 0/0 and x/0
        const std::vector<double> mags = { 0.0, 0.3 * T.flo[0], T.flo[0], 0.5 * (T.flo[0] + T.flo[1]), T.flo.back(), 1.5 * T.flo.back() };
        std::vector<double> q, thp, alq, bhp;
        for (double a : mags) for (double l : mags) for (double v : { 0.0, 40.0 * T.flo[0], 300.0 * T.flo[1], 2e3 * T.flo.back() })
            for (double tp : positions(T.thp)) for (double al : positions(T.alq)) {
                const double b[3] = { 5e6, 1.2e7, 4e7 };         // below, inside and above the table's bhp values, in turn
                q.push_back(sgn * a); q.push_back(sgn * l); q.push_back(sgn * v); thp.push_back(tp); alq.push_back(al); bhp.push_back(b[thp.size() % 3]);
            }
        const int n = int(thp.size());
        std::vector<double> bo(n), dq(3 * n), to(n);
        if (vfp_host_evaluate(ntab, c.data(), t, n, q.data(), thp.data(), alq.data(), bhp.data(), bo.data(), dq.data(), to.data()) != OPMGPU_OK) { std::printf("table %d refused\n", t); return 1; }
        evaluated += n;
        for (int i = 0; i < n; ++i) {
            check(std::isfinite(bo[i]) && std::isfinite(dq[3 * i]) && std::isfinite(dq[3 * i + 1]) && std::isfinite(dq[3 * i + 2]), "finite bhp and gradient",
                  t, q[3 * i], q[3 * i + 1], q[3 * i + 2], thp[i], alq[i], bhp[i]);
            check(T.c.nthp == 1 ? to[i] == T.thp[0] : std::isfinite(to[i]), "finite thp", t, q[3 * i], q[3 * i + 1], q[3 * i + 2], thp[i], alq[i], bhp[i]);
        }

        // non-finite arguments, one at a time, at a point inside every axis
        const double fl = 0.5 * (T.flo[0] + T.flo[1]);
        const double base[6] = { sgn * 0.2 * fl, sgn * 0.8 * fl, sgn * 150.0 * fl, 0.5 * (T.thp[0] + T.thp[T.c.nthp > 1 ? 1 : 0]), T.c.nalq > 1 ? 0.5 * (T.alq[0] + T.alq[1]) : 0.0, 1.2e7 };
        for (int k = 0; k < 6; ++k) for (double bad : { nan, inf, -inf }) {
            double p[6]; for (int j = 0; j < 6; ++j) p[j] = base[j];
            p[k] = bad;
            double b1 = 0.0, d1[3] = { 0.0, 0.0, 0.0 }, t1 = 0.0;
            if (vfp_host_evaluate(ntab, c.data(), t, 1, p, p + 3, p + 4, p + 5, &b1, d1, &t1) != OPMGPU_OK) { std::printf("table %d refused\n", t); return 1; }
            ++evaluated;
            if (bad != bad) {
                // a NaN flo: every table looks flo up (its type decides which rates it is made of)
                const bool in_flo = (k == 1 && T.c.flo_type != OPMGPU_VFP_FLO_GAS) || (k == 0 && T.c.flo_type == OPMGPU_VFP_FLO_LIQ) || (k == 2 && T.c.flo_type == OPMGPU_VFP_FLO_GAS);
                if (in_flo) check(b1 != b1 && (T.c.nthp == 1 || t1 != t1), "NaN flo gives NaN", t, p[0], p[1], p[2], p[3], p[4], p[5]);
                if (k == 3 && T.c.nthp > 1) check(b1 != b1, "NaN thp gives NaN", t, p[0], p[1], p[2], p[3], p[4], p[5]);
                if (k == 4 && T.c.nalq > 1) check(b1 != b1 && (T.c.nthp == 1 || t1 != t1), "NaN alq gives NaN", t, p[0], p[1], p[2], p[3], p[4], p[5]);
                if (k == 5 && T.c.nthp > 1) check(t1 != t1, "NaN bhp gives NaN", t, p[0], p[1], p[2], p[3], p[4], p[5]);
            }
        }
    }
    // an unknown table is refused
    double z[6] = { 0, 0, 0, 0, 0, 0 }, o[5];
    if (vfp_host_evaluate(ntab, c.data(), ntab, 1, z, z + 3, z + 4, z + 5, o, o + 1, o + 4) != OPMGPU_EINVAL) { std::printf("unknown table accepted\n"); return 1; }
    std::printf("vfp_host_check: %ld evaluations on %d tables, %d failed checks\n", evaluated, ntab, failures);
    return failures ? 1 : 0;
}
