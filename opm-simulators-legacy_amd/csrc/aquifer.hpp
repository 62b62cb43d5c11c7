// aquifer.hpp -- analytic aquifers (Fetkovich, Carter-Tracy) as source terms of the water equation: what BlackoilDevice keeps for them.
// The rule is stated in include/opmgpu.h at opmgpu_set_aquifers; the kernels are in aquifer.hip.
#ifndef OPMGPU_AQUIFER_HPP
#define OPMGPU_AQUIFER_HPP

#include "blackoil.hpp"

namespace opmgpu {

// per aquifer: the parameters (set once), the scalars of the begun step (k_aquifer_scalars), the committed state
enum { AQP_PA0 = 0, AQP_DATUM, AQP_CTV0, AQP_J, AQP_BETA, AQP_TC, AQP_COUNT };
enum { AQI_KIND = 0, AQI_TAB, AQI_NTAB, AQI_COUNT };                 // kind, first row and row count of the influence table
enum { AQS_B = 0 /* J E or b */, AQS_PA /* Fetkovich: p_a */, AQS_PP /* Carter-Tracy: P' */, AQS_TDEN /* T_c den */, AQS_COUNT };
enum { AQT_WE = 0, AQT_WS, AQT_T, AQT_COUNT };
// per connection: the frozen values of the begun step (k_aquifer_coeffs)
enum { AQC_RHO0 = 0, AQC_P0, AQC_A, AQC_B, AQC_COUNT };

struct BlackoilDevice::AquiferDev {
    int naq = 0, nconn = 0, ncells = 0, ntab = 0;
    // the caller's set (cells in the caller's numbering): what a re-plan rebinds from
    std::vector<int32_t> kind, tab_ptr, conn_ptr, conn_cell;
    std::vector<double> pa0, datum, CtV0, J, beta, Tc, tab_td, tab_pd, conn_alpha;
    bool begun = false;         // a step has begun: the coefficients are valid and every assembly adds the aquifers' terms
    double dt = 0.0;            // its length
    DevArray<double> par, tab /* t_D | P_D | slopes, stride ntab */, state, scal, alpha, coef, qout /* [nconn][2]: q, qs */;
    DevArray<int32_t> ipar, status, d_conn_ptr, conn_row, conn_aq;
    // the distinct connected rows with their connections in the listing order (CSR)
    DevArray<int32_t> cell_rows, cell_ptr, cell_conn;
};

} // namespace opmgpu
#endif
