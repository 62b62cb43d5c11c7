/*
 * opmgpu.h -- C ABI of libopmgpu.so: the MI355X (gfx950) fully-implicit black-oil
 * Newton step that drops in behind flow_legacy's BlackoilModel /
 * NewtonIterationBlackoilInterface.
 *
 * Every entry point names the reference interface it replaces (paths relative to
 * the OPM/opm-simulators-legacy tree).  Conventions:
 *   - plain C linkage, plain pointers + sizes, no C++/torch types cross the boundary;
 *   - every call returns an int status: OPMGPU_OK (0) or an OPMGPU_E* code that the
 *     C++ shim maps to the exception the reference would throw;
 *   - the caller owns all host buffers, the library owns all device memory behind the
 *     opaque handle; a handle is bound to ONE GPU and is not thread-safe;
 *   - there is NO CPU fallback: without a usable HIP device every compute entry
 *     point returns OPMGPU_ENODEVICE;
 *   - cell-indexed host arrays are in the CALLER's (natural) cell order, vectors of
 *     unknowns are equation-major [all p | all sw | all xvar] exactly like the
 *     reference's dx (BlackoilModelBase_impl.hpp:1162-1175);
 *   - sign convention of the Newton update: x_new = x_old - dx (ibid. :1177-1183).
 */
#ifndef OPMGPU_H
#define OPMGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -> reference exceptions (AdaptiveTimeStepping_impl.hpp:244-281) ---- */
enum {
    OPMGPU_OK = 0,
    OPMGPU_EINVAL = 1,            /* bad argument                      -> std::logic_error      */
    OPMGPU_ENODEVICE = 2,         /* no HIP device / HIP runtime error -> std::runtime_error    */
    OPMGPU_ENUMERICAL = 3,        /* NaN / too large residual          -> Opm::NumericalIssue   (BlackoilModelBase_impl.hpp:1828-1854) */
    OPMGPU_ELINSOLVE = 4,         /* linear solver did not converge    -> Opm::LinearSolverProblem (ISTLSolver.hpp:358-368) */
    OPMGPU_EBREAKDOWN = 5,        /* BiCGStab breakdown (rho/omega/h)  -> Dune::ISTLError       */
    OPMGPU_ESINGULAR = 6,         /* singular diagonal block in ILU0   -> Dune::MatrixBlockError */
    OPMGPU_ENOMEM = 7,
    OPMGPU_ECOMM = 8              /* RCCL failure                                               */
};

/* HydroCarbonState, opm/core/simulator/BlackoilState.hpp:33-37 */
enum { OPMGPU_HC_GAS_ONLY = 0, OPMGPU_HC_GAS_AND_OIL = 1, OPMGPU_HC_OIL_ONLY = 2 };

/* three-phase oil relative permeability model (opmgpu_tables.threephase_model) */
enum { OPMGPU_KRO_DEFAULT = 0, OPMGPU_KRO_STONE1 = 1, OPMGPU_KRO_STONE2 = 2 };

/* active phases (opmgpu_tables.active_phases); 0 = water, oil and gas */
enum { OPMGPU_PHASES_ALL = 0, OPMGPU_PHASES_OIL_WATER = 1 };

/* ILU0 elimination order.  NATURAL reproduces serial dune-istl bilu0 in the caller's
 * row order (level-scheduled on the device); MULTICOLOR is the reference's own
 * ilu_redblack idea (ISTLSolver.hpp:204-209) generalised to greedy colouring. */
enum { OPMGPU_ORDER_NATURAL = 0, OPMGPU_ORDER_MULTICOLOR = 1 };

typedef struct opmgpu_ctx opmgpu_ctx;

/* Static grid data = what the reference pulls from UnstructuredGrid + DerivedGeology
 * (GeoProps.hpp:84-195) + HelperOps (AutoDiffHelpers.hpp:44-174).  Connections are the
 * interior faces in grid face order followed by the NNCs; conn_cells[2*f+0] is the cell
 * with ngrad coefficient +1 (c1), conn_cells[2*f+1] the one with -1 (c2). */
typedef struct opmgpu_grid {
    int32_t        nc;          /* number of (active) cells                                     */
    int32_t        nconn;       /* interior faces + NNCs                                        */
    const int32_t* conn_cells;  /* [nconn*2]                                                    */
    const double*  trans;       /* [nconn]  transmissibility, SI: finite and >= 0 (0 is legal and
                                 * closes the connection); a negative, NaN or infinite value is
                                 * OPMGPU_EINVAL at opmgpu_create, the message names the connection */
    const double*  pv;          /* [nc]     pore volume (geo_.poreVolume())                     */
    const double*  z;           /* [nc]     cell centroid depth (geo_.z())                      */
    double         gravity;     /* geo_.gravity()[2]                                            */
    const double*  thpres;      /* [nconn] threshold pressures by connection, or NULL           */
    const int32_t* pvtnum;      /* [nc] 0-based PVT region (cellPvtRegionIdx_), or NULL (=0)    */
    const int32_t* satnum;      /* [nc] 0-based saturation region, or NULL (=0)                 */
    /* ENDSCALE (two-point saturation scaling, SCALECRS NO): per-cell scaled end points as opm-material's
     * EclEpsScalingPointsInfo holds them (materialLawParams(cell), SaturationPropsFromDeck.cpp:91-92).  Either all
     * eight are given or all are NULL (no end-point scaling).  Order: SWL SWCR SWU SOWCR SGL SGCR SGU SOGCR. */
    const double*  eps[8];
    /* SCALECRS YES: three-point horizontal scaling of the relative-permeability curves (EclEpsScalingPoints with
     * enableThreePointKrSatScaling): the critical saturation of the displacing phase is a third fixed point -- krw [SWCR,
     * 1-SOWCR-SGL, SWU], krow (in Sw) [SWL+SGL, SWCR+SGL, 1-SOWCR-SGL], krg [SGCR, 1-SOGCR-SWL, SGU], krog (in So) [SOGCR,
     * 1-SGCR-SWL, 1-SWL-SGL]; capillary pressures stay two-point.  Needs eps[]. */
    int32_t        scalecrs;
    /* vertical scaling (ENDSCALE with KRW / KRO / KRG / PCW / PCG arrays): per-cell maximum of the curve; the table value is
     * multiplied by (cell maximum / table maximum) (EclEpsTwoPhaseLaw::unscaledToScaledKrw_ etc.).  Any pointer may be NULL. */
    const double*  eps_v[5];            /* KRW, KRO, KRG, PCW, PCG */
    /* Relative-permeability hysteresis (SATOPTS HYSTER, EHYSTR item 2 = 0: Carlson's model for the non-wetting phases -- oil in the
     * oil-water system, gas in the gas-oil system -- drainage curves for the wetting phases, EHYSTR item 5 = KR: no capillary
     * pressure hysteresis; EclHysteresisTwoPhaseLaw, reached from SaturationPropsFromDeck.cpp:74-204 / updateSatHyst :206-222).
     * imbnum: 0-based saturation region of every cell's IMBIBITION curves (IMBNUM), NULL = no hysteresis.  ieps: scaled end points
     * of the imbibition curves (ISWL ISWCR ISWU ISOWCR ISGL ISGCR ISGU ISOGCR), all eight or all NULL (= the drainage ones, eps[]).
     * The history (minimum wetting saturation seen by each two-phase system) lives on the device: opmgpu_update_hysteresis.
     * EHYSTR item 2 = 2, Killough's model for the same two phases, is chosen after creation: opmgpu_set_hysteresis_model. */
    const int32_t* imbnum;
    const double*  ieps[8];
} opmgpu_grid;

/* Fluid tables, already converted to SI and pre-processed the way opm-material stores
 * them (call sites BlackoilPropsAdFromDeck.cpp:264-738, SaturationPropsFromDeck.cpp:74-204).
 * All "ptr" arrays are CSR-style offsets with one extra trailing entry. */
typedef struct opmgpu_tables {
    int32_t n_pvt_regions, n_sat_regions;
    int32_t has_disgas, has_vapoil;            /* DISGAS / VAPOIL                               */
    const double*  surface_density;            /* [n_pvt][3]  water, oil, gas                   */
    const double*  pvtw;                       /* [n_pvt][5]  pref, Bw_ref, Cw, mu_ref, Cv      */
    /* oil: saturated curve nodes (PVTO rows; PVDO = nodes with rs == 0, has_disgas == 0)       */
    const int32_t* oil_node_ptr;               /* [n_pvt+1]                                     */
    const double  *oil_rs, *oil_psat, *oil_invb_sat, *oil_invbmu_sat;   /* per node             */
    const int32_t* oil_col_ptr;                /* [n_nodes+1] undersaturated column of node     */
    const double  *oil_col_p, *oil_col_invb, *oil_col_invbmu;           /* per column sample    */
    /* gas: nodes keyed by gas pressure (PVTG; PVDG = nodes with rv == 0, has_vapoil == 0)      */
    const int32_t* gas_node_ptr;               /* [n_pvt+1]                                     */
    const double  *gas_pg, *gas_rvsat, *gas_invb_sat, *gas_invbmu_sat;  /* per node             */
    const int32_t* gas_col_ptr;                /* [n_nodes+1] column over Rv, ascending         */
    const double  *gas_col_rv, *gas_col_invb, *gas_col_invbmu;
    /* SWOF / SGOF per saturation region                                                        */
    const int32_t* swof_ptr;                   /* [n_sat+1]                                     */
    const double  *swof_sw, *swof_krw, *swof_krow, *swof_pcow;
    const int32_t* sgof_ptr;                   /* [n_sat+1]                                     */
    const double  *sgof_sg, *sgof_krg, *sgof_krog, *sgof_pcgo;
    /* ROCK (RockCompressibility.cpp:86-125, quadratic form)                                    */
    double rock_pref, rock_comp;
    /* VAPPARS (BlackoilPropsAdFromDeck.cpp:168-172, applyVap :1052-1078): rvSat *= (so/soMax)^vap1,
     * rsSat *= (so/soMax)^vap2 where soMax > 0.01 and so < soMax; 0 = off.  soMax per cell: see
     * opmgpu_set_sat_oil_max / opmgpu_update_sat_oil_max.                                       */
    double vap1, vap2;
    /* ROCKTAB (RockCompressibility.cpp:50-62, :86-125), single region: pore-volume and
     * transmissibility multipliers tabulated against pressure, piecewise linear with linear
     * extrapolation; rocktab_n == 0 = use the quadratic ROCK form above (trans multiplier 1).    */
    int32_t rocktab_n;
    const double *rocktab_p, *rocktab_pvmult, *rocktab_transmult;
    /* Three-phase oil relative permeability (the deck's STONE1 / STONE2 = STONE keywords; the reference hands the choice to the
     * material-law manager at SaturationPropsFromDeck.cpp:74-204).  OPMGPU_KRO_DEFAULT is the ECLIPSE default model, the
     * saturation-weighted blend of krow and krog.  The arithmetic of the two Stone laws belongs to opm-material, which is not part
     * of the reference tree, so THE RULE BELOW IS OURS (not pinned against opm-material), per cell and in double:
     *   Swco  = the connate water saturation of the default model: the cell's scaled SWL with end-point scaling, else the first
     *           Sw node of the cell's SWOF table;   Sw* = max(Sw, Swco)  (d Sw* / d Sw = 0 for Sw < Swco)
     *   krocw = krow(Swco) = first krow node of the region's SWOF table x the cell's vertical KRO factor (eps_v[1]) where given
     *   krw = krw(Sw), krg = krg(Sg) as in every model;  krow = the krow curve at Sw* (the water saturation alone, NOT Sw + Sg);
     *   krog = the krog curve at oil saturation 1 - Swco - Sg (the gas saturation alone); both with the cell's horizontal and
     *   vertical scaling as in the default model.
     *   STONE2:  kro = max(0, krocw [(krow/krocw + krw)(krog/krocw + krg) - krw - krg]);  0 when krocw = 0.
     *   STONE1:  Som = min(SOWCR, SOGCR) (the cell's scaled values with end-point scaling, else the critical oil saturations read
     *            off the region's tables), D = 1 - Swco - Som, So* = 1 - Sw* - Sg.  D <= 0 or So* <= Som: kro = 0.  Otherwise
     *            SSo = (So* - Som)/D, SSw = (Sw* - Swco)/D, SSg = Sg/D, beta = (SSo / ((1 - SSw)(1 - SSg)))^eta,
     *            kro = max(0, beta krow krog / krocw);  0 when krocw = 0.  eta = stone1_exponent[region] (STONE1EX), > 0.
     *   Where kro is clamped to 0 all its derivatives are 0.
     * Both laws give krow(Sw) at Sg = 0 when krog(Sg = 0) = krocw, and krog at Sw = Swco.
     * Hysteresis (opmgpu_grid.imbnum != NULL) with a Stone model is refused (OPMGPU_EINVAL): how opm-material feeds the Stone laws
     * into the hysteresis history is not recalled with confidence.  Any other value of threephase_model and an exponent <= 0 are
     * OPMGPU_EINVAL too; the text of a refused opmgpu_create is opmgpu_last_error(NULL).                                          */
    int32_t threephase_model;                  /* OPMGPU_KRO_*                                  */
    /* Active phases (the deck's OIL / WATER / GAS of RUNSPEC; the reference's phase_usage / active_[], consulted all over
     * BlackoilModelBase_impl.hpp).  0 = water + oil + gas; OPMGPU_PHASES_OIL_WATER = a deck without a gas phase.  No other set is
     * supported (oil-gas, gas-water and single-phase decks: OPMGPU_EINVAL).  The field lies in the four bytes that alignment left
     * free between threephase_model and stone1_exponent: the size of the struct and the offset of every other field are what they
     * were, and a caller that zero-initialises the struct gets today's three phases.
     * With OPMGPU_PHASES_OIL_WATER:
     *   - sgof_*, gas_*, sgof_ptr, gas_node_ptr, gas_col_ptr may be NULL (the caller's arrays are never read; the library keeps a
     *     two-row stand-in of its own for its host-side bookkeeping, which no oil-water kernel evaluates) and surface_density[..][2] is
     *     ignored; of opmgpu_grid.eps[] only SWL SWCR SWU SOWCR are read (the gas end points may be NULL; SGL counts as 0) and of
     *     eps_v[] only KRW KRO PCW.
     *   - THE LAW (opm-material's EclTwoPhaseMaterial, oil-water approach; opm-material is outside the reference tree, so as with
     *     Stone's the rule is ours): krw(Sw) and pcow(Sw) exactly as with three phases; kro = krow(Sw), the krow column of SWOF
     *     at the cell's water saturation with the cell's two- / three-point horizontal scaling and vertical KRO factor, constant
     *     beyond the table's ends.  There is no connate-water clamp and none of the default three-phase law's 1e-5 blend.
     *   - The block size stays 3.  The gas unknown is a pinned dummy: the gas equation of every cell is the identity row (diagonal
     *     entry exactly 1 whatever matbalscale[2] is, off-diagonal entries and residual exactly 0), the third column of every
     *     water / oil row is exactly 0 and the gas CPR weight is 0, so the third component of every solve's dx is exactly 0.
     *     Sg, rs and rv of the state are exactly 0 and stay so; the state's hc is ignored on input and reported as
     *     OPMGPU_HC_GAS_AND_OIL, its oil saturation is taken as given.
     *   - Where three phases are still indexed (perforation properties, simulator data, convergence, fluid in place) the inactive
     *     gas phase presents b_g = 1, mob_g = 0, rho_g = 0, p_g = p_o, kr_g = 0, mu_g = 1 (and 1 / b_g = 1 per cell in B_avg);
     *     opmgpu_voidage_coefficients gives the gas coefficient 0; the gas, dissolved-gas and vaporised-oil rows of
     *     opmgpu_compute_fluid_in_place are 0.
     *   - OPMGPU_EINVAL, with the text in opmgpu_last_error(NULL), for: has_disgas, has_vapoil, vap1 or vap2 set;
     *     threephase_model != OPMGPU_KRO_DEFAULT; hysteresis (opmgpu_grid.imbnum != NULL); any other value of active_phases.
     *     opmgpu_set_device_wells refuses (OPMGPU_EINVAL, text in opmgpu_last_error(ctx)) a well whose comp_frac has a gas entry, a
     *     control whose distribution has a gas entry, and a THP control.                                                        */
    int32_t active_phases;                     /* 0 or OPMGPU_PHASES_OIL_WATER                  */
    const double* stone1_exponent;             /* [n_sat_regions], NULL = 1.0                   */
} opmgpu_tables;

/* Newton + linear-solver knobs: BlackoilModelParameters.cpp:76-102, BlackoilModelBase_impl.hpp:139,
 * FlowLinearSolverParameters fields read at ISTLSolver.hpp:142-270. */
typedef struct opmgpu_params {
    double dp_max_rel;              /* 0.3    */
    double ds_max;                  /* 0.2    */
    double dr_max_rel;              /* 1e9    */
    double max_residual_allowed;    /* 1e7    */
    double tolerance_mb;            /* 1e-5   */
    double tolerance_cnv;           /* 1e-2   */
    double matbalscale[3];          /* {1.1169, 1.0031, 0.0031}                                 */
    double linear_solver_reduction; /* 1e-2   */
    int32_t linear_solver_maxiter;  /* 150 (solver_approach=interleaved); the reference's CPR plug-in defaults to 50 (NewtonIterationBlackoilCPR.cpp:63) */
    double ilu_relaxation;          /* 0.9    */
    int32_t ilu_ordering;           /* OPMGPU_ORDER_*                                           */
    int32_t ignore_convergence_failure; /* 0  */
    int32_t use_cpr;                /* 0 = block-ILU0 (solver_approach=interleaved, the default, FlowMain.hpp:806-830);
                                       1 = CPR: AMG V-cycle on the pressure system + block-ILU0
                                           (solver_approach=cpr, NewtonIterationBlackoilCPR.cpp:79-185)     */
    int32_t newton_use_gmres;       /* 0 = BiCGStab; 1 = Dune::RestartedGMResSolver (ISTLSolver.hpp:257-264): left-preconditioned
                                       restarted GMRES, modified Gram-Schmidt (also decomposed);
                                       2 = flexible (right-preconditioned) GMRES, NOT a reference solver: stops on the true residual like
                                           the default BiCGStab and saves the application M^-1 b, but needs more columns for the same
                                           reduction (measured 4.95 against 3.65 on the bench deck: slower) */
    int32_t linear_solver_restart;  /* 40     */
    /* well model (device wells): BlackoilModelParameters.cpp:78-79, :96, :85 */
    int32_t solve_welleq_initially; /* 1: explicit well pre-solve at the initial assembly (BlackoilModelBase_impl.hpp:827-829) */
    double tolerance_wells;         /* 1e-4   */
    double tolerance_well_control;  /* 1e-7   */
    double dbhp_max_rel;            /* 1.0    */
    int32_t update_equations_scaling; /* 0; 1: matbalscale[a] = mean over the cells of 1 / b_a of the state being assembled
                                         (BlackoilModelBase::updateEquationsScaling, BlackoilModelBase_impl.hpp:909, :919-947); the values in
                                         use are read back with opmgpu_get_matbalscale */
    int32_t gmres_verify_residual;  /* 0 = Dune::RestartedGMResSolver as it is (ISTLSolver.hpp:257-264): the iteration stops when the
                                         PRECONDITIONED residual || M^-1 (b - A x) || has fallen by linear_solver_reduction;
                                       1 = before such a solve is reported converged the TRUE residual b - A x is formed (one product) and the
                                           iteration continues from it, with a lowered threshold, until || b - A x || <= reduction || b || -- the
                                           statement the reference's default BiCGStab makes; the reported reduction is then the true one.
                                           Not a reference option; costs one SpMV per solve; left-preconditioned GMRES only.
                                           LIMIT with a float solve (single_precision = 1): b - A x is then formed in float, so the verified
                                           reduction cannot go below the rounding of that product (about 1e-6 x the conditioning of the
                                           scaled system; on the 1 M-cell bench deck a verified 1e-5 is NOT reached within 1000 iterations
                                           and the solve ends in OPMGPU_ELINSOLVE) -- ask a float solve for reductions >= 1e-3 with the
                                           check, or solve in double (tests/test_gpu_linsolver.py::test_gmres_verify_with_float_vectors) */
    int32_t cpr_reference_transform; /* 0 = CPR as DESIGN.md 4b describes it (only the pressure stage sees the combined equation);
                                        1 = the reference's formulation for comparability (NewtonIterationUtilities.cpp:253-287,
                                            NewtonIterationBlackoilCPR.cpp:117-131): the WHOLE system is row-transformed by L (per cell: its
                                            first equation is replaced by the sum of the dominant equations), the pressure row scaled by
                                            200 bar, and the Krylov method iterates on (and measures) L A x = L b;
                                        2 = 1, and the second stage is the reference's own: a POINT ILU0 of L A taken as a scalar matrix in
                                            equation-major order (`DuneMatrix istlA(A)`, NewtonIterationBlackoilCPR.cpp:129-133), where 0 and
                                            1 keep the 3x3-block ILU0.  With ilu_ordering = OPMGPU_ORDER_NATURAL this is dune's elimination
                                            order: linear iteration counts become comparable one to one with a solver_approach=cpr run of
                                            flow_legacy.  Double, single GPU; a comparison mode (the scalar plan's index lists take ~3.6 GB
                                            at 10^6 cells and a minute of host time per pattern) */
    /* --- the reference's CPR parameters (NewtonIterationBlackoilCPR.hpp:59-63 documents the first four with these defaults; they are read
     *     by the external opm-simulators CPRPreconditioner, whose source is NOT under /root/reference) ------------------------------------ */
    double cpr_relax;               /* 1.0: relaxation of the CPR preconditioner -- the ILU0 of stage 2 is built with it INSTEAD of
                                       ilu_relaxation, and a value != 1 also scales the pressure correction of stage 1 */
    int32_t cpr_ilu_n;              /* 0: fill-in level of stage 2's ILU(n) (NewtonIterationBlackoilCPR.hpp:61): n > 0 = block ILU(n) with level-of-fill, see
                                       ilu_fillin_level below.  0..8; not with cpr_reference_transform = 2 */
    int32_t cpr_use_amg;            /* 0 = the elliptic (pressure) part is preconditioned by a POINT ILU0 of A_p (the documented default),
                                       1 = by one AMG V-cycle on A_p (amg.hip) */
    int32_t cpr_use_bicgstab;       /* 1 = BiCGStab for the elliptic part, 0 = CG */
    /* the elliptic part's inner Krylov solve.  Its stopping rule lives in the external CPRPreconditioner: the two values below are this
     * library's RECOLLECTION of that file (cpr_solver_tol 1e-2, cpr_max_elliptic_iter 25), unpinned by anything in the container */
    double cpr_solver_tol;          /* 1e-2: reduction of || b_p - A_p x_p || the inner solve stops at */
    double cpr_stage2_relax;        /* 1.0.  LIBRARY EXTENSION: an extra relaxation of the second stage ALONE,
                                           M^-1 d = cpr_relax (x_p + cpr_stage2_relax ILU0^-1 (d - A x_p)).
                                       cpr_relax by itself multiplies the whole preconditioner by a scalar (that is what the reference's
                                       CPRPreconditioner::apply does with it, as recalled), which no Krylov method notices; damping stage 2
                                       against the pressure correction is a different preconditioner -- rounds 1-3 of this library ran 0.9,
                                       which is what the Norne-like deck (isolated cells) needs to reach 1e-10: tests/test_gpu_fullsize.py */
    int32_t preconditioner_single;  /* 0.  LIBRARY EXTENSION, 1 = mixed precision: a DOUBLE solve (single_precision = 0) builds and applies its
                                       preconditioner -- the ILU0 factors and sweeps, under CPR also the pressure stage and the stage-2 residual --
                                       in FLOAT; the Krylov method, its operator A, its residual and the solution stay double, so the solve meets
                                       the same reduction on the same double system.  The preconditioner's bytes are half (the path is HBM-bound).
                                       The reference's plug-ins have no such option: bench.py runs it as a variant, not as the headline.
                                       LIMIT: a float M^-1 is not one fixed linear operator (its rounding depends on the vector), which the
                                       recurrences of both Krylov methods assume -- BiCGStab stalls around 1e-9 .. 1e-10 (measured: 163
                                       iterations to 9.9e-10, then a breakdown, where the double preconditioner takes 12 iterations to
                                       7.5e-13), left-preconditioned GMRES's residual estimate drifts below ~1e-6.  Meant for the reductions
                                       Newton solves ask for (1e-2 by default); ask for no less than 1e-8 / 1e-6 with it */
    int32_t cpr_max_ell_iter;       /* 25: iteration limit of the inner solve (reaching it is NOT an error here: the outer method goes on with
                                       what the inner one attained).  0 = library extension, no inner Krylov method at all: ONE application
                                       of the elliptic preconditioner (with cpr_use_amg = 1: one V-cycle, its coarse-grid corrections scaled
                                       as DESIGN.md section 4b describes) -- what bench.py's headline runs, and says so */
    int32_t ilu_fillin_level;       /* 0: `ilu_fillin_level` of the interleaved solver (ISTLSolver.hpp:205, handed to ParallelOverlappingILU0):
                                       n > 0 = block ILU(n) with level-of-fill instead of the ILU0.  Under use_cpr the second stage takes
                                       cpr_ilu_n (above) instead.  Both run csrc/fillilu.inl: the level-of-fill rule for the pattern
                                       (lev(i,j) = min lev(i,k) + lev(k,j) + 1 <= n, rows in the caller's order; dune-istl is not in the
                                       reference tree: parity unpinned), this library's block ILU kernels on that pattern's own plan.  With
                                       ilu_ordering = OPMGPU_ORDER_NATURAL the elimination order is the caller's (dune's); MULTICOLOR colours
                                       the filled graph.  n <= 8; a filled pattern beyond 12 x the matrix's blocks is refused.  Measured
                                       (profiles/r04_aj_ilu_n.log): fewer iterations, never less time -- an option for parity of settings */
} opmgpu_params;

void opmgpu_default_params(opmgpu_params* p);
/* the equation scaling the last assembly used (== params.matbalscale unless update_equations_scaling) */
int opmgpu_get_matbalscale(opmgpu_ctx* ctx, double* scale3);
/* CPR with an inner Krylov method on the elliptic part (cpr_max_ell_iter > 0; the reference's external CPRPreconditioner::solveElliptic,
 * reached from NewtonIterationBlackoilCPR.cpp:148-165): inner solves and inner iterations since the context was created */
int opmgpu_cpr_elliptic_stats(opmgpu_ctx* ctx, int64_t* solves, int64_t* iterations);
/* diagnostic of cpr_reference_transform = 2: v = relax * (L U)^-1 d with the point ILU0 of the last such solve's (transformed) matrix;
 * d3 / v3 block-interleaved like opmgpu_ilu0_apply.  tests/test_gpu_linsolver.py checks it against a numpy ILU0 of the scalar matrix. */
int opmgpu_point_ilu_apply(opmgpu_ctx* ctx, const double* d3, double* v3, double relax);
/* diagnostic: the scaling of the pressure cycle's coarse-grid corrections the LAST CPR solve ran with (into level 0 / below it; DESIGN.md
 * section 5: 1.9, or on matrices of the model's own assembly the per-time-step choice between 1.9 and 2.3 -- and, after a failed solve, which is
 * repeated with 1.0, from the ladder 1.0 / 1.45 / 1.9 / 2.3; external matrices of the B1 path keep 1.9).  OPMGPU_EINVAL before the first CPR solve. */
int opmgpu_cpr_correction_factors(opmgpu_ctx* ctx, double* into_level0, double* below);
/* diagnostics of the pressure hierarchy of the last CPR solve, in the precision it ran in (the float work set under single precision or
 * preconditioner_single).  They change nothing the next solve sees; OPMGPU_EINVAL before the first CPR solve.  tests/test_gpu_cpr_stages.py
 * checks every level and application against a float64 restatement (tests/amg_reference.py).
 *   opmgpu_cpr_levels: *nlevels in = room in n / nnz (may be 0), out = number of levels; n[l] = rows of level l (level 0 counts its well
 *     border rows), nnz[l] = its stored entries; *nw = wells of the border (0: no border).
 *   opmgpu_cpr_level_get: level l as CSR with values widened to double.  Level 0 in caller numbering -- cells in caller order, then one
 *     row per well --, coarse levels in their own.  agg[n] = coarse row of every row (not for the last level); dense_inv = the coarsest
 *     level's explicit inverse, row-major n x n, when it has one (n <= 96).  Any output pointer may be NULL.
 *   opmgpu_cpr_vcycle_apply: x = one V-cycle from a zero start on the level-0 vector b (n[0] entries, numbered like level 0).
 *   opmgpu_cpr_apply: v3 = the whole two-stage preconditioner as a solve applies it (d3 / v3 block-interleaved like opmgpu_ilu0_apply).
 *     It takes the path of the context's last solve: behind a double GMRES solve on that path's conditions the pressure correction is
 *     added inside the ILU0 sweeps (OPMGPU_CPR_CANCEL_P) and the top level's stage-2 residual goes through the ILU0 factor
 *     (OPMGPU_CPR_FACTOR_P); behind any other solve it is the plain sequence.
 *   opmgpu_cpr_elliptic_ilu_apply: x = cpr_relax (L U)^-1 b with the point ILU0 of A_p that preconditions the inner elliptic solve
 *     (cpr_use_amg = 0, cpr_max_ell_iter > 0); border rows by their own diagonal.  b / x numbered like level 0. */
int opmgpu_cpr_levels(opmgpu_ctx* ctx, int32_t* nlevels, int32_t* n, int64_t* nnz, int32_t* nw);
int opmgpu_cpr_level_get(opmgpu_ctx* ctx, int level, int32_t* rowptr, int32_t* col, double* val, int32_t* agg, double* dense_inv);
int opmgpu_cpr_vcycle_apply(opmgpu_ctx* ctx, const double* b, double* x);
/* The distributed pressure hierarchy (opmgpu_comm_set_pressure_hierarchy mode 1) in global numbering.
 *   opmgpu_cpr_dist_levels: number of levels, and how many of them are distributed (0: a rank-local or single-domain hierarchy); the
 *   levels behind those are replicated on every rank.
 *   opmgpu_cpr_dist_level_get: counts[0] = rows returned, counts[1] = their entries (every other pointer may be NULL to ask for these).
 *   A distributed level returns this rank's owned rows: level 0 in caller-local numbering (owned cells in order, columns may be ghost
 *   cells, the wells at n_local + k), coarser ones with global row and column ids.  A replicated level returns the whole matrix.
 *   agg_gid = global id of the aggregate of every row (-1 on the coarsest level).
 * On a decomposed context with the distributed hierarchy opmgpu_cpr_vcycle_apply is collective and b / x hold the rank's owned cells,
 * then its wells. */
int opmgpu_cpr_dist_levels(opmgpu_ctx* ctx, int32_t* nlevels, int32_t* ndist);
int opmgpu_cpr_dist_level_get(opmgpu_ctx* ctx, int level, int64_t* counts, int64_t* row_gid, int32_t* rowptr, int64_t* col_gid, double* val,
                              int64_t* agg_gid);
int opmgpu_cpr_apply(opmgpu_ctx* ctx, const double* d3, double* v3);
int opmgpu_cpr_elliptic_ilu_apply(opmgpu_ctx* ctx, const double* b, double* x);

/* ------------------------------------------------------------------------------------------
 * B2 boundary: BlackoilModel hooks (BlackoilModelBase_impl.hpp:239-326: assemble ->
 * getConvergence -> solveJacobianSystem -> updateState).
 * ---------------------------------------------------------------------------------------- */

/* Replaces the BlackoilModel constructor's static inputs (BlackoilModel.hpp:63-79): grid,
 * BlackoilPropsAdFromDeck, DerivedGeology, RockCompressibility, model parameters.
 * Persists across report steps (SimulatorBase_impl.hpp:201-203 rebuilds the model object,
 * the device context lives with the linear solver, FlowMain.hpp:237). */
int opmgpu_create(opmgpu_ctx** ctx, int device, const opmgpu_grid* grid,
                  const opmgpu_tables* tables, const opmgpu_params* params);
void opmgpu_destroy(opmgpu_ctx* ctx);
/* Text of the context's last error.  ctx == NULL: the text of the calling thread's last REFUSED opmgpu_create (which leaves no
 * context behind), "null context" when there was none. */
const char* opmgpu_last_error(const opmgpu_ctx* ctx);

/* Wells topology (Wells::well_connpos / well_cells).  The BSR pattern becomes
 * stencil U per-well cliques, the fill eliminateVariable() creates
 * (NewtonIterationUtilities.cpp:98-115).  Call before the first assemble of a report step. */
int opmgpu_set_wells(opmgpu_ctx* ctx, int nw, const int32_t* well_connpos /*nw+1*/,
                     const int32_t* well_cells /*nperf*/);

/* ReservoirState in/out (BlackoilState.hpp:40-90): pressure[nc], saturation[nc*3]
 * cell-major interleaved (w,o,g), gasoilratio[nc], rv[nc], hydroCarbonState[nc]. */
int opmgpu_set_state(opmgpu_ctx* ctx, const double* p, const double* sat, const double* rs,
                     const double* rv, const int8_t* hcstate);
int opmgpu_get_state(opmgpu_ctx* ctx, double* p, double* sat, double* rs, double* rv,
                     int8_t* hcstate);

/* BlackoilModelBase::assemble (BlackoilModelBase_impl.hpp:757-840) minus the host well model:
 * variableState -> [initial: computeAccum(state0,0)] -> assembleMassBalanceEq.
 * State pointers may all be NULL to use the device-resident state.  `initial` is the
 * reference's initial_assembly flag (iteration == 0): accum0 is (re)computed, which is what
 * makes re-entry with a rolled-back state and a chopped dt safe. */
int opmgpu_assemble(opmgpu_ctx* ctx, double dt, int initial, const double* p, const double* sat,
                    const double* rs, const double* rv, const int8_t* hcstate);

/* Per-perforation cell quantities the host StandardWells model needs
 * (extractWellPerfProperties, StandardWells_impl.hpp:396-571).  out is [nperf][OPMGPU_PERF_K]:
 * for q in {p_o, rs, rv, b_w, b_o, b_g, mob_w, mob_o, mob_g}: value, d/dP, d/dSw, d/dXvar. */
#define OPMGPU_PERF_K 36
int opmgpu_perf_props(opmgpu_ctx* ctx, double* out);

/* addWellContributionToMassBalanceEq (BlackoilModelBase_impl.hpp:953-975) + the Schur
 * complement of eliminateVariable (NewtonIterationUtilities.cpp:45-128), computed on the host:
 * resid_delta[nperf*3] is ADDED to the (unscaled) residual of the perforated cells (phase
 * fastest), schur blocks (UNSCALED, row-major 3x3, d eq / d var) are ADDED to J at
 * (schur_rc[2k], schur_rc[2k+1]) in caller cell numbering; the library applies matbalscale. */
int opmgpu_add_well_terms(opmgpu_ctx* ctx, const double* resid_delta, int nblk,
                          const int32_t* schur_rc, const double* schur_blocks);

/* Right-hand-side part of the Schur elimination: -B D^-1 r_well per perforation (UNSCALED, phase fastest).  Unlike
 * resid_delta above it must NOT enter the convergence check (the reference eliminates on a copy inside the linear
 * solver, NewtonIterationBlackoilInterleaved.cpp:221-231), so it is kept apart and only added when the RHS is built.
 * Cleared by every opmgpu_assemble. */
int opmgpu_add_well_rhs(opmgpu_ctx* ctx, const double* rhs_delta /*nperf*3*/);
/* Newton increment of the perforated cells after opmgpu_solve (for recoverVariable, NewtonIterationUtilities.cpp:134-184):
 * out[nperf*3] = dP, dSw, dXvar per perforation. */
int opmgpu_perf_dx(opmgpu_ctx* ctx, double* out);

/* Precision of the coming opmgpu_solve, known before the assembly like the reference's residual_.singlePrecision = dt <
 * maxSinglePrecisionTimeStep (BlackoilModelBase_impl.hpp:284).  With single_precision != 0 the next opmgpu_assemble writes
 * the Jacobian as float directly (no f64 copy, no conversion pass; opmgpu_get_jacobian_bsr then returns the float values
 * widened, and a double solve after such an assembly works on the widened values).  Default 0 = double. */
int opmgpu_set_solve_precision(opmgpu_ctx* ctx, int single_precision);

/* getConvergence / convergenceReduction (BlackoilModelBase_impl.hpp:1633-1857) for the reservoir
 * equations: B_avg, CNV, MB per phase plus the L-inf residual norms of computeResidualNorms
 * (:1551-1589).  *converged = all MB < tol_mb && all CNV < tol_cnv.  Returns OPMGPU_ENUMERICAL
 * on NaN or > max_residual_allowed exactly where the reference throws NumericalIssue. */
int opmgpu_convergence(opmgpu_ctx* ctx, double dt, double* B_avg3, double* CNV3, double* MB3,
                       double* linf3, int* converged);

/* solveJacobianSystem -> NewtonIterationBlackoilInterleaved::computeNewtonIncrement
 * (NewtonIterationBlackoilInterleaved.cpp:202-292, :467-487) on the assembled, matbal-scaled
 * device system: block-ILU0 + BiCGStab in float if single_precision (the reference's
 * dt < 20 d switch, :478-480), else double.  dx (3*nc, equation-major, caller cell order) may be
 * NULL to keep the increment resident for opmgpu_update_state. */
int opmgpu_solve(opmgpu_ctx* ctx, int single_precision, double* dx, int* iters, double* reduction);

/* updateState (BlackoilModelBase_impl.hpp:1147-1389): dp/ds chopping, saturation
 * renormalisation, rs/rv limits, phase-state switching.  dx NULL = use the resident increment
 * of the last opmgpu_solve.  relax multiplies dx first (NonlinearSolver_impl.hpp:283-301, dampen). */
int opmgpu_update_state(opmgpu_ctx* ctx, const double* dx, double relax);

/* ------------------------------------------------------------------------------------------
 * Wells on the device: the standard well model of StandardWells_impl.hpp:396-998 evaluated per well on
 * the GPU, the well unknowns (q_s[3], bhp) Schur-eliminated like NewtonIterationUtilities.cpp:45-128 -- but kept in
 * factored form (diagonal-block updates + a rank-7 operator per well applied inside the SpMV) instead of filling the
 * matrix with a clique per well.  Alternative to the host-well path (opmgpu_set_wells / perf_props / add_well_terms):
 * after opmgpu_set_device_wells, opmgpu_assemble adds the well terms itself, opmgpu_solve uses the coupled operator,
 * opmgpu_update_state also recovers and updates the well unknowns (updateWellState, :611-650), and
 * opmgpu_save_state / restore_state carry the well state along.  Fields mirror opm-core's `Wells` struct.
 * Shared cells: any number of DIFFERENT wells may perforate one cell (a water and a gas injector of a WAG pair at the same I, J, K, a
 * producer and its sidetrack, two deviated wells crossing), as in the reference, whose StandardWells works on perforation-to-cell
 * operators.  One well naming the same cell twice is OPMGPU_EINVAL.  The wells' contributions to such a cell's row -- residual, diagonal
 * block, right-hand-side term of the eliminated well equations, the coupled operator's P t terms, the pressure stage's border columns
 * -- are summed in ascending perforation index, the order of well_cells: a fixed order, so every result is the same bits from run to
 * run.  Refused with shared cells (OPMGPU_EINVAL, text in opmgpu_last_error): a decomposed context (a communicator is attached, whichever
 * call comes first) and the subdomain coarse space (OPMGPU_COARSE=2, OPMGPU_EMULATE_RANKS > 1); OPMGPU_WELL_WOODBURY=1 is switched off
 * for such a well list, with one line on stderr.
 * ---------------------------------------------------------------------------------------- */
typedef struct opmgpu_wells {
    int32_t        nw;
    const int32_t* well_connpos;   /* [nw+1]                                                   */
    const int32_t* well_cells;     /* [nperf] (wells may share a cell; no cell twice in ONE well) */
    const double*  WI;             /* [nperf] well index (connection transmissibility factor)  */
    const int32_t* type;           /* [nw] 0 = INJECTOR, 1 = PRODUCER                          */
    const int32_t* allow_cf;       /* [nw] allow cross flow; NULL = all 1                      */
    const double*  depth_ref;      /* [nw] bhp reference depth                                 */
    const double*  comp_frac;      /* [nw*3] injection stream composition (w, o, g)            */
    const int32_t* ctrl_type;      /* [nctrl] OPMGPU_CTRL_*                                    */
    const double*  ctrl_target;    /* [nctrl]                                                  */
    const double*  ctrl_distr;     /* [nctrl*3] rate-control phase weights; NULL = 0           */
    /* WellControls with several controls per well (opm-core well_controls.h): control ctrl_ptr[w] is the well's initial
     * CURRENT control (an equation), the others are inequality constraints that updateWellControls switches to when broken
     * (StandardWells_impl.hpp:709-800).  ctrl_ptr == NULL: one control per well (nctrl == nw).                           */
    const int32_t* ctrl_ptr;       /* [nw+1] or NULL                                           */
    const int32_t* ctrl_vfp;       /* [nctrl] VFP table id of the THP controls, or NULL        */
    const double*  ctrl_alq;       /* [nctrl] artificial lift quantity of THP controls, or NULL */
} opmgpu_wells;
enum { OPMGPU_CTRL_BHP = 0, OPMGPU_CTRL_SURFACE_RATE = 1, OPMGPU_CTRL_THP = 2, OPMGPU_CTRL_RESERVOIR_RATE = 3 };

/* VFP tables for THP control (VFPProdPropertiesLegacy.cpp:36-154, VFPInjPropertiesLegacy.cpp:36-130; opm-common's VFPProdTable /
 * VFPInjTable).  SI units.  Producer data is [nthp][nwfr][ngfr][nalq][nflo], injector data [nthp][nflo] (the other axes have
 * length 1 and may be NULL).  Multilinear interpolation, linear extrapolation outside the axes. */
enum { OPMGPU_VFP_FLO_OIL = 0, OPMGPU_VFP_FLO_LIQ = 1, OPMGPU_VFP_FLO_GAS = 2 };
enum { OPMGPU_VFP_WFR_WOR = 0, OPMGPU_VFP_WFR_WCT = 1, OPMGPU_VFP_WFR_WGR = 2 };
enum { OPMGPU_VFP_GFR_GOR = 0, OPMGPU_VFP_GFR_GLR = 1, OPMGPU_VFP_GFR_OGR = 2 };
typedef struct opmgpu_vfp_table {
    int32_t id, is_injector;
    int32_t flo_type, wfr_type, gfr_type;
    double  datum_depth;
    int32_t nflo, nthp, nwfr, ngfr, nalq;
    const double *flo, *thp, *wfr, *gfr, *alq;
    const double* data;
} opmgpu_vfp_table;

/* Call BEFORE opmgpu_set_device_wells when a well has a THP control; n == 0 removes the tables. */
int opmgpu_set_vfp_tables(opmgpu_ctx* ctx, int n, const opmgpu_vfp_table* tables);
/* diagnostic: the device's VFP evaluators (csrc/vfp.hpp, what the well kernels call) at n points on table number `table` -- its index in the
 * last opmgpu_set_vfp_tables call, so a producer and an injector table with the same id stay apart.  Per point i: rates q[3i..3i+2] = (aqua,
 * liquid, vapour) with the well's signs (a producer's are negative), thp[i], alq[i] -> bhp_out[i] and dbhp_dq[3i..3i+2] = d bhp / d q
 * (VFPProd/InjPropertiesLegacy::bhp); bhp_in[i] -> thp_out[i] (::thp, the inversion along the THP axis at the same rates and alq).  No
 * hydrostatic correction.  It changes nothing a later solve sees; OPMGPU_EINVAL without tables or for an unknown table.
 * tests/test_gpu_vfp.py compares it with the host restatement opmgpu/vfp.py. */
int opmgpu_vfp_evaluate(opmgpu_ctx* ctx, int table, int n, const double* q, const double* thp, const double* alq, const double* bhp_in,
                        double* bhp_out, double* dbhp_dq, double* thp_out);
/* nw == 0 removes them.  Multi-GPU: a well lives on ONE rank, and EVERY rank of a run with wells makes this call (nw = 0 where it owns
 * none) -- opmgpu_well_convergence is collective, and the call tells the pressure stage's coarse space that the run has wells. */
int opmgpu_set_device_wells(opmgpu_ctx* ctx, const opmgpu_wells* wells);
/* Well efficiency factors (WEFAC): factors[nw] in the order of opmgpu_set_device_wells, each in (0, 1]; NULL = all ones.  The reference
 * builds one value per perforation from the well's factor (StandardWells_impl.hpp:1405-1434) and subtracts efficiency_factors * cq_s from
 * the mass balance of the perforated cells (addWellContributionToMassBalanceEq, BlackoilModelBase_impl.hpp:953-975).  The rule: for every
 * perforation j of well w, R_a[cell_j] -= e_w cq_s[a][j] with every derivative of that term -- the own-cell block -e_w d cq_s / d cell and
 * the reservoir-row, well-column coupling e_w B_j.  The WELL equations do not see e_w: flux and control equation, D, C, D^-1, wellbore
 * mixture, cross-flow rules, connection pressures, perfPhaseRates, wellRates, bhp, thp, the pre-solve and opmgpu_well_convergence are
 * what they are without it.  With every factor 1 the assembly gives bit for bit what it gives without the call.
 * Call AFTER opmgpu_set_device_wells; a later opmgpu_set_device_wells resets the factors to ones (the well list changed).  The factors are
 * no part of the saved state: they last through opmgpu_save_state / opmgpu_restore_state, a change of the solve's precision and a
 * re-plan.  Multi-GPU: rank-local (the factors of this rank's wells), no communication.
 * OPMGPU_EINVAL with text in opmgpu_last_error(ctx): no device wells are set; a factor is not finite; a factor is outside (0, 1]. */
int opmgpu_set_well_efficiency(opmgpu_ctx* ctx, const double* factors);
/* Group rate control (GCONPROD, GCONINJE) shared by guide rates.  The reference calls the group logic from its Newton loop
 * (setupGroupControl at the first assembly of a time step, updateWellTargets behind updateWellControls at every assembly and inside the
 * well pre-solve: BlackoilModelBase_impl.hpp:779-792, :1090-1093) but WellCollection / WellsGroup themselves are opm-core's and not part
 * of the reference tree.  The sharing rule below is therefore OURS: stated here, pinned by a numpy restatement
 * (tests/group_reference.py), and unpinned against opm-core.
 * A controlled group g has a sign s_g (-1 production, +1 injection), a target T_g >= 0 (surface volume rate, SI), phase weights d_g[3]
 * in water, oil, gas order (ORAT {0,1,0}, WRAT {1,0,0}, GRAT {0,0,1}, LRAT {1,1,0}; an injection group: the unit vector of its phase) and
 * member wells M_g, each with a guide rate gamma_w > 0.  A well belongs to at most one controlled group.  Every member carries one GROUP
 * SLOT: a SURFACE_RATE control with distr d_g that is the LAST control of the well (so updateWellControls, which switches to the first
 * broken constraint, gives it the lowest priority); s_w is its index within the well.  With r_w = e_w (d_g . qs_w) (e_w: the well's
 * efficiency factor), I = {w in M_g : current[w] != s_w} (individual control) and C = M_g \ I (group control), the slot targets are a pure
 * function of (current, qs, gamma, e, T):
 *     w in C:  Gamma   = sum_{v in C} gamma_v,             rem   = max(0, T_g - s_g sum_{v in I} r_v),           target_w = s_g (gamma_w / Gamma)   rem   / e_w
 *     w in I:  Gamma_w = gamma_w + sum_{v in C} gamma_v,   rem_w = max(0, T_g - s_g sum_{v in I, v != w} r_v),   target_w = s_g (gamma_w / Gamma_w) rem_w / e_w
 * (for a well in I: what it would get if it joined).  The rule is stateless: a well that left group control has a defined way back.
 * Nothing else of a well's controls changes.  The device re-shares (k_group_targets) before and after updateWellControls at every
 * assembly, behind the control update of every iteration of the well pre-solve, which takes its unfused path while groups are set, and
 * behind the restore of the well state after a pre-solve that did not converge.
 * Sums run per group in a fixed order without floating-point atomics: the same input gives the same bits in every run.
 * opmgpu_set_well_groups: members of group g = group_wells[group_ptr[g] .. group_ptr[g+1]) (well indices of opmgpu_set_device_wells),
 * guide[] in the same positions, sign[ngroups], target[ngroups], distr[ngroups*3].  Call AFTER opmgpu_set_device_wells; ngroups == 0
 * removes the groups and puts the slots' targets back to what the caller gave them.  A later opmgpu_set_device_wells removes the groups
 * (the well list changed); they are no part of the saved state and last through opmgpu_save_state / opmgpu_restore_state, a change of
 * the solve's precision and a re-plan.  With no groups set nothing is launched and every path gives the bits it gave before.
 * OPMGPU_EINVAL with text in opmgpu_last_error(ctx), and the groups in force stay: no device wells are set; a communicator is attached
 * (a group's wells may sit on several ranks: out of scope); a well is in two groups; a member's last control is not a SURFACE_RATE slot
 * with the group's distr; a guide rate is not finite or not positive; a target is not finite or negative.
 * opmgpu_get_well_group_targets: runs the rule on the well state and current controls as they stand and returns slot_target[nw] (NaN for
 * a well in no group) and group_rate[ngroups] = sum_{w in M_g} r_w (signed as the wells' rates are); either pointer may be NULL. */
int opmgpu_set_well_groups(opmgpu_ctx* ctx, int ngroups, const int32_t* group_ptr, const int32_t* group_wells, const double* sign,
                           const double* target, const double* distr, const double* guide);
int opmgpu_get_well_group_targets(opmgpu_ctx* ctx, double* slot_target, double* group_rate);
/* Cells perforated by more than one well (computeWellFlux, StandardWells_impl.hpp:396-560, and addWellContributionToMassBalanceEq,
 * BlackoilModelBase_impl.hpp:953-975, which superpose any number of perforations on a cell): *shared_rows = number of such cells,
 * *max_wells_per_cell = the most wells found in one cell; both 0 for a well list without shared cells.  Either pointer may be NULL.
 * OPMGPU_EINVAL without device wells. */
int opmgpu_well_shared_cells(opmgpu_ctx* ctx, int32_t* shared_rows, int32_t* max_wells_per_cell);
/* the factors in force (factors[nw]); OPMGPU_EINVAL without device wells */
int opmgpu_get_well_efficiency(opmgpu_ctx* ctx, double* factors);
/* WellStateFullyImplicitBlackoil fields: bhp[nw], wellRates qs[nw*3]; perfPress perf_press[nperf] and perfPhaseRates
 * perf_rates[nperf*3] may be NULL (keep).  perf_press feeds the average well-block pressures of computeWellConnectionPressures. */
int opmgpu_well_state_set(opmgpu_ctx* ctx, const double* bhp, const double* qs, const double* perf_press, const double* perf_rates);
int opmgpu_well_state_get(opmgpu_ctx* ctx, double* bhp, double* qs, double* perf_press, double* perf_rates);
/* currentControls() (index into each well's controls, relative to ctrl_ptr[w]) and thp() of the well state; any pointer may be NULL.
 * get also reports the iteration count and outcome of the last explicit well pre-solve (solveWellEq). */
int opmgpu_well_controls_set(opmgpu_ctx* ctx, const int32_t* current, const double* thp);
int opmgpu_well_controls_get(opmgpu_ctx* ctx, int32_t* current, double* thp, int32_t* presolve_iterations, int32_t* presolve_converged);
/* well_controls_iset_target / well_controls_iset_distr for ALL controls (order of opmgpu_set_device_wells; either pointer may be NULL = keep):
 * what SimulatorBase::computeRESV does to the RESERVOIR_RATE controls once per report step (SimulatorBase_impl.hpp:551-553). */
int opmgpu_well_controls_set_targets(opmgpu_ctx* ctx, const double* ctrl_target, const double* ctrl_distr);
/* computePropertiesForWellConnectionPressures (StandardWells_impl.hpp:218-296) for the HOST well model: b_w, b_o, b_g, rsSat, rvSat
 * of the perforated cells (opmgpu_set_wells order) evaluated at the given pressures with the cells' own rs / rv / phase condition /
 * oil saturation.  out[nperf*5]. */
int opmgpu_perf_pvt(opmgpu_ctx* ctx, const double* pressure, double* out);
/* B_avg of getWellConvergence (BlackoilModelBase_impl.hpp:1876-1891) for the host well model's pre-solve: mean 1/b per phase of the
 * last assembly. */
int opmgpu_average_b(opmgpu_ctx* ctx, double* B_avg3);
/* well part of getConvergence (BlackoilModelBase_impl.hpp:1769-1779) after opmgpu_assemble: max |flux equation| per
 * phase (to be multiplied by B_avg and compared with tolerance_wells) and max |control equation|. */
int opmgpu_well_convergence(opmgpu_ctx* ctx, double* flux_residual3, double* control_residual);

/* Device-side last_state of AdaptiveTimeStepping (AdaptiveTimeStepping_impl.hpp:211-212, :318-319, :346-347): save = copy
 * the resident reservoir state aside, restore = copy it back after a failed sub-step (the state never leaves the device),
 * relative_change = BlackoilModelBase::relativeChange(previous = saved, current = resident)
 * (BlackoilModelBase_impl.hpp:1595-1631): (|p0-p|^2 + |s0-s|^2) / (|p|^2 + |s|^2), what the PID controllers consume. */
int opmgpu_save_state(opmgpu_ctx* ctx);
int opmgpu_restore_state(opmgpu_ctx* ctx);
int opmgpu_relative_change(opmgpu_ctx* ctx, double* value);

/* RateConverter::SurfaceToReservoirVoidage (RateConverterLegacy.hpp:407-770), the two halves SimulatorBase::computeRESV
 * (SimulatorBase_impl.hpp:476-553) and computeWellVoidageRates (BlackoilModelBase_impl.hpp:2490-2534) call:
 * defineState -> calcAverages (:718-768): per region the SUMS of p, rs, rv of the RESIDENT state over the cells and their number,
 *   sums[nregions][4]; region[nc] in the caller's cell order with values 0 .. nregions-1, NULL = one region of all cells (what
 *   SimulatorBase builds, SimulatorBase_impl.hpp:66).  Collective in decomposed runs (owned cells, summed over the ranks: the is_parallel
 *   branch).  The division -- and the reference's habit of NOT clearing rs / rv between calls (:733-737) -- stay with the caller's mirror.
 * calcCoeff (:495-548): coeff[n][3] (water, oil, gas) with q_rT = sum_p coeff[p] q_s[p] at n given (p, rs, rv) points; pvt_region NULL = 0. */
int opmgpu_region_state_sums(opmgpu_ctx* ctx, const int32_t* region, int nregions, double* sums);
int opmgpu_voidage_coefficients(opmgpu_ctx* ctx, int n, const double* p, const double* rs, const double* rv, const int32_t* pvt_region, double* coeff);

/* BlackoilModelBase::computeFluidInPlace (BlackoilModelBase_impl.hpp:2263-2445; called by SimulatorBase_impl.hpp:207, :278 and
 * AdaptiveTimeStepping_impl.hpp:322) for the RESIDENT state: per cell fip[phase] = pv_mult * b_phase * s_phase * pv (b at the phase
 * pressures and the cell's phase condition), dissolved gas rs * fip[oil], vaporised oil rv * fip[gas], summed per region together with
 * the pore volume and the hydrocarbon-pore-volume weighted average pressure.
 *   fipnum    [nc] region of every cell in the caller's cell order, 1-based, 0 = in no region (the reference's fipnum[c] - 1 == -1);
 *             NULL = one region of all cells
 *   values    [nregions][7]: water, oil, gas, dissolved gas, vaporised oil, pore volume, weighted pressure (SimulatorData::FipId,
 *             BlackoilModelEnums.hpp:53-61)
 *   fip_cells [7][nc] or NULL: the per-cell arrays of SimulatorData::fip (getFIPData()), caller's cell order
 * The per-cell evaluation runs on the device, the region loops on the host in the reference's cell order.  Decomposed runs (the
 * reference's parallel branch, :2369-2446): a COLLECTIVE call; every rank passes the fipnum of its local cells (ghost cells included --
 * only owned cells are counted) and the GLOBAL number of regions, the sums are taken over the owned cells and all-reduced, every rank
 * receives the global values (fip_cells: this rank's cells, zeros in the pv / weighted-pressure rows of its ghosts). */
int opmgpu_compute_fluid_in_place(opmgpu_ctx* ctx, const int32_t* fipnum, int nregions, double* fip_cells, double* values);

/* BlackoilModelBase's SimulatorData (BlackoilModelBase_impl.hpp:662-683, rq_[].b/rho/mu/kr; turned into named restart arrays by
 * SimulatorFullyImplicitBlackoilOutput.hpp:512-567 and written per RPTRST mnemonic by getRestartData, :585-845) of the RESIDENT state,
 * evaluated as the assembly evaluates it (end-point and vertical scaling, hysteresis, VAPPARS, ROCKTAB).  out is [OPMGPU_SIMDATA_K][nc],
 * SI units, the same cells in the same order as opmgpu_get_state (decomposed runs: the rank's local cells; no communication):
 *   b, rho, mu of water / oil / gas   rq_[phase].b / .rho (fluidDensity, :2009-2027) / .mu
 *   kr                                rq_[phase].kr: the relative permeability itself, no transmissibility multiplier, not over mu
 *   RSSAT, RVSAT                      sd_.rsSat = fluidRsSat(p_o, so), sd_.rvSat = fluidRvSat(p_g, so) (:662, :668): the saturated
 *                                     ratios, VAPPARS factor included, of EVERY cell whatever its phase state; 0 without DISGAS / VAPOIL
 *   PBUB, PDEW                        bubblePointPressure(rs), dewPointPressure(rv) of the solution state's rs / rv (:678-683,
 *                                     BlackoilPropsAdFromDeck.cpp:959-1004).  The inversion itself is opm-material's; OUR rule: the
 *                                     pressure at which the PVT region's plain tabulated saturated curve (piecewise linear, end segments
 *                                     extrapolated, no VAPPARS factor) takes the value, first matching segment from the lowest pressure
 *                                     upwards; 0 when no segment contains it, the segment is flat or the result is not finite, and 0
 *                                     everywhere without DISGAS (PBUB) / VAPOIL (PDEW).
 * One launch and one device-to-host copy on the context's stream; nothing an assembly relies on is touched.  OPMGPU_EINVAL for a NULL
 * pointer or before a state has been set. */
#define OPMGPU_SIMDATA_K 16
enum {
    OPMGPU_SD_BW = 0, OPMGPU_SD_BO, OPMGPU_SD_BG,                       /* "1OVERBW", "1OVERBO", "1OVERBG" */
    OPMGPU_SD_WAT_DEN, OPMGPU_SD_OIL_DEN, OPMGPU_SD_GAS_DEN,            /* "WAT_DEN", "OIL_DEN", "GAS_DEN" */
    OPMGPU_SD_WAT_VISC, OPMGPU_SD_OIL_VISC, OPMGPU_SD_GAS_VISC,         /* "WAT_VISC", "OIL_VISC", "GAS_VISC" */
    OPMGPU_SD_WATKR, OPMGPU_SD_OILKR, OPMGPU_SD_GASKR,                  /* "WATKR", "OILKR", "GASKR" */
    OPMGPU_SD_RSSAT, OPMGPU_SD_RVSAT, OPMGPU_SD_PBUB, OPMGPU_SD_PDEW    /* "RSSAT", "RVSAT", "PBUB", "PDEW" */
};
int opmgpu_get_simulator_data(opmgpu_ctx* ctx, double* out /* [OPMGPU_SIMDATA_K * nc] */);

/* BlackoilModelBase::setThresholdPressures (BlackoilModelBase_impl.hpp:421-443; called from SimulatorBase_impl.hpp:467-468 once the
 * initial state exists, because a defaulted THPRES value is computed from it): replaces the threshold pressures of ALL connections, in
 * the connection order of opmgpu_grid.conn_cells (grid faces, then NNCs); NULL removes them.  Works on a context created with or without
 * opmgpu_grid.thpres and lasts through later opmgpu_set_wells / opmgpu_set_device_wells calls.  The assembly applies them as before
 * (applyThresholdPressures, :1518-1545); no kernel of the Newton path changes.  A negative or non-finite value: OPMGPU_EINVAL, text in
 * opmgpu_last_error(ctx), nothing changed.  Decomposed runs: the rank's local connections, no communication. */
int opmgpu_set_threshold_pressures(opmgpu_ctx* ctx, const double* thpres /* [nconn] or NULL */);

/* PVCDO: the dead oil of constant compressibility and viscosibility.  The reference takes the keyword through opm-material's
 * ConstantCompressibilityOilPvt (FluidSystem::initFromDeck, BlackoilPropsAdFromDeck.cpp:164), which is outside its tree, so THE RULE
 * BELOW IS OURS and is pinned against opm-material by nothing.  It is the arithmetic of PVTW (ConstantCompressibilityWaterPvt) with oil's
 * row at the oil pressure.  Per PVT region one row (p_ref [Pa], B_ref, C_o [1/Pa], mu_ref [Pa s], C_v [1/Pa]):
 *   X = C_o (p - p_ref)            1 / B_o        = (1 + X (1 + X / 2)) / B_ref
 *   Y = (C_o - C_v) (p - p_ref)    1 / (B_o mu_o) = (1 + Y (1 + Y / 2)) / (B_ref mu_ref)
 * with analytic derivatives with respect to p and no dependence on Sw, rs or rv.  The oil is dead: RSSAT and PBUB of the output record
 * are 0.  The tables a context is created with cannot express this (they are piecewise linear in 1 / B and 1 / (B mu)); the context is
 * created with any valid dead-oil table in their place, and from this call on every evaluator of the oil -- the assembly, the perforation
 * properties and PVT, the voidage coefficients, the fluid in place, the output record, computeMaxDp -- takes the form above instead of
 * that table.  NULL goes back to the tabulated oil.  To be called before an assembly; it lasts through opmgpu_set_wells /
 * opmgpu_set_device_wells, opmgpu_save_state / opmgpu_restore_state and a change of the solve's precision, and a context re-planned
 * after the call assembles bit for bit what one re-planned before it does.  has_vapoil (wet gas over dead oil) is allowed.
 * OPMGPU_EINVAL with text in opmgpu_last_error(ctx), nothing changed: a context with has_disgas != 0, a non-finite entry, B_ref <= 0 or
 * mu_ref <= 0.  Decomposed runs: every rank sets its own copy; no communication. */
int opmgpu_set_pvcdo(opmgpu_ctx* ctx, const double* pvcdo /* [n_pvt_regions][5], SI; NULL = back to the tabulated oil */);

/* computeMaxDp (opm/simulators/thresholdPressures.hpp:46-298; called at FlowMain.hpp:675-680) for the RESIDENT state: the largest
 * phase-potential difference across every pair of equilibration regions, which a defaulted THPRES item takes as its value
 * (thresholdPressures / thresholdPressuresNNC, ibid. :320-369, :383-417).
 *   eqlnum      [nc] equilibration region of every cell, 1-based, caller's cell order
 *   n_face_conn the first n_face_conn connections are grid faces and are scanned; the NNCs behind them are not (the reference loops over
 *               the grid's faces only)
 *   dp_conn     [nconn] or NULL: per connection the largest |p1 - p2| over the phases that count; 0 when none counts, when both cells lie
 *               in one region and for f >= n_face_conn
 *   max_dp      [nregions][nregions], symmetric: the maximum of dp_conn over the face connections joining regions a and b; -1.0 where no
 *               face connection joins them (the reference's "pair absent from the map"); 0.0 for a joined pair whose phases never count
 * Per cell and phase (:109-248), by rules that are NOT the Newton path's: p_o = the state's pressure, p_w = p_o - pcow(Sw),
 * p_g = p_o + pcgo(Sg) at the state's saturations with the cell's end-point and vertical scaling; rho_w = rhoS_w b_w(p_w);
 * rho_o = (rhoS_o + rhoS_g Rs) b_o with the state's Rs and b_o from the saturated curve at p_o when Rs >= RsSat(p_o), else undersaturated
 * at (p_o, Rs); rho_g = (rhoS_g + rhoS_o Rv) b_g likewise by Rv >= RvSat(p_g) at p_g.  RsSat / RvSat carry no VAPPARS factor, the phase
 * condition of the state is not consulted.  Per face and active phase (:278-296): p1 = p(c1), p2 = p(c2) + (rho(c1) + rho(c2))/2 g
 * (z1 - z2); the phase counts when (p1 > p2 && s1 > sres1) || (p2 > p1 && s2 > sres2), strict, with the residual saturations of satRange
 * (SaturationPropsFromDeck.cpp:212-250): water the cell's scaled SWL else the first Sw node of its table, gas SGL likewise, oil
 * max(0, 1 - SWU - SGU).  OPMGPU_PHASES_OIL_WATER: water and oil only, oil residual max(0, 1 - SWU); no gas table is read.
 * The per-face evaluation runs on the device, the maxima per pair on the host over the downloaded plane.  Decomposed runs: a COLLECTIVE
 * call; every rank passes its local cells' eqlnum, its local n_face_conn and the GLOBAL number of regions, and receives the maxima over
 * all ranks (a connection two ranks both hold is harmless to a maximum); dp_conn stays local.
 * OPMGPU_EINVAL (with text) for a NULL eqlnum / max_dp, a region outside [1, nregions], n_face_conn outside [0, nconn], or no state. */
int opmgpu_compute_max_dp(opmgpu_ctx* ctx, const int32_t* eqlnum, int nregions, int n_face_conn, double* dp_conn, double* max_dp);

/* SWATINIT: BlackoilPropsAdFromDeck::setSwatInitScaling (BlackoilPropsAdFromDeck.cpp:1009-1019; called at FlowMain.hpp:683-690 "to match
 * the scaled capillary pressure in props").  Rescales every cell's maximum oil-water capillary pressure (PCW) so that the imposed water
 * saturation sw[c] is in equilibrium with the target pcow[c] = p_o - p_w.  The reference hands each cell to
 * EclMaterialLawManager::applySwatinit, which is opm-material and outside its tree, so THE RULE BELOW IS OURS.  It is pinned by the known
 * answers of the reference's DeckWithSwatinit test (tests/test_equil_legacy.cpp:916-1060: 60 saturations, 12 scaled capillary pressures),
 * which it reproduces, and by nothing else.  For cell c with its drainage scaled end points Swl, Swu (the cell's SWL / SWU, else the first /
 * last Sw node of its SWOF table):
 *   pcow[c] < 0:  sw_out = Swu, PCW unchanged;
 *   else          Sw = min(max(sw[c], Swl), Swu), sw_out = Sw (a saturation clamped to Swl is still scaled);
 *                 pc_at = the cell's oil-water capillary pressure at Sw under its CURRENT end-point and vertical scaling;
 *                 pc_at > 0: PCW_c *= pcow[c] / pc_at;  pc_at <= 0 (a table without capillary pressure, or a zero at Sw): unchanged.
 * Applying it again with pcow equal to the scaled curve at sw_out changes nothing (the ratio is 1); calling it twice with the same target
 * compounds, as the reference's would.  No cap on the scaled PCW (PPCWMAX), no mixed-wettability handling.
 * pc_at is evaluated on the device by the evaluators of the Newton path (one kernel, one thread per cell); the new PCW is kept on the
 * host as a pressure and reaches the device as opmgpu_grid.eps_v[3] does at creation.  So a context scaled here, a context created with
 * eps_v[3] = the array opmgpu_get_pcw returns, and either after opmgpu_set_wells / opmgpu_set_device_wells assemble bit for bit the same.
 * Works on a context created with or without end points / vertical arrays, with every three-phase model and without a gas phase; the
 * imbibition curves of a hysteresis context carry no capillary pressure and are untouched.  sw_out may be NULL.
 * OPMGPU_EINVAL with text in opmgpu_last_error(ctx), nothing changed: a non-finite sw or pcow, sw outside [0, 1], a NULL sw / pcow.
 * Decomposed runs: the rank's local cells, ghosts included (a ghost's PCW enters the owner's flux); no communication. */
int opmgpu_set_swatinit_scaling(opmgpu_ctx* ctx, const double* sw /* [nc] */, const double* pcow /* [nc] */, double* sw_out /* [nc] or NULL */);

/* Each cell's current maximum oil-water capillary pressure [Pa]: its PCW (opmgpu_grid.eps_v[3], or what opmgpu_set_swatinit_scaling left);
 * for a context without vertical scaling of that curve -- and for a cell whose table's first pcow node is zero, which is never scaled --
 * the first pcow node of the SWOF table of the cell's saturation region. */
int opmgpu_get_pcw(opmgpu_ctx* ctx, double* pcw /* [nc] */);

/* BlackoilPropsAdFromDeck::capPress: pc[c] = pcow = p_o - p_w and pc[nc + c] = pcgo = p_g - p_o of every cell at the saturations sat
 * ([nc][3] water, oil, gas) or, sat == NULL, at the resident state's, through the cell's end-point and vertical scaling -- the curves the
 * assembly evaluates.  OPMGPU_PHASES_OIL_WATER: pcgo = 0.  One kernel; the resident state is only read.  OPMGPU_EINVAL (with text) for a
 * NULL pc, or a NULL sat before a state has been set. */
int opmgpu_cap_press(opmgpu_ctx* ctx, const double* sat /* [nc*3] or NULL */, double* pc /* [2*nc] */);

/* Maximum historical oil saturation per cell (BlackoilPropsAdFromDeck::satOilMax_, used by VAPPARS).
 * set: explicit values (nc, caller order; restart).  update: soMax = max(soMax, so of the resident state) --
 * what SimulatorBase_impl.hpp:192 does at the start of every report step (updateSatOilMax, :933-945).
 * Starts at zero like the reference's (BlackoilPropsAdFromDeck.cpp:175). */
int opmgpu_set_sat_oil_max(opmgpu_ctx* ctx, const double* so_max);
int opmgpu_update_sat_oil_max(opmgpu_ctx* ctx);
int opmgpu_get_sat_oil_max(opmgpu_ctx* ctx, double* so_max);

/* DRSDT / DRVDT: limits on how fast the dissolved-gas ratio Rs and the vaporised-oil ratio Rv of a cell may RISE within a time step.
 * The reference has neither keyword (VAPPARS is its only brake), so THE RULE IS OURS; it is stated here, restated independently under
 * tests/ and pinned to no other simulator.
 *
 * Per context: a rate a_s >= 0 [1/s] for Rs with the flag free_only, and a rate a_v >= 0 [1/s] for Rv; each may be off.  With a limit on,
 * the context carries two per-cell planes rs_cap[nc], rv_cap[nc]; +inf means no cap.
 *
 * Begin of a time step of length dt (opmgpu_begin_dissolution_step, after any state upload and again whenever a failed sub-step has
 * restored the saved state and a shorter dt is tried): the host forms d_s = a_s * dt and d_v = a_v * dt once, in float64; one kernel
 * writes per cell rs_cap[c] = rs[c] + d_s and rv_cap[c] = rv[c] + d_v from the RESIDENT state (one addition, one rounding, no FMA: a
 * float64 restatement matches bit for bit).  With free_only, cells whose resident sg[c] == 0 get rs_cap = +inf (DRSDT's option FREE: the
 * limit acts only where free gas is present); DRVDT has no option.  A rate that is off writes +inf everywhere.
 *
 * Evaluator (every kernel that evaluates a cell: assembly, perforation properties, fluid in place, the output record; three-phase models
 * only).  After the VAPPARS factor, capped_s = rs_cap[c] < RsSat (strict: a tie is not capped).  When capped, the effective saturated
 * ratio is the CONSTANT rs_cap[c], all derivatives zero; otherwise it is RsSat as before.  rs of the cell is the primary variable in an
 * OIL_ONLY cell, else the effective saturated ratio.  The oil PVT takes its saturated branch iff !has_disgas || (free gas && !capped_s),
 * otherwise the undersaturated table at (rs, p): a capped cell with free gas holds undersaturated oil at (p, rs_cap), whose derivatives
 * with respect to the third variable vanish through the chain rule.  Rv is symmetric: capped_v = rv_cap[c] < RvSat, the gas PVT is
 * saturated iff !has_vapoil || (free oil && !capped_v), otherwise the table at (p_g, rv).  opmgpu_simulator_data reports the effective
 * values as RSSAT / RVSAT; PBUB / PDEW are unchanged.
 *
 * State update (opmgpu_update_state): the two saturated Rs values the phase switching compares against (at the old and at the new
 * pressure) each become min(value, rs_cap[c]), the two of Rv min(value, rv_cap[c]).  Nothing else in the switching logic changes.
 * That logic frees gas from an OIL_ONLY cell only when its new rs passes the saturated ratio by the factor 1 + sqrt(DBL_EPSILON) AND its
 * old rs was within that factor of it, so by itself it lets rs stand above the cap for an iteration (and within the factor for good).
 * Therefore a cell that the decision -- taken with the unlimited new value, as before -- leaves OIL_ONLY gets rs = min(new rs,
 * rs_cap[c]), and one it leaves GAS_ONLY rv = min(new rv, rv_cap[c]): after every update every cell has rs <= rs_cap, rv <= rv_cap.  The
 * next assembly evaluates the limited state, so a converged step is converged for it; where the cap does not bind nothing changes.
 *
 * Unchanged: the well-bore mixture of opmgpu_perf_pvt (average well-block pressures; the plain curves), opmgpu_compute_max_dp, the
 * voidage coefficients, the bubble- / dew-point inversion.
 *
 * set_dissolution_limits: a negative rate means off; both off removes the planes, and every kernel is again the one a context that
 * never had limits runs.  OPMGPU_EINVAL (with text, the previous limits stay in force) for: a context without a gas phase; a PVCDO context
 * (and opmgpu_set_pvcdo refuses a context with limits); drsdt on without has_disgas; drvdt on without has_vapoil; a non-finite rate; a
 * context with a communicator attached (opmgpu_comm_init* in turn refuses a context with limits: ghost cells' step-start Rs is not
 * exchanged).  begin_dissolution_step: OPMGPU_EINVAL for dt <= 0 or not finite, without limits, or before a state has been set.
 * get / set_dissolution_caps: the planes in the caller's cell order (restart; tests); either pointer may be NULL; get without limits
 * gives +inf, set without limits or with a NaN is OPMGPU_EINVAL.  Limits and caps last through opmgpu_set_wells / opmgpu_set_device_wells (a re-plan),
 * opmgpu_save_state / opmgpu_restore_state (which do not touch the caps) and a change of the solve precision. */
int opmgpu_set_dissolution_limits(opmgpu_ctx* ctx, double drsdt /* [1/s], < 0 = off */, int drsdt_free_only, double drvdt /* [1/s], < 0 = off */);
int opmgpu_begin_dissolution_step(opmgpu_ctx* ctx, double dt);
int opmgpu_get_dissolution_caps(opmgpu_ctx* ctx, double* rs_cap /* [nc] or NULL */, double* rv_cap /* [nc] or NULL */);
int opmgpu_set_dissolution_caps(opmgpu_ctx* ctx, const double* rs_cap /* [nc] or NULL */, const double* rv_cap /* [nc] or NULL */);

/* Rock regions and irreversible compaction (ROCKCOMP, ROCKNUM): a rock per cell instead of the one rock of opmgpu_tables, and pore volume
 * and transmissibility that do not come back when the pressure recovers.  The reference holds one table and has neither keyword, so THE
 * RULE IS OURS; it is stated here, restated independently under tests/ and pinned to no other simulator.
 *
 * Per context: nregions >= 1, a region r = rocknum[c] (0-based) per cell, and a mode, OPMGPU_ROCK_REVERSIBLE or OPMGPU_ROCK_IRREVERSIBLE.
 * A region has either a TABLE -- rows tab_ptr[r] .. tab_ptr[r+1] of (p, pv_mult, trans_mult), at least 2 rows, p strictly increasing --
 * or, with 0 rows, the ROCK FORM: the pair (rock_pref[r], rock_comp[r]) in the quadratic form of opmgpu_tables: pv_mult = 1 + X + X^2 / 2,
 * X = rock_comp (p - rock_pref), and transmissibility multiplier 1.  The context carries one history plane p_min[nc], which starts at +inf.
 *
 * Evaluator (every kernel that evaluates a cell, three-phase and OPMGPU_PHASES_OIL_WATER).  For a cell c in a table region:
 *   on_curve = (mode == OPMGPU_ROCK_REVERSIBLE) || (p <= p_min[c])        a tie is on the curve: a cell that goes on declining needs the slope
 *   x        = on_curve ? p : p_min[c]
 *   pv_mult  = L(pv table of r, x),  trans_mult = L(trans table of r, x)
 * where L is ROCKTAB's rule (opmgpu_tables): piecewise linear, at a breakpoint the LEFT segment, beyond both ends the end segment
 * extrapolated; y_i + slope_i (x - x_i) with slope_i = (y_(i+1) - y_i) / (x_(i+1) - x_i) formed once, in float64.  d/dp of both is
 * slope_i when on_curve, else exactly 0.0.  A ROCK-form region is always evaluated at p (elastic), whatever the mode.  Nothing else in
 * the evaluator changes: pv_mult enters every accumulation term, trans_mult multiplies the three mobilities of the cell, as the one
 * ROCKTAB of opmgpu_tables does.  While regions are set the rock fields of opmgpu_tables are not read.
 *
 * History.  opmgpu_update_rock_history: one kernel, one thread per cell, p_min[c] = fmin(p_min[c], p[c]) from the RESIDENT state (exact:
 * a float64 restatement matches bit for bit).  The caller runs it once on the initial (or restarted) state and after every converged
 * sub-step.  opmgpu_save_state / opmgpu_restore_state do not touch p_min: a failed sub-step never updated it.  Regions and p_min last
 * through opmgpu_set_wells / opmgpu_set_device_wells (a re-plan), a change of the solve precision and save / restore.  In REVERSIBLE mode
 * p_min is kept and updated all the same; no evaluator reads it.
 *
 * set_rock_regions(NULL) removes the regions (and p_min): the context is again the one that never had any, and runs the kernels that one
 * runs.  A new set of regions keeps p_min.  OPMGPU_EINVAL (with text, the previous set stays in force) for: a NULL array; nregions < 1; a rocknum outside [0, nregions); an
 * unknown mode; tab_ptr not starting at 0 or decreasing; a table of exactly 1 row; a p that is not strictly increasing; a non-finite
 * entry; pv_mult <= 0; trans_mult < 0; a non-finite rock_pref / rock_comp; a PVCDO context or a context with dissolution limits
 * (opmgpu_set_pvcdo and opmgpu_set_dissolution_limits in turn refuse a context with rock regions).  set_rock_history (restart): a NaN, or
 * no regions are set.  get_rock_history without regions gives +inf.  get_rock_multipliers: pv_mult and trans_mult of every cell at the
 * resident state (one kernel; either pointer may be NULL; without regions the multipliers of the rock of opmgpu_tables); OPMGPU_EINVAL
 * before a state has been set.
 *
 * Decomposed runs are rank-local: a rank passes the regions of its local cells, ghosts included (a ghost's trans_mult enters the owner's
 * flux), and updates its own plane; nothing is communicated. */
#define OPMGPU_ROCK_REVERSIBLE 0
#define OPMGPU_ROCK_IRREVERSIBLE 1
typedef struct opmgpu_rock_regions {
    int32_t nregions, mode;
    const int32_t* rocknum;                            /* [nc] caller order, 0-based */
    const double  *rock_pref, *rock_comp;              /* [nregions] */
    const int32_t* tab_ptr;                            /* [nregions+1] */
    const double  *tab_p, *tab_pvmult, *tab_transmult; /* [tab_ptr[nregions]] */
} opmgpu_rock_regions;
int opmgpu_set_rock_regions(opmgpu_ctx* ctx, const opmgpu_rock_regions* regions /* NULL: back to the rock of opmgpu_tables */);
int opmgpu_update_rock_history(opmgpu_ctx* ctx);
int opmgpu_get_rock_history(opmgpu_ctx* ctx, double* p_min /* [nc] */);
int opmgpu_set_rock_history(opmgpu_ctx* ctx, const double* p_min /* [nc] */);
int opmgpu_get_rock_multipliers(opmgpu_ctx* ctx, double* pv_mult /* [nc] or NULL */, double* trans_mult /* [nc] or NULL */);

/* Analytic aquifers (AQUFETP: Fetkovich, AQUCT: Carter-Tracy, connected by AQUANCON) as source terms of the water equation.  The reference
 * has no aquifers, so THE RULE IS OURS; it is stated here, restated independently under tests/ (tests/aquifer_reference.py) and pinned to
 * no other simulator.  All quantities are SI.  Every product and sum below is ONE IEEE float64 operation, evaluated in the order the
 * parentheses give (left to right where there are none) and never contracted into a fused multiply-add.
 *
 * An aquifer a feeds the connections j in [conn_ptr[a], conn_ptr[a+1]), each a pair (cell c_j, fraction alpha_j > 0) with sum_j alpha_j = 1
 * within 1e-12.  The GLOBAL connection index j (aquifers in order, the connections of one in the order given) is "the listing order".
 * Both models reduce to one linear law per connection and time step,
 *     q_j = A_j - B_j * pw_j          [reservoir m3/s of water, positive INTO the cell],
 * pw_j the water-phase pressure of c_j at the current iterate: the evaluator's VP_PW value p - pcow.
 *
 * Begin of a time step of length dt (opmgpu_aquifer_begin_step, after any state upload and again whenever a failed sub-step has restored
 * the saved state and a shorter dt is tried).  A_j and B_j are fixed here until the next begin.  Every connection evaluates its cell from
 * the RESIDENT state with the cell evaluator and keeps rho0_j = the water density and p0_j = the water pressure of c_j, and forms
 *     h_j = (rho0_j * g) * (z[c_j] - d_a)          (d_a the aquifer's datum depth, g the grid's gravity, z the cell depth).
 * Fetkovich (kind OPMGPU_AQUIFER_FETKOVICH; parameters p_a0, CtV0 = C_t V_0, J; state W_e = the cumulative reservoir volume), per aquifer
 *     p_a = p_a0 - W_e / CtV0,   tau = CtV0 / J,   x = dt / tau,   E = -expm1(-x) / x,   JE = J * E
 * and per connection
 *     B_j = alpha_j * JE,        A_j = B_j * (p_a + h_j).
 * (E = (1 - exp(-x)) / x makes the step exact for a constant cell pressure; expm1 keeps it accurate for small x.)
 * Carter-Tracy (OPMGPU_AQUIFER_CARTER_TRACY; parameters p_a0, beta, T_c and the influence table (t_D, P_D)[tab_ptr[a] .. tab_ptr[a+1]) of at
 * least 2 rows with strictly increasing t_D; state W_e and the aquifer time t = the sum of the committed dt), per aquifer
 *     tD = t / T_c,   tDp = (t + dt) / T_c,
 *     i = the segment of tDp by the rule of the PVT tables (Tabulated1DFunction: with n rows i = [t_D[1] < tDp] + sum_{k=2}^{n-2} [t_D[k] <= tDp],
 *         so the first and the last segment extrapolate linearly beyond the ends),
 *     Pp = (P_D[i+1] - P_D[i]) / (t_D[i+1] - t_D[i])   (formed once when the aquifers are set),   P = P_D[i] + Pp * (tDp - t_D[i]),
 *     den = P - tD * Pp,   Tden = T_c * den,   b = beta / Tden,
 * and per connection
 *     a_j = (beta * ((p_a0 + h_j) - p0_j) - W_e * Pp) / Tden,   B_j = alpha_j * b,   A_j = alpha_j * (a_j + b * p0_j).
 * A den that is not positive and finite makes opmgpu_aquifer_begin_step fail with OPMGPU_ENUMERICAL (text names the aquifer) and no step
 * is begun: it never becomes a NaN in the matrix.  p_a of a Carter-Tracy aquifer, as an output only, is p_a0 - W_e / beta.
 *
 * Assembly (every opmgpu_assemble and opmgpu_nonlinear_iteration while aquifers are set and a step has begun; behind the wells' terms).
 * ONE thread per distinct connected cell evaluates the cell (b_w and pw with their derivatives with respect to v = (p, Sw, X); d pw / d v
 * = (1, d pw / d Sw, 0)) and, for its connections in the listing order, starting from zeros,
 *     q_j = A_j - B_j * pw,   s += b_w * q_j,   d_v += (d b_w / d v) * q_j - (b_w * B_j) * (d pw / d v),
 * then R_water[c] -= s and, for the three entries of the water row of the cell's diagonal block, D[water][v] -= scale_water * d_v (the
 * sign convention of the well terms; in a float matrix the entry is widened, changed and rounded back once).  A cell may have connections
 * of several aquifers; no atomics, so the bits are the same from run to run.  No other equation, row or off-diagonal block changes.  The
 * float copy of a double Jacobian (preconditioner_single) and the CPR weights of the connected rows follow the final diagonal blocks.
 * Stated limit: outflow (q_j < 0) is not limited by the cell's mobile water.
 *
 * Commit (opmgpu_aquifer_commit_step, after a converged step): per aquifer, from the resident (converged) state, q_j as above and qs_j =
 * b_w,j * q_j per connection; Q = sum_j q_j and Qs = sum_j qs_j by THIS tree: with n connections numbered k = 0 .. n-1 within the aquifer,
 * slot T (0 <= T < 256) sums its connections k = T, T + 256, T + 512, ... in ascending order starting from 0.0; within each group of 64
 * consecutive slots (a wave) the slots are folded six times, v[l] = v[l] + v[l + off] for l < off with off = 32, 16, 8, 4, 2, 1 in
 * turn, leaving the wave's sum in its first slot; the four wave sums are added in order, ((w0 + w1) + w2) + w3.
 * Then W_e += dt * Q, W_s += dt * Qs (the surface volume, for the material balance), t += dt, and the step is no longer begun.
 *
 * Lifecycle.  A begun step that is not committed is discarded by the next begin, and by opmgpu_restore_state (how a failed sub-step is
 * handled); opmgpu_save_state and opmgpu_restore_state do not touch the committed state (W_e, W_s, t).  Aquifers and their state last
 * through opmgpu_set_wells / opmgpu_set_device_wells (a re-plan, which discards a begun step like it discards the saved state) and a
 * change of the solve precision.
 *
 * opmgpu_set_aquifers: NULL or naq == 0 removes the aquifers and the context is again the one that never had any; a new set starts with
 * W_e = W_s = t = 0.  OPMGPU_EINVAL (with text, the previous set stays in force) for: an unknown kind; a non-finite p_a0 or datum; a CtV0, J
 * (Fetkovich) or beta, T_c (Carter-Tracy) that is not finite and positive; an aquifer without connections; a cell out of range; an alpha
 * that is not finite and positive, or alphas not summing to 1 within 1e-12; the same cell twice in ONE aquifer; a Carter-Tracy table with
 * fewer than 2 rows, a non-finite entry or t_D not strictly increasing; a context with a communicator attached (opmgpu_comm_init* in turn
 * refuses a context with aquifers).  begin_step: OPMGPU_EINVAL for dt <= 0 or not finite, without aquifers, or before a state has been
 * set.  commit_step: OPMGPU_EINVAL without a begun step.  state_get / state_set: per aquifer W_e, W_s, t (any pointer may be NULL); p_a is
 * a derived output of get; set refuses non-finite values and discards a begun step.  connections_get: out[6 j + 0..5] = rho0_j, p0_j, A_j,
 * B_j and, at the RESIDENT state, q_j and qs_j (tests, summary output); OPMGPU_EINVAL without a begun step. */
enum { OPMGPU_AQUIFER_FETKOVICH = 0, OPMGPU_AQUIFER_CARTER_TRACY = 1 };
typedef struct opmgpu_aquifers {
    int32_t        naq;
    const int32_t* kind;          /* [naq] OPMGPU_AQUIFER_*                                                  */
    const double*  p_a0;          /* [naq] initial aquifer pressure at the datum                             */
    const double*  datum;         /* [naq] datum depth d_a                                                   */
    const double*  CtV0;          /* [naq] Fetkovich: total compressibility x initial water volume (else ignored) */
    const double*  J;             /* [naq] Fetkovich: productivity index [m3/s/Pa] (else ignored)            */
    const double*  beta;          /* [naq] Carter-Tracy: influx constant [m3/Pa] (else ignored)              */
    const double*  Tc;            /* [naq] Carter-Tracy: time constant [s] (else ignored)                    */
    const int32_t* tab_ptr;       /* [naq+1] rows of the influence tables (a Fetkovich aquifer has none); NULL without Carter-Tracy aquifers */
    const double*  tab_td;        /* [tab_ptr[naq]]                                                          */
    const double*  tab_pd;        /* [tab_ptr[naq]]                                                          */
    const int32_t* conn_ptr;      /* [naq+1]                                                                 */
    const int32_t* conn_cell;     /* [conn_ptr[naq]] caller cell index                                       */
    const double*  conn_alpha;    /* [conn_ptr[naq]]                                                         */
} opmgpu_aquifers;
enum { OPMGPU_AQUIFER_CONN_K = 6 };
int opmgpu_set_aquifers(opmgpu_ctx* ctx, const opmgpu_aquifers* aquifers);
int opmgpu_aquifer_begin_step(opmgpu_ctx* ctx, double dt);
int opmgpu_aquifer_commit_step(opmgpu_ctx* ctx);
int opmgpu_aquifer_state_get(opmgpu_ctx* ctx, double* W_e /* [naq] or NULL */, double* W_s, double* t, double* p_a);
int opmgpu_aquifer_state_set(opmgpu_ctx* ctx, const double* W_e /* [naq] or NULL */, const double* W_s, const double* t);
int opmgpu_aquifer_connections_get(opmgpu_ctx* ctx, double* out /* [nconn][OPMGPU_AQUIFER_CONN_K] */);

/* Hysteresis history (EclHysteresisTwoPhaseLawParams::update, called once per report step by SimulatorBase_impl.hpp:190-191 ->
 * BlackoilPropsAdFromDeck::updateSatHyst): update = take the resident state's saturations into the history (krnSwMdc of both two-phase
 * systems = running minimum of 1 - So resp. 1 - Sg, the reference's "inconsistent" update) and recompute the Carlson shifts.
 * set / get: the two history planes [nc] each (restart); they start at the no-history value 2.0 (EclHysteresisTwoPhaseLawParams). */
int opmgpu_update_hysteresis(opmgpu_ctx* ctx);
int opmgpu_set_hysteresis(opmgpu_ctx* ctx, const double* krn_sw_mdc_ow, const double* krn_sw_mdc_go);
int opmgpu_get_hysteresis(opmgpu_ctx* ctx, double* krn_sw_mdc_ow, double* krn_sw_mdc_go, double* delta_ow, double* delta_go);
/* (Under OPMGPU_HYST_KILLOUGH, below, the two delta planes hold the offsets of the affine form the device evaluates the scanning curves
 * in, with Carlson's signs: the imbibition krow is read at  m_ow Sw_ow + delta_ow,  the imbibition krg at  m_go Sg - delta_go;  that is
 * delta_ow = 1 - Sncri_ow - m_ow (1 - Sncrt_ow),  delta_go = m_go Sncrt_go - Sncri_go.) */

/* The model of the non-wetting phases' scanning curves (EHYSTR item 2): OPMGPU_HYST_CARLSON, the default and what every context has
 * until this call, or OPMGPU_HYST_KILLOUGH with killough_a = EHYSTR item 4 (0.1 in a deck that defaults it).  opm-material's Killough
 * model is not part of the reference tree, so the rule is OURS:
 *
 *   Two two-phase systems per cell, as for Carlson.  Sn is the non-wetting saturation, mdc the system's history plane.
 *     gas-oil:    Sn = Sg.  krnd = the cell's drainage krg (SATNUM table through eps[] / eps_v[]), krni = its imbibition krg (IMBNUM
 *                 table through ieps[]).  Shy = 1 - krn_sw_mdc_go.
 *     oil-water:  Sn = 1 - Sw_ow with Sw_ow = Sg + max(Sw, Swco), the abscissa of krow in the three-phase law.  krnd(S) = the cell's
 *                 drainage krow at 1 - S, krni likewise from the imbibition curve.  Shy = 1 - krn_sw_mdc_ow.
 *   The history planes, their update (once per report step, opmgpu_update_hysteresis) and the switch between the drainage and the
 *   scanning curve (scanning where 1 - Sn > mdc) are Carlson's.  Wetting phases stay on their drainage curves; capillary pressure
 *   carries no hysteresis.
 *
 *   Per cell and system:  Sncrd = the largest Sn at which the scaled drainage curve is still zero (the end of the table's run of zeros,
 *   mapped through the cell's scaling),  Sncri = the same of the imbibition table through the imbibition scaling,  Snmax = the largest
 *   non-wetting saturation of the scaled drainage curve (gas: the last Sg node; oil: 1 - the first Sw node),  a = killough_a.
 *   With a history (mdc < 2) and Shy clamped to at most Snmax:
 *     kd = krnd(Shy),  ki = krni(Snmax),  D = Shy - Sncrd
 *     C     = 1 / (Sncri - Sncrd) - 1 / (Snmax - Sncrd)
 *     Sncrt = Sncrd + D / (1 + a (Snmax - Shy) + C D)                           (Land / Killough trapped saturation)
 *     m     = (Snmax - Sncri) / (Shy - Sncrt),   R = kd / ki
 *     krn(Sn) = R krni(Sncri + m (Sn - Sncrt)),   d krn / d Sn = R m krni'(.)    on the scanning side
 *   Guards, exact and without tolerances:  kd <= 0, ki <= 0 or Snmax <= Sncri  ->  R = m = 0 (the scanning side is zero, which is
 *   the drainage curve there);  Sncri <= Sncrd, or a drainage curve without a mobile range (Snmax <= Sncrd)  ->  Sncrt = Sncrd.
 *   The manual's form divides by krnd(Snmax); this one divides by krni(Snmax), so the curve is continuous at the turning point whatever
 *   the tables are, and equals the manual's where the two curves meet at Snmax, as decks make them.  Shy = Snmax gives the imbibition
 *   curve itself.  Without a history (mdc = 2) m = R = 1, Sncrt = 0 and the offsets are 0.
 *
 * The call recomputes the derived planes of a resident history and makes a loaded matrix stale (assemble again).  The model is no part
 * of the saved state, of the tables or of the plan: it lasts through opmgpu_save_state / opmgpu_restore_state, a change of the solve's
 * precision, opmgpu_set_wells / opmgpu_set_device_wells and a re-plan.  Multi-GPU: rank-local, no communication.
 * OPMGPU_EINVAL with text in opmgpu_last_error(ctx), nothing changed: a context without hysteresis (opmgpu_grid.imbnum == NULL); a model
 * that is neither of the two; a killough_a that is not finite or is negative. */
#define OPMGPU_HYST_CARLSON  0
#define OPMGPU_HYST_KILLOUGH 2
int opmgpu_set_hysteresis_model(opmgpu_ctx* ctx, int model, double killough_a);
/* The scanning-curve parameters in force, [nc] each in the caller's order, any pointer may be NULL: Sncrt, m and R of the oil-water and
 * of the gas-oil system.  Under OPMGPU_HYST_CARLSON m = R = 1 and Sncrt = 0 (not computed).  OPMGPU_EINVAL without hysteresis. */
int opmgpu_get_hysteresis_scanning(opmgpu_ctx* ctx, double* sncrt_ow, double* m_ow, double* r_ow, double* sncrt_go, double* m_go, double* r_go);

/* NonlinearSolver::stabilizeNonlinearUpdate (NonlinearSolver_impl.hpp:260-301) on the resident
 * increment: dx_old <- dx, then DAMPEN: dx *= omega, SOR: dx = omega*dx + (1-omega)*dx_old(previous).
 * dx_old is zeroed by opmgpu_assemble(initial_assembly = 1) (BlackoilModelBase_impl.hpp:254-260).
 * The oscillation detection itself (detectOscillations, :221-257) works on the three L-inf norms
 * that opmgpu_convergence returns and stays with the caller (host/opmgpu.hpp, opmgpu/model.py). */
#define OPMGPU_RELAX_DAMPEN 0
#define OPMGPU_RELAX_SOR 1
int opmgpu_stabilize_update(opmgpu_ctx* ctx, int relax_type, double omega);

/* ------------------------------------------------------------------------------------------
 * B1 boundary: NewtonIterationBlackoilInterface::computeNewtonIncrement
 * (NewtonIterationBlackoilInterface.hpp:31-52) with the matrix supplied by the reference's own
 * AD assembly after formInterleavedSystem (NewtonIterationBlackoilInterleaved.cpp:110-194):
 * BCRSMatrix<3x3> as BSR (rowptr[nb+1], col[nnzb], val[nnzb*9] row-major blocks), rhs/x
 * block-interleaved [nb][3] like Dune BlockVector.  The context may come from
 * opmgpu_create_solver (no grid/tables).  The sparsity plan is cached while the pattern
 * is unchanged. */
int opmgpu_create_solver(opmgpu_ctx** ctx, int device, const opmgpu_params* params);
int opmgpu_solve_bsr(opmgpu_ctx* ctx, int nb, const int32_t* rowptr, const int32_t* col,
                     const double* val9, const double* rhs3, int single_precision, double* x3,
                     int* iters, double* reduction);

/* ------------------------------------------------------------------------------------------
 * Kernel-level entry points (parity tests, roofline bench).  They operate on the matrix held
 * by the context: the last opmgpu_solve_bsr / opmgpu_load_bsr / opmgpu_assemble system.
 * ---------------------------------------------------------------------------------------- */
int opmgpu_load_bsr(opmgpu_ctx* ctx, int nb, const int32_t* rowptr, const int32_t* col,
                    const double* val9, int single_precision);
/* y = A x, x/y block-interleaved [nb][3] (MatrixAdapter::apply, used at ISTLSolver.hpp:267). */
int opmgpu_spmv(opmgpu_ctx* ctx, const double* x3, double* y3);
/* ILU0 of the loaded matrix (ParallelOverlappingILU0 ctor) and one application
 * v = w * U^-1 L^-1 d (its apply()). */
int opmgpu_ilu0_factor(opmgpu_ctx* ctx);
int opmgpu_ilu0_apply(opmgpu_ctx* ctx, const double* d3, double* v3);
/* factors back in the caller's BSR layout: L strictly lower / U strictly upper blocks in the
 * slots of the input pattern w.r.t. the ELIMINATION order, diagonal slot = inverted pivot. */
int opmgpu_ilu0_get(opmgpu_ctx* ctx, double* val9);
/* elimination position of every caller row (perm[row] = position) and its level. */
int opmgpu_get_ordering(opmgpu_ctx* ctx, int32_t* position, int32_t* level, int32_t* nlevels);
/* per-cell 0/1 weights of the CPR pressure equation after a solve with use_cpr (formEllipticSystem's dominance test,
 * NewtonIterationUtilities.cpp:212-252): w[3*nb], equation-major (water, oil, gas), caller row order. */
int opmgpu_get_cpr_weights(opmgpu_ctx* ctx, double* w);
/* assembled reservoir system back to the host in caller numbering: residual (unscaled,
 * equation-major 3*nc), and the matbal-scaled Jacobian in BSR. */
int opmgpu_get_residual(opmgpu_ctx* ctx, double* r);
int opmgpu_get_jacobian_nnzb(opmgpu_ctx* ctx, int32_t* nnzb);
int opmgpu_get_jacobian_bsr(opmgpu_ctx* ctx, int32_t* rowptr, int32_t* col, double* val9);
/* diagnostic (mixed precision, preconditioner_single): the float copy of the DOUBLE Jacobian that came with the last assembly, widened, in
 * the block order of opmgpu_get_jacobian_bsr.  OPMGPU_EINVAL (with text) when the context holds no such copy at the moment -- a float
 * assembly, no copy written, or one that is stale: the solve then makes it from the double matrix. */
int opmgpu_get_jacobian_float_copy(opmgpu_ctx* ctx, double* val9);
/* timing of device work: runs `reps` launches of one kernel on the context's stream between two
 * hipEvents and returns the average milliseconds per launch (HIP events on the launch stream). */
enum { OPMGPU_K_SPMV = 0, OPMGPU_K_ILU_APPLY = 1, OPMGPU_K_ILU_FACTOR = 2, OPMGPU_K_ASSEMBLE = 3,
       OPMGPU_K_DOT = 4, OPMGPU_K_AXPY = 5, OPMGPU_K_PROPS = 6, OPMGPU_K_STREAM_COPY = 7,
       OPMGPU_K_CPR_APPLY = 8 /* whole two-stage preconditioner application */, OPMGPU_K_VCYCLE = 9 /* its AMG V-cycle alone */,
       OPMGPU_K_CPR_SETUP = 10 /* pressure extraction + Galerkin + coarsest inverse */,
       OPMGPU_K_SPMV_COLD = 11 /* the SpMV rotating over copies of the matrix that together exceed the 256 MiB Infinity Cache: HBM-resident operands */ };
int opmgpu_time_kernel(opmgpu_ctx* ctx, int kernel, int reps, double* ms_per_launch);
/* In-situ timing of kernel CLASSES during real Newton iterations: after opmgpu_kernel_timing(ctx, 1) every launch (group) of a class
 * is bracketed by a HIP event pair on the launch stream; opmgpu_kernel_timing_get sums the elapsed times per class since the switch-on
 * (total_ms[OPMGPU_KT_COUNT], launches[OPMGPU_KT_COUNT] bracket counts).  Off by default -- the brackets cost a few microseconds each,
 * so bench.py uses a separate profiled pass for its per-kernel roofline table. */
enum { OPMGPU_KT_CELL_PROPS = 0, OPMGPU_KT_FLUX, OPMGPU_KT_WELLS, OPMGPU_KT_CONV, OPMGPU_KT_ILU_FACTOR, OPMGPU_KT_CPR_SETUP, OPMGPU_KT_SPMV1,
       OPMGPU_KT_SPMV2, OPMGPU_KT_ILU_APPLY, OPMGPU_KT_VCYCLE, OPMGPU_KT_CPR_OTHER, OPMGPU_KT_VECTOR, OPMGPU_KT_UPDATE_STATE, OPMGPU_KT_COUNT };
int opmgpu_kernel_timing(opmgpu_ctx* ctx, int enable);
int opmgpu_kernel_timing_get(opmgpu_ctx* ctx, double* total_ms, int64_t* launches);
/* elapsed device milliseconds of the last assemble / solve / update_state call. */
int opmgpu_last_timings(opmgpu_ctx* ctx, double* assemble_ms, double* solve_ms, double* update_ms);
/* Per-call timing of opmgpu_nonlinear_iteration WITHOUT a synchronisation inside the timed calls (the median over the Newton
 * iterations that include a linear solve).  After opmgpu_iteration_marks(ctx, 1) every call records one event on the library's stream when
 * it has enqueued its last kernel, and one event pair around each of its phases; opmgpu_iteration_marks_get waits for the last recorded
 * event and returns for the first max_calls calls since the switch-on: call_ms[i] = device time from the end of call i - 1 (the switch-on
 * for i = 0) to the end of call i -- the host round trips of an iteration serialise consecutive calls, so this is the iteration's wall
 * time --, solved[i] = 1 if the call ran solveJacobianSystem + updateState (a converged call does not: BlackoilModelBase_impl.hpp:277-281),
 * linear_iterations[i], phase_ms[3 i + {0, 1, 2}] = assemble / solve / update (0 where the phase did not run).  Any output may be NULL;
 * *n_calls = calls made since the switch-on.  At most 16384 calls are recorded (later ones run unmarked and only count); the events are
 * recycled through a pool that lives as long as the context.  opmgpu_iteration_marks(ctx, 0) switches off and returns the events to it. */
int opmgpu_iteration_marks(opmgpu_ctx* ctx, int enable);
int opmgpu_iteration_marks_get(opmgpu_ctx* ctx, int max_calls, double* call_ms, int32_t* solved, int32_t* linear_iterations, double* phase_ms, int* n_calls);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU (domain decomposition with a one-cell halo; mirrors owner/overlap of
 * ParallelISTLInformation, ISTLSolver.hpp:286-298).  One process per GPU; the RCCL unique id
 * is created on rank 0 and handed to the other ranks by the caller (torch.distributed / MPI).
 * Cells [0, n_owned) of the rank-local grid are owned, [n_owned, nc) are ghosts.
 * send lists name owned local cells, recv lists name ghost local cells, grouped per
 * neighbour rank.
 * ---------------------------------------------------------------------------------------- */
#define OPMGPU_UNIQUE_ID_BYTES 128
int opmgpu_comm_unique_id(uint8_t* id /*OPMGPU_UNIQUE_ID_BYTES*/);
int opmgpu_comm_init(opmgpu_ctx* ctx, int rank, int nranks, const uint8_t* id, int32_t n_owned,
                     int n_neigh, const int32_t* neigh_rank, const int32_t* send_ptr,
                     const int32_t* send_cells, const int32_t* recv_ptr, const int32_t* recv_cells);

/* The same communicator over a caller-supplied TRANSPORT instead of RCCL -- e.g. the MPI communicator flow_legacy already owns
 * (ParallelISTLInformation), or the shared-memory test transport of tests/support.  The library calls back for its two
 * primitives, both on device buffers and ordered on the given HIP stream (the callback enqueues on it or synchronises it):
 *   allreduce: in-place sum (is_max = 0) or max of n doubles;
 *   exchange:  for every neighbour q send scount[q] bytes from sbuf + soff[q] to rank neigh_rank[q] and receive rcount[q] bytes
 *              from it into rbuf + roff[q] (byte offsets / counts).
 * The stream is not always the same one: exchanges of the solver arrive on the library's second ("halo") stream while the rows that
 * need no ghost value are multiplied on the main stream; calls are issued in the same order on every rank and never concurrently.
 * A non-zero return value becomes OPMGPU_ECOMM.  The struct is copied; `destroy(self)` is called when the context goes away. */
typedef struct opmgpu_transport {
    void* self;
    int  (*allreduce)(void* self, double* dbuf, int n, int is_max, void* hip_stream);
    int  (*exchange)(void* self, int n_neigh, const int32_t* neigh_rank, const void* sbuf, const int64_t* soff, const int64_t* scount,
                     void* rbuf, const int64_t* roff, const int64_t* rcount, void* hip_stream);
    void (*destroy)(void* self);
    /* OPTIONAL (may be NULL: the library then calls allreduce and exchange one after the other).  One all-reduce (sum) and one neighbour
     * exchange that do not depend on each other, as ONE operation -- the decomposed GMRES sends the new basis vector's halo together with
     * its projections, and the pressure correction's halo together with the coarse space's restricted residual: two latencies per column
     * instead of four.  The built-in RCCL transport issues them back to back by default (OPMGPU_RCCL_FUSED=1: one ncclGroup). */
    int  (*allreduce_exchange)(void* self, double* dbuf, int n, int n_neigh, const int32_t* neigh_rank, const void* sbuf, const int64_t* soff,
                               const int64_t* scount, void* rbuf, const int64_t* roff, const int64_t* rcount, void* hip_stream);
} opmgpu_transport;
/* Coarse space of the decomposed pressure stage: by default one unknown per rank in runs with wells (index-range
 * blocks of the owned cells would cut the wells, which was measured to hurt), m = 4 index-range blocks without.  A caller that knows the
 * geometry supplies m <= 8 blocks per rank that keep every well inside ONE block -- e.g. sub-slabs along the cut direction for vertical
 * wells: block_of_owned_cell[c] in [0, m) for the owned cells in local numbering.  Same m on every rank; m = 0 restores the default.
 * Call after opmgpu_comm_init*, before the first CPR solve (the map is agreed collectively there). */
int opmgpu_comm_set_coarse_blocks(opmgpu_ctx* ctx, int m, const int32_t* block_of_owned_cell);
/* Pressure hierarchy of the decomposed CPR stage: 0 = rank-local levels below a level 0 that sees the neighbours, plus one coarse unknown
 * per rank (Nicolaides); 1 = a distributed hierarchy whose levels span all ranks -- aggregates inside a rank, Galerkin products with the
 * couplings to the neighbours' aggregates, an exchange before every operation that reads them, and the levels of at most 384 global
 * rows replicated on every rank (one all-reduce per cycle into them).  Default: OPMGPU_CPR_GLOBAL_AMG (1 = mode 1, else 0), read at
 * opmgpu_comm_init*.  Call after opmgpu_comm_init*, before the first CPR solve; no effect on one rank.  OPMGPU_EINVAL for another
 * mode, and for mode 1 with level-0 Gauss-Seidel (OPMGPU_AMG_GS; with OPMGPU_CPR_GLOBAL_AMG=1 the default then stays 0, with a message on
 * stderr).  In mode 1 building the hierarchy is collective (all-reduces and neighbour exchanges), like the solve: every call that drops
 * it -- opmgpu_set_device_wells, a change of the sparsity pattern, a change of the mode -- must be made on all ranks alike, so that all
 * rebuild it at the same CPR solve. */
int opmgpu_comm_set_pressure_hierarchy(opmgpu_ctx* ctx, int mode);
int opmgpu_comm_init_transport(opmgpu_ctx* ctx, int rank, int nranks, const opmgpu_transport* transport, int32_t n_owned,
                               int n_neigh, const int32_t* neigh_rank, const int32_t* send_ptr,
                               const int32_t* send_cells, const int32_t* recv_ptr, const int32_t* recv_cells);

/* ----------------------------------------------------------------------------------------
 * One whole Newton iteration in one call: BlackoilModelBase::nonlinearIteration (BlackoilModelBase_impl.hpp:239-326) with the
 * update stabilisation of NonlinearSolver (NonlinearSolver_impl.hpp:221-301) --
 *   iteration == 0: the residual-norm history and the relaxation factor are reset;
 *   assemble(initial = iteration == 0) -> getConvergence (reservoir, and the wells of the device well model) ->
 *   if not converged, or iteration < min_iter:  solveJacobianSystem -> detectOscillations -> stabilizeNonlinearUpdate -> updateState.
 * It is the sequence opmgpu_set_solve_precision / assemble / convergence / well_convergence / solve / stabilize_update / update_state
 * that the host mirrors issue call by call (opmgpu/model.py, host/opmgpu.hpp), with the host round trips between them inside the
 * library: the GPU idles ~0.1 ms per iteration less.  The history lives in the context.  Status codes as for the single calls.
 * ---------------------------------------------------------------------------------------- */
typedef struct opmgpu_newton_ctl {
    int32_t min_iter;                  /* 1   (NonlinearSolver: min_iter_) */
    int32_t use_update_stabilization;  /* 1   (BlackoilModelParameters::use_update_stabilization_) */
    int32_t relax_type;                /* OPMGPU_RELAX_DAMPEN */
    double  relax_max;                 /* 0.5 */
    double  relax_increment;           /* 0.1 */
    double  relax_rel_tol;             /* 0.2 */
} opmgpu_newton_ctl;
int opmgpu_nonlinear_iteration(opmgpu_ctx* ctx, double dt, int iteration, int single_precision, const opmgpu_newton_ctl* ctl,
                               int* converged, int* linear_iterations, double* linf3 /* may be NULL */, double* relaxation /* may be NULL */);

/* Host-only planning entry (no device needed): elimination position and level of every row for
 * the given ordering -- the same plan opmgpu_get_ordering reports for a loaded matrix. */
int opmgpu_plan_ordering(int nb, const int32_t* rowptr, const int32_t* col, int ordering,
                         int32_t* position, int32_t* level, int32_t* nlevels);

/* library / build information */
const char* opmgpu_version(void);
int opmgpu_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* OPMGPU_H */
