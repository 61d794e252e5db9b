/* ckmi.h -- C ABI of libckmi.so, the MI355X (gfx950) batched batch-reactor engine.
 *
 * This is the drop-in boundary for PyChemkin's batch-reactor hot path.  The reference
 * reaches the closed Chemkin library through ctypes (chemkin_wrapper.py:244,271-272) with
 * Fortran-style by-pointer scalars, caller-allocated arrays and an int error return
 * (0 = success).  libckmi keeps that convention and adds batched entry points that take
 * device-resident struct-of-arrays buffers:
 *
 *   ckmi_mech_create        replaces KINPreProcess + KINGetChemistrySizes + table getters
 *                           (chemkin_wrapper.py:303-316,333-397; chemistry.py:675-703).
 *                           The Chemkin-format text is parsed on the host
 *                           (pychemkin_amd/mechanism.py) and handed over as flat tables.
 *   ckmi_rop_thermo         batched KINGetGasROP + KINGetGasMixtureSpecificHeat /
 *                           KINGetGasMixtureEnthalpy (chemkin_wrapper.py:427-440,482-489;
 *                           mixture.py:1236,1341,1442).
 *   ckmi_reaction_rates     batched KINGetGasReactionRates (chemkin_wrapper.py:490-498;
 *                           mixture.py:1551).
 *   ckmi_species_thermo     batched KINGetGasSpecificHeat / SpeciesEnthalpy /
 *                           SpeciesInternalEnergy (chemkin_wrapper.py:375-392).
 *   ckmi_reactor_run        batched KINAll0D_SetupBatchInputs + KINAll0D_SetUserKeyword +
 *                           KINAll0D_Calculate + KINAll0D_GetIgnitionDelay +
 *                           KINAll0D_GetGasSolnResponse (chemkin_wrapper.py:606-618,
 *                           688-689,698-699,751-763; batchreactor.py:1036-1159,582,1396).
 *   ckmi_set_afactor /      KINSetAFactorForAReaction / KINGetReactionRateParameters
 *   ckmi_get_arrhenius      (chemkin_wrapper.py:499-511; chemistry.py:1627,1665).
 *
 * All buffers passed to ckmi_rop_thermo / ckmi_reaction_rates / ckmi_species_thermo /
 * ckmi_reactor_run are device pointers on the handle's device; `stream` is a hipStream_t
 * (NULL = default stream).  The calls are asynchronous on that stream.
 */
#ifndef CKMI_H
#define CKMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version returned by ckmi_version(): bumped whenever a struct layout or a table stride changes.
 * 1: round-1/2 layout (CKMI_SLOTS 4, ckmi_reactor_cfg up to prof3_v); 2: CKMI_SLOTS 8, cfg.eng[20], cfg.tran;
 * 3: desc.MM / desc.ncf (element counts) and cfg.no_elem_proj. */
#define CKMI_ABI_VERSION 3

/* the reactor kernels hold element conservation (ckmi_reactor_cfg.no_elem_proj) for mechanisms whose
 * species contain at most this many distinct elements */
#define CKMI_PROJ_MMAX 8

#define CKMI_SLOTS 8 /* distinct species per reaction side in the flat tables ([II][CKMI_SLOTS] arrays) */

/* reaction types */
#define CKMI_RXN_ELEMENTARY 0
#define CKMI_RXN_THIRDBODY 1
#define CKMI_RXN_FALLOFF 2
#define CKMI_RXN_PLOG 3 /* elementary with a PLOG table: ln k linear in ln P, clamped outside */
#define CKMI_RXN_CHEMACT 4 /* chemically activated: arr = k0, low = HIGH (k_inf); k = k0 F / (1 + Pr) */
/* Chebyshev (TCHEB / PCHEB / CHEB on a (+M) reaction): log10 k = sum_t sum_p a[t][p] T_t(Tr) T_p(Pr),
 * Tr = (2/T - 1/Tmin - 1/Tmax) / (1/Tmax - 1/Tmin), Pr = (2 log P - log Pmin - log Pmax) /
 * (log Pmax - log Pmin), no [M] factor, not clamped outside the range.  Its plog_par rows:
 * (NT, NP, 0, 0), (Tmin [K], Tmax [K], Pmin [atm], Pmax [atm]), then a[t][p] t-major, 4 per row. */
#define CKMI_RXN_CHEB 5
/* Landau-Teller elementary reaction: k = A T^b exp(-E/RT + B T^(-1/3) + C T^(-2/3)), low = (B, C, 0);
 * with REV, fpar[0..1] = the RLT (B, C) of the reverse rate */
#define CKMI_RXN_LT 6
/* falloff forms */
#define CKMI_FALL_NONE 0
#define CKMI_FALL_LINDEMANN 1
#define CKMI_FALL_TROE3 2
#define CKMI_FALL_TROE4 3
#define CKMI_FALL_SRI 4

/* error codes (0 = success, as the KIN* functions) */
#define CKMI_OK 0
#define CKMI_ERR_ARG 1
#define CKMI_ERR_HIP 2
#define CKMI_ERR_SIZE 3
#define CKMI_ERR_UNSUPPORTED 4

/* Flat mechanism tables (host pointers), layout produced by Mechanism.to_tables(). */
typedef struct {
  int32_t KK, II;
  const double* wt;       /* [KK] molecular weights, g/mol */
  const double* thermo;   /* [KK][17]: tlow, tmid, thigh, low a1..a7, high a1..a7 */
  const int32_t* rtype;   /* [II] CKMI_RXN_* */
  const int32_t* rev;     /* [II] 1 reversible */
  const int32_t* nr;      /* [II] reactant slots used */
  const int32_t* np;      /* [II] product slots used */
  const int32_t* rsp;     /* [II][CKMI_SLOTS] reactant species */
  const int32_t* psp;     /* [II][CKMI_SLOTS] product species */
  const double* rnu;      /* [II][CKMI_SLOTS] reactant stoichiometric coefficients */
  const double* pnu;      /* [II][CKMI_SLOTS] product stoichiometric coefficients */
  const double* arr;      /* [II][3] ln A (cgs), b, E/R (K) */
  const double* low;      /* [II][3] falloff low-pressure limit */
  const double* revp;     /* [II][3] explicit reverse parameters (REV) */
  const int32_t* has_rev; /* [II] */
  const int32_t* ftype;   /* [II] CKMI_FALL_* */
  const double* fpar;     /* [II][5] TROE a,T***,T*,T** or SRI a,b,c,d,e */
  const int32_t* tbsp;    /* [II] -1 mixture M, else collider species index */
  const int32_t* eff_ptr; /* [II+1] CSR into eff_sp / eff_val */
  const int32_t* eff_sp;
  const double* eff_val;  /* third-body efficiencies (absolute) */
  const int32_t* plog_ptr; /* [II+1] CSR into plog_par for CKMI_RXN_PLOG reactions (may be NULL if none) */
  const double* plog_par;  /* [npl][4] ln P (dyn/cm2), ln A (cgs), b, E/R (K); ascending, distinct P */
  const double* ford;      /* [II][CKMI_SLOTS] forward order of each reactant slot (FORD; = rnu without it), or NULL */
  const double* rord;      /* [II][CKMI_SLOTS] reverse order of each product slot (RORD; = pnu without it), or NULL */
  int32_t MM;              /* elements (0 with ncf NULL: the reactors do not hold element conservation) */
  const int32_t* ncf;      /* [MM][KK] element counts of each species (KINGetGasSpeciesComposition), or NULL */
} ckmi_mech_desc;

typedef struct ckmi_mech ckmi_mech; /* opaque: tables resident in HBM of one device */

/* Reactor-run configuration (one per batch; the reference passes these as keyword text,
 * reactormodel.py:966-996, batchreactor.py:1106-1114). */
typedef struct {
  int32_t energy;      /* 1 ENERGY equation, 2 given (constant) temperature */
  double t_end;        /* TIME [s] */
  double atol, rtol;   /* ATOL / RTOL */
  double h0;           /* HO initial step [s], 0 = estimate */
  double hmax;         /* STPT max step [s], 0 = t_end/100 */
  int32_t nneg;        /* NNEG */
  int32_t ign_mode;    /* 0 none, 1 TIFP, 2 DTIGN, 3 TLIM, 4 KLIM */
  double ign_val;      /* DTIGN rise [K] or TLIM temperature [K] */
  int32_t ign_species; /* KLIM species index */
  int32_t ign_stop;    /* IGN_STOP */
  int32_t max_steps;   /* 0 = 200000 */
  int32_t nprof;       /* VPRO (CONV) / PPRO (CONP) / TPRO profile points, 0 = none (<= 64) */
  double prof_t[64];
  double prof_v[64];
  int32_t prof_kind;   /* 0: the profile is VPRO (CONV) or PPRO (CONP); 1: TPRO (energy = 2) */
  double gfac;         /* GFAC gas-phase rate multiplier (reactormodel.py:1452-1468); 0 is read as 1 */
  double qloss;        /* QLOS heat loss rate to the surroundings [cal/s] (batchreactor.py:1884-1907) */
  double htc;          /* HTC wall heat-transfer coefficient [cal/cm2-K-s] (:1910-1939) */
  double areaq;        /* AREAQ heat-transfer area [cm2] (:1974-2003) */
  double tamb;         /* TAMB ambient temperature [K] (:1942-1971) */
  int32_t asteps;      /* ADAP/ASTEPS: extra solution point every asteps steps, 0 = off (:373-460) */
  int32_t avar;        /* ADAP/AVAR: extra point when variable avar changed by avalue since the last
                          one; -1 off, 0 temperature, 1 + k mass fraction of species k */
  double avalue;       /* AVALUE */
  int32_t nprof2;      /* second profile (energy runs), 0 = none (<= 64): */
  int32_t prof2_kind;  /* 1 QPRO heat loss rate [cal/s] (replaces QLOS), 2 AEXT area [cm2] (replaces AREAQ) */
  double prof2_t[64];
  double prof2_v[64];
  int32_t nprof3;      /* AEXT area profile [cm2] beside a QPRO in the second slot (prof2_kind 1): the */
  double prof3_t[64];  /* heat loss is then QPRO(t) + HTC AEXT(t) (T - TAMB) (batchreactor.py:2005-2067); */
  double prof3_v[64];  /* 0 = none (<= 64) */
  /* problem 4 (single-zone IC engine, KINAll0D_SetupHCCIInputs, engines/HCCI.py): CKMI_ENG_* parameters */
  double eng[20];
  /* [KK][8] device: ln-T cubics of ln eta_k [g/(cm s)] (0..3, ckmi_transport_fit) and ln lambda_k
   * [erg/(cm s K)] (4..7, ckmi_conductivity_fit) for the engine's ICHX wall heat transfer (else NULL) */
  const double* tran;
  /* 0 (default): element conservation is held to 0.1 rtol -- after an accepted step whose element content
   * (sum_k a_mk Y_k / W_k) has drifted by more than 0.1 rtol of the largest element content from the
   * initial mixture's, the corrector is projected back onto it (oracle/ckoracle.c elem_project);
   * 1: no projection (diagnostics) */
  int32_t no_elem_proj;
} ckmi_reactor_cfg;

/* engine parameter block (ckmi_reactor_cfg.eng; oracle/ckoracle.h CKO_ENG_* is the same layout) */
#define CKMI_ENG_CA0 0      /* DEG0 crank angle at t = 0 [deg] */
#define CKMI_ENG_RPM 1      /* RPM */
#define CKMI_ENG_CMPR 2     /* CMPR compression ratio */
#define CKMI_ENG_BORE 3     /* BORE [cm] */
#define CKMI_ENG_STROKE 4   /* STRK [cm] */
#define CKMI_ENG_LOLR 5     /* connecting rod length / crank radius */
#define CKMI_ENG_POLEN 6    /* POLEN piston pin offset [cm] */
#define CKMI_ENG_HTMODEL 7  /* 0 adiabatic, 1 ICHX (Nu = a Re^b Pr^c, tran required) */
#define CKMI_ENG_HTA 8
#define CKMI_ENG_HTB 9
#define CKMI_ENG_HTC 10
#define CKMI_ENG_TWALL 11   /* [K] */
#define CKMI_ENG_C11 12     /* GVEL Woschni C11 C12 C2 swirl ratio */
#define CKMI_ENG_C12 13
#define CKMI_ENG_C2 14
#define CKMI_ENG_SWIRL 15
#define CKMI_ENG_CYBAR 16   /* cylinder-head (clearance) surface / bore area */
#define CKMI_ENG_PSBAR 17   /* piston-head surface / bore area */

/* Optional per-reactor inputs / outputs of ckmi_reactor_run_ex (any pointer may be NULL). */
typedef struct {
  /* brute-force A-factor sensitivity (sensitivity.py:141-160, chemistry.py:1636-1678): reactor r
   * runs with the pre-exponential factor of reaction afac_rxn[r] (0-based, original order;
   * < 0 = none) multiplied by afac[r]. */
  const int32_t* afac_rxn; /* [n] device */
  const double* afac;      /* [n] device */
  /* adaptive solution points (cfg.asteps > 0): up to max_adap per reactor */
  int32_t max_adap;
  double* t_adap;          /* [n][max_adap] device */
  double* y_adap;          /* [n][max_adap][KK+1] device (T, Y) */
  int32_t* n_adap;         /* [n] device: points written */
  /* time of the final state (Tend, Yend): t_end, or the time the run stopped early (IGN_STOP,
   * solver failure).  DTSV rows after it (y_save) are NaN. */
  double* t_stop;          /* [n] device */
} ckmi_reactor_ext;

/* per-reactor statistics written by ckmi_reactor_run (int32 [n][8]) */
#define CKMI_STAT_NST 0
#define CKMI_STAT_NFE 1
#define CKMI_STAT_NJE 2
#define CKMI_STAT_NLU 3
#define CKMI_STAT_NCF 4
#define CKMI_STAT_NEF 5
#define CKMI_STAT_STATUS 6
#define CKMI_STAT_NNI 7 /* Newton iterations = linear solves */
#define CKMI_NSTAT 8

/* reactor status (CKMI_STAT_STATUS) */
#define CKMI_RUN_OK 0
#define CKMI_RUN_MAXSTEPS 1
#define CKMI_RUN_ERRTEST 2
#define CKMI_RUN_CONVFAIL 3
/* the state left the physical domain after an accepted step and the run was ended there: a mass
 * fraction below -max(1e-3, 1e3 atol), or (energy runs) T outside [min_k T_low,k / 2, 2 max_k T_high,k]
 * of the NASA-7 fits (the margin lets legitimately hot runs extrapolate the fits).  Without NNEG a loose tolerance can let trace concentrations go negative and
 * drive bimolecular rates of the wrong sign until the temperature runs away; the guard ends such a
 * reactor at once instead of letting it burn max_steps. */
#define CKMI_RUN_RUNAWAY 4
/* plug flow (problem 3) without a PPRO profile: the accepted state has no subsonic solution of the
 * inviscid momentum equation P + G u = P0 + G u0 any more (P0 + G u0)^2 < 4 G^2 R T / Wbar -- the
 * tube is choked (thermally, at the isothermal sound speed) and the run ends there */
#define CKMI_RUN_CHOKED 5
/* ckmi_psr_run: t_max was reached before the steady-state rule was met (the returned state is the
 * transient's state at t_max, resid its scaled residual) */
#define CKMI_RUN_NOT_STEADY 6

/* Native Chemkin-II interpreter (host only, no GPU): the parse half of KINPreProcess
 * (chemkin_wrapper.py:303-316).  chem.inp text (+ optional therm.dat text; an inline THERMO block
 * overrides it) -> the ckmi_mech_desc tables, symbols, atomic weights and element counts.  Same
 * grammar and bitwise the same tables as pychemkin_amd/mechanism.py (tests/test_parse_native.py).
 * The desc pointers stay valid until ckmi_parsed_free. */
typedef struct ckmi_parsed ckmi_parsed;
int ckmi_parse_mechanism(const char* chem_text, const char* therm_text, ckmi_parsed** out);
int ckmi_parse_files(const char* chemfile, const char* thermfile, ckmi_parsed** out);
const char* ckmi_parse_last_error(void);
void ckmi_parsed_free(ckmi_parsed* p);
int ckmi_parsed_sizes(const ckmi_parsed* p, int32_t* MM, int32_t* KK, int32_t* II);
int ckmi_parsed_desc(const ckmi_parsed* p, ckmi_mech_desc* desc);
/* species [KK][16] and elements [MM][16] NUL-padded, awt [MM], ncf [MM][KK] row-major (any may be NULL) */
int ckmi_parsed_symbols(const ckmi_parsed* p, char* species, char* elements, double* awt, int32_t* ncf);
/* reaction i (0-based) as written in the file, whitespace removed */
int ckmi_parsed_equation(const ckmi_parsed* p, int32_t i, char* buf, int32_t cap, int32_t* len);

const char* ckmi_last_error(void);
int ckmi_version(void);

/* Build device tables on the current HIP device. */
int ckmi_mech_create(const ckmi_mech_desc* desc, ckmi_mech** out);
int ckmi_mech_destroy(ckmi_mech* mech);
int ckmi_mech_sizes(const ckmi_mech* mech, int32_t* KK, int32_t* II);

/* A-factor get/set (original reaction order, 0-based); set takes effect for later calls. */
int ckmi_get_arrhenius(const ckmi_mech* mech, double* A, double* b, double* E_R);
int ckmi_set_afactor(ckmi_mech* mech, int32_t irxn, double A);
/* Device slot of every reaction (slot[II], original order): the rate kernels visit slots in strips of 64,
 * elementary reactions first, then third-body, then falloff.  A diagnostic for tests and profiling. */
int ckmi_reaction_slots(const ckmi_mech* mech, int32_t* slot);

/* Species thermo per state: cp/R, h/RT, s/R  (device, [KK][n] each; any may be NULL). */
int ckmi_species_thermo(const ckmi_mech* mech, int32_t n, const double* T, double* cp_R, double* h_RT,
                        double* s_R, void* stream);

/* Batched ROP + mixture thermo at (T, P, Y):  T[n], P[n] dyn/cm2, Y[KK][n] mass fractions
 * -> wdot[KK][n] mol/cm3-s, cp[n] erg/g-K, h[n] erg/g (cp and h may be NULL). */
int ckmi_rop_thermo(const ckmi_mech* mech, int32_t n, const double* T, const double* P, const double* Y,
                    double* wdot, double* cp, double* h, void* stream);

/* Kernel selection for ckmi_rop_thermo (process-wide): 0 = automatic (the mechanism-specialised
 * kernel -- one state per lane, generated from the mechanism and compiled with hipRTC at first use
 * -- for batches of >= 16384 states when the mechanism has no PLOG / chemically activated
 * reactions, else the generic reaction-per-lane kernel), 1 = generic kernel, 2 = specialised kernel
 * (error if it is unavailable).  ckmi_rop_jit_state: 0 not compiled yet, 1 ready, -1 unavailable
 * (ckmi_last_error() then says why). */
int ckmi_set_rop_path(int32_t path);
int ckmi_rop_jit_state(const ckmi_mech* mech, int32_t* state);
/* The generated source of the specialised kernel (len = its length; copied into buf when given) and
 * a compile-only check (hipRTC, no GPU needed; code_bytes = size of the gfx950 code object). */
int ckmi_rop_jit_source(const ckmi_mech_desc* desc, char* buf, int64_t cap, int64_t* len);
int ckmi_rop_jit_compile(const ckmi_mech_desc* desc, int64_t* code_bytes);

/* Batched forward/reverse rates of progress: qf[II][n], qr[II][n] mol/cm3-s. */
int ckmi_reaction_rates(const ckmi_mech* mech, int32_t n, const double* T, const double* P, const double* Y,
                        double* qf, double* qr, void* stream);

/* Batched closed homogeneous reactors.
 *   problem[n]   1 CONP (given pressure), 2 CONV (given volume), 3 plug flow (PFR: the integration
 *                variable is the distance x [cm]; t_end / t_save / profiles / tau are in cm; V0 is the
 *                inlet velocity [cm/s] and Vend the outlet velocity; constant flow area; the pressure
 *                from the inviscid momentum equation P + rho u^2 = P0 + rho0 u0^2, or the PPRO
 *                profile in x; replaces KINAll0D_SetupPFRInputs + KINAll0D_Calculate,
 *                chemkin_wrapper.py / flowreactors/PFR.py:498-512.  Wall heat-loss fields are not
 *                applied to plug-flow reactors; the front ends reject them.),
 *                4 single-zone IC engine (closed, V(t) from the slider-crank of cfg->eng, V0 ignored;
 *                ICHX / Woschni wall heat transfer replaces QLOS / HTC; KK + 1 <= 64 only;
 *                replaces KINAll0D_SetupHCCIInputs + KINAll0D_Calculate, engines/HCCI.py:1105-1239)
 *   T0, P0, V0   [n] initial temperature [K], pressure [dyn/cm2], volume [cm3]
 *   Y0           [n][KK] initial mass fractions (reactor-major)
 *   tau          [n] ignition delay [s] (-1 if not detected)
 *   Tend, Pend, Vend [n], Yend [n][KK] final state (at t_end, or at the stop time)
 *   stats        [n][CKMI_NSTAT] int32
 *   nsave, t_save[nsave] (device) and y_save [n][nsave][KK+1] (T, Y) optional (nsave = 0)
 */
int ckmi_reactor_run(const ckmi_mech* mech, const ckmi_reactor_cfg* cfg, int32_t n, const int32_t* problem,
                     const double* T0, const double* P0, const double* V0, const double* Y0, double* tau,
                     double* Tend, double* Pend, double* Vend, double* Yend, int32_t* stats, int32_t nsave,
                     const double* t_save, double* y_save, void* stream);

/* ckmi_reactor_run plus the optional per-reactor inputs / outputs of `ext` (NULL = none):
 * the batched form of the reference's A-factor sensitivity loop and of adaptive saving. */
int ckmi_reactor_run_ex(const ckmi_mech* mech, const ckmi_reactor_cfg* cfg, int32_t n, const int32_t* problem,
                        const double* T0, const double* P0, const double* V0, const double* Y0,
                        const ckmi_reactor_ext* ext, double* tau, double* Tend, double* Pend, double* Vend,
                        double* Yend, int32_t* stats, int32_t nsave, const double* t_save, double* y_save,
                        void* stream);

/* Batched perfectly stirred reactors (steady-state PSR, gas only, one effective inlet; the reference's
 * stirreactors/PSR.py run one at a time).  Each reactor marches the open-reactor equations at constant
 * pressure from its estimate until they are steady:
 *   dY_k/dt  = (Y_k,in - Y_k) / tau + wdot_k W_k / rho
 *   cp dT/dt = (H_in - sum_k Y_k,in h_k(T)) / tau - sum_k h_k wdot_k W_k / rho - Q / (rho V)    (energy = 1)
 *   dT/dt    = 0, T = Tguess                                                                    (energy = 2)
 * with rho = P Wbar / (R T), H_in = sum_k Y_k,in h_k(T_in) and Q = QLOS + HTC AREAQ (T - TAMB) from cfg
 * (cal units as for the closed reactors).  mode 1: tau = tau_or_vol is given and V = tau mdot / rho;
 * mode 2: V = tau_or_vol is given and tau = rho V / mdot follows the state.
 * A state is steady when a fresh right-hand side f satisfies tau |f_k| <= ss_rtol |Y_k| + ss_atol for
 * every species and tau |f_T| <= ss_rtol T.  The run ends at the first steady state (status CKMI_RUN_OK) or
 * at t_max = cfg->t_end (0: 1000 tau) with CKMI_RUN_NOT_STEADY.  cfg->rtol / atol are the time integrator's
 * tolerances; ignition detection, profiles and adaptive saving do not apply (CKMI_ERR_ARG).
 * The result is the steady state the transient reaches FROM THE ESTIMATE: where a PSR has an ignited and an
 * extinguished branch, a burnt estimate stays ignited and an unburnt one may blow out, whereas a damped
 * Newton solver (Chemkin's TWOPNT) can land on either branch from the same estimate.
 * KK + 1 <= 64 only (CKMI_ERR_UNSUPPORTED above).  All arrays are device pointers:
 *   P, Tin, mdot, tau_or_vol, Tguess [n]; Yin, Yguess [n][KK]           inputs (dyn/cm2, K, g/s, s or cm3)
 *   Tss [n], Yss [n][KK], rho [n] g/cm3, tau_res [n] s, vol [n] cm3     the returned state
 *   resid [n]    the largest scaled residual of the rule at it (<= 1: steady)
 *   stats [n][CKMI_NSTAT] */
typedef struct {
  int32_t mode; /* 1 residence time given, 2 volume given */
  double ss_rtol, ss_atol;
} ckmi_psr_cfg;
int ckmi_psr_run(const ckmi_mech* mech, const ckmi_reactor_cfg* cfg, const ckmi_psr_cfg* psr, int32_t n,
                 const double* P, const double* Tin, const double* Yin, const double* mdot,
                 const double* tau_or_vol, const double* Tguess, const double* Yguess, double* Tss, double* Yss,
                 double* rho, double* tau_res, double* vol, double* resid, int32_t* stats, void* stream);

/* Batched networks of steady-state PSRs with recycle streams (the reference's hybridreactornetwork.ReactorNetwork,
 * one network and one reactor at a time there).  n_net independent networks of R reactors each, solved by
 * Gauss-Seidel sweeps in the order given: for position i = 0..R-1 the effective inlet of reactor i
 * is mixed by mass and enthalpy from its external inlets and from the upstream solutions present (a mixing kernel,
 * one wave per network), ckmi_psr_run solves that position of every active network in one launch, and a tear kernel
 * ends the sweep.  Through-flows come once from the linear balance (I - F^T) mdot = mdot_ext.  A feed-forward
 * network (no split entry j -> i with j >= i) takes exactly one sweep; the others sweep until the change of every
 * tear-point reactor between two sweeps satisfies |dT| <= tear_rtol T and |dY_k| <= tear_atol + tear_rtol |Y_k|
 * (all of them, not any of them as the reference tests), or max_sweeps is reached.  A network that declares no
 * tear point but has recycle is tested at every reactor.  Networks that are done leave the active list (rebuilt in
 * network order after every sweep) and are not integrated again; a network's result does not depend on the rest of
 * the batch.  R <= CKMI_NET_RMAX and KK + 1 <= 64 (CKMI_ERR_UNSUPPORTED above); E >= 1.
 * cfg[R], psr[R] and guess_mode[R] are HOST arrays, one entry per position; everything else is a device pointer:
 *   P [n_net][R] dyn/cm2; tau_or_vol [n_net][R] s or cm3 by psr[i].mode
 *   split [n_net][R][R+1]      mass fraction of reactor j's outflow that enters reactor i; column R leaves the network
 *   ext_mdot, ext_T [n_net][R][E], ext_Y [n_net][R][E][KK]   external inlets in E padded slots (mdot = 0: unused)
 *   Tguess [n_net][R], Yguess [n_net][R][KK]; guess_mode[i] 0: the estimate as given, 1: Tguess with the effective
 *                              inlet's composition (reset_estimate_composition(inlet.X)); later sweeps start from the
 *                              reactor's previous solution
 *   tear [n_net][R] int32      1: a tear point
 *   Tss, mdot, rho, tau_res, vol, resid [n_net][R], Yss [n_net][R][KK], stats [n_net][R][CKMI_NSTAT]   per reactor
 *                              (mdot: the through-flow g/s)
 *   net_stats [n_net][CKMI_NET_NSTAT] int32, tear_resid [n_net]   per network: status, sweeps taken, flags, and the
 *                              last scaled tear residual (<= 1: converged; 0 for a feed-forward network)
 * The call synchronises the stream once per sweep (a 4-byte count of active networks sizes the next launches). */
typedef struct {
  int32_t max_sweeps;          /* 0 = 200 */
  double tear_rtol, tear_atol; /* 0 = 1e-6, 1e-8 */
  double relax;                /* new = old + relax (new - old) after every sweep but the first; 0 = 1 */
} ckmi_network_cfg;
#define CKMI_NET_RMAX 16
#define CKMI_NET_STAT_STATUS 0
#define CKMI_NET_STAT_SWEEPS 1
#define CKMI_NET_STAT_FLAGS 2 /* bit 0: feed-forward, bit 1: no tear point declared, every reactor is tested */
#define CKMI_NET_NSTAT 4
#define CKMI_NET_OK 0
#define CKMI_NET_TEAR_LIMIT 10      /* max_sweeps reached (the reference's code) */
#define CKMI_NET_REACTOR_FAILED 11  /* a member's stats say which reactor and why; the network stops there */
#define CKMI_NET_FLOW_SINGULAR 12   /* the flow balance has no solution (a closed loop with no exit) or leaves a
                                       reactor without through-flow; the network is never integrated (outputs NaN) */
int ckmi_psr_network_run(const ckmi_mech* mech, int32_t n_net, int32_t R, int32_t E, const ckmi_reactor_cfg* cfg,
                         const ckmi_psr_cfg* psr, const ckmi_network_cfg* net, const int32_t* guess_mode,
                         const double* P, const double* split, const double* ext_mdot, const double* ext_T,
                         const double* ext_Y, const double* tau_or_vol, const double* Tguess, const double* Yguess,
                         const int32_t* tear, double* Tss, double* Yss, double* mdot, double* rho, double* tau_res,
                         double* vol, double* resid, int32_t* stats, int32_t* net_stats, double* tear_resid,
                         void* stream);

/* Batched gas-phase chemical equilibrium and Chapman-Jouguet detonation states (ideal gas, element
 * potentials; replaces KINCalculateEquil / KINCalculateEquilWithOption / KINCalculateEqGasWithOption,
 * chemkin_wrapper.py:513-541, mixture.py:3574-3961, one state per call there).  n independent states per
 * launch, one option per state (mixture.py:3604-3617):
 *   1 T and P    2 T and V    3 T and S    4 P and V    5 P and H
 *   6 P and S    7 V and U    8 V and H    9 V and S   10 Chapman-Jouguet detonation
 * held at the values of the given state (T, P, Y).  Per gram of mixture the unknowns are ln n_j, ln n, ln T
 * and ln P; every option is the same damped Newton iteration on the reduced (MM + 3)-row system of the element
 * balances, the total-moles row and the option's two rows, cold-started.  A state has
 * converged at an undamped step whose relative corrections are all <= tol.  Option 10 holds V and the Hugoniot
 * H - (P - P1)(V1 + V) / 2 = H1 of the given state and finds the V / V1 in [cj_vlo, cj_vhi] of the least
 * detonation speed D = V1 sqrt((P - P1) / (V1 - V)) by a bracketed secant iteration inside the kernel, from
 * cj_start, until V / V1 moves by <= cj_tol; at most cj_iter Hugoniot points.
 * Works for any species count; needs the element counts (desc.ncf) of at most CKMI_PROJ_MMAX elements
 * (CKMI_ERR_UNSUPPORTED otherwise).  A zero cfg field selects its default.  All arrays are device pointers:
 *   option [n] int32; T [n] K, P [n] dyn/cm2, Y [n][KK] mass fractions          the given states
 *   Teq, Peq [n], Yeq [n][KK]                                                   the equilibrium states
 *   sound, detspeed [n]  cm/s: the burnt gas's sound speed D V2 / V1 (the CJ condition) and D; 0 for options 1-9
 *   stats [n][CKMI_EQ_NSTAT] int32
 * A state that does not converge within max_iter iterations (per Hugoniot point for option 10), a CJ minimum
 * on an end of the bracket, an option outside 1..10 or T, P <= 0 gets CKMI_RUN_EQ_NOT_CONVERGED and its last
 * iterate (the given state if it never started). */
typedef struct {
  double tol;       /* convergence tolerance, default 1e-12 */
  int32_t max_iter; /* Newton iteration cap, default 200 */
  double cj_vlo, cj_vhi; /* bracket of V / V1, default 0.30, 0.97 */
  double cj_start;  /* first V / V1, default 0.60 */
  double cj_tol;    /* default 1e-9 */
  int32_t cj_iter;  /* Hugoniot points at most, default 40 */
} ckmi_equil_cfg;
#define CKMI_EQ_STAT_ITER 0    /* Newton iterations (option 10: over all Hugoniot points) */
#define CKMI_EQ_STAT_STATUS 1  /* CKMI_RUN_OK or CKMI_RUN_EQ_NOT_CONVERGED */
#define CKMI_EQ_STAT_CJ_ITER 2 /* Hugoniot points solved (option 10) */
#define CKMI_EQ_NSTAT 4
#define CKMI_RUN_EQ_NOT_CONVERGED 7
int ckmi_equil_run(const ckmi_mech* mech, const ckmi_equil_cfg* cfg, int32_t n, const int32_t* option,
                   const double* T, const double* P, const double* Y, double* Teq, double* Peq, double* Yeq,
                   double* sound, double* detspeed, int32_t* stats, void* stream);

/* Heat rates of a single-zone engine run (problem 4) on its saved states, evaluated with the
 * integrator's own right-hand side: the output side of KINAll0D_GetEngineHeatRelease
 * (engine.py:953-988).  T0, P0 and Y0 [KK] (device) are the cylinder's initial state (they fix its
 * mass and the Woschni reference state); t [n] and y [n][KK+1] (T, Y; device) the saved states.
 *   ahrr[n]   apparent heat-release rate m c_v dT/dt + P dV/dt [erg/s] (chemical heat release net of
 *             the wall loss)
 *   qloss[n]  wall heat-loss rate h A (T - T_wall) [erg/s] (0 for an adiabatic engine)
 * Divide by 6 RPM for the rates per crank-angle degree. */
int ckmi_engine_heat_rates(const ckmi_mech* mech, const ckmi_reactor_cfg* cfg, double T0, double P0,
                           const double* Y0, int32_t n, const double* t, const double* y, double* ahrr,
                           double* qloss, void* stream);

/* Right-hand side and analytic Jacobian of the reactor kernels at given states.  A diagnostic for tests: it
 * evaluates the device functions the integrators are compiled from (reactor_rhs of the wave kernel, rhs_big of
 * the workgroup kernel) once per state, in probe kernels of their own; it does not run the integrators.
 *   problem [n]                       1..5 per state; problem 5 (open reactor) only for every state of a call
 *   T0, P0, V0 [n], Y0 [n][KK]        the reactor's initial state, which fixes its context (mass, plug-flow mass
 *                                     flux, the engine's reference state) as ckmi_reactor_run builds it; for
 *                                     problem 5: the estimate, the pressure and tau_or_vol as ckmi_psr_run takes them
 *   t [n], y [n][KK+1]                the evaluation points (T, Y_1..Y_KK); a profile is evaluated on the piece
 *                                     that contains t
 *   ext                               optional; only afac_rxn / afac are honoured
 *   psr                               the inlet of problem 5 (required there, ignored otherwise)
 *   f [n][KK+1]                       f(t, y)
 *   J [n][KK+1][KK+1]                 row-major, J[i][j] = d f_i / d y_j; NULL: the plain pass, f only.  The wave
 *                                     kernel's J is FP64; the workgroup kernel's comes back through the FP32 slot it
 *                                     parks its Jacobian in.  Plug flow: scaled by rho / G like f.
 * The kernel and its template parameters come from the chooser ckmi_reactor_run / ckmi_psr_run call (wave_plan /
 * big_plan of csrc/ckmi_dispatch.hpp, readable through ckmi_reactor_variant), on the mechanism, the problems,
 * cfg->rtol and ckmi_set_reactor_path.  CKMI_ERR_UNSUPPORTED: problem 4 or 5 with
 * KK + 1 > 64 (problem 4 also on the forced workgroup path); CKMI_ERR_SIZE: an image the workgroup kernel's LDS
 * does not hold; CKMI_ERR_ARG: a problem outside 1..5, n < 0, a missing array.  All arrays are device pointers;
 * the call synchronises the stream once (it reads problem[] on the host). */
typedef struct {
  int32_t mode;       /* 1 residence time given, 2 volume given (V0 holds tau_or_vol) */
  const double* Tin;  /* [n] K */
  const double* Yin;  /* [n][KK] */
  const double* mdot; /* [n] g/s */
} ckmi_rhs_psr;
int ckmi_reactor_rhs_jac(const ckmi_mech* mech, const ckmi_reactor_cfg* cfg, int32_t n, const int32_t* problem,
                         const double* T0, const double* P0, const double* V0, const double* Y0, const double* t,
                         const double* y, const ckmi_reactor_ext* ext, const ckmi_rhs_psr* psr, double* f, double* J,
                         void* stream);

/* Set-up and solves of the reactor kernels' Newton matrix M = I - gamma J on given matrices.  A diagnostic for
 * tests: probe kernels of their own call the member functions the integrators call (build_factor / solve of the
 * wave kernel's NewtonMatrixGJ64 and NewtonMatrixF32S, build / factor / solve of the workgroup kernel's BigMatrixM
 * and BigMatrix) on one matrix object per wave / workgroup; the integrators do not run, and no mechanism is needed.
 *   kernel, size, f32_stored          the matrix class: kernel 1 (wave) with size N = 32, 54 or 64 and the FP32-stored
 *                                     (1) or FP64 (0) inverse, no FP64 form at N = 32; kernel 2 (workgroup) with
 *                                     size NB = 4..12 (order 16 NB; NB <= 11 the MFMA form) and f32_stored = 0
 *   nsys, n                           systems and their order, 2 <= n <= N resp. 16 NB
 *   J [nsys][n][n], gamma [nsys]      J in FP32, row-major: what both kernels park
 *   J_prev, gamma_prev                optional (both or neither): a set-up made first on the same matrix object and
 *                                     the same LDS, as a refactorisation or the next reactor of the persistent loop
 *   nrhs, B [nsys][nrhs][n]           right-hand sides; b_pad: what a wave lane >= n hands to solve(), which zeroes
 *                                     it (kernel 2 takes 0 only: its solve's contract)
 *   X [nsys][nrhs][n]                 the solutions
 *   perm [nsys][n]                    the pivot row of step k
 *   ok [nsys]                         0 if a pivot's FP32 key was zero (X is then garbage), else 1
 * CKMI_ERR_ARG: a class that is not compiled, n outside its range, a missing array.  All arrays are device
 * pointers on the current device. */
int ckmi_newton_probe(int32_t kernel, int32_t size, int32_t f32_stored, int32_t nsys, int32_t n, const float* J,
                      const double* gamma, const float* J_prev, const double* gamma_prev, int32_t nrhs, const double* B,
                      double b_pad, double* X, int32_t* perm, int32_t* ok, void* stream);

/* Reactor kernel selection (diagnostic / testing): 0 = automatic (one wave per reactor for KK + 1 <= 64,
 * its Newton inverse stored in FP32 unless rtol < 1e-9; one 4-wave workgroup per reactor above, up to
 * KK + 1 = 192), 1 = the workgroup-per-reactor kernel for every mechanism (lets tests run both
 * integrators on the same GRI-3.0 reactors), 2 / 3 = the wave kernel with the FP64 / FP32-stored
 * Newton inverse whatever the tolerances.  Process-wide. */
int ckmi_set_reactor_path(int32_t path);

/* Host-only capacity query of the workgroup-per-reactor kernel (no GPU needed): the largest mechanism
 * image in bytes (MechImage, staged in LDS) it accepts for nvar = KK + 1 state variables, KKp padded
 * species and G third-body groups on a CU with lds_max bytes of LDS; -1 if none fits.  A mechanism
 * whose image is larger gets CKMI_ERR_SIZE from ckmi_reactor_run. */
int ckmi_big_max_image_bytes(int32_t nvar, int32_t KKp, int32_t G, int32_t lds_max);

/* Host-only query of the variant chooser (no GPU needed, no state read or written): the compiled variant
 * ckmi_reactor_run (open_reactor = 0) or ckmi_psr_run (open_reactor = 1) and the probes of
 * ckmi_reactor_rhs_jac launch for nvar = KK + 1 state variables, a mechanism with / without PLOG-class
 * (has_plog) and FORD / RORD / fractional-order (has_general) reactions, cfg->rtol and the
 * ckmi_set_reactor_path value path.
 *   out[0]  1: the wave-per-reactor kernel, 2: the workgroup-per-reactor kernel
 *   wave:      out[1] N of the FP32-inverse launch (0: none), out[2] N of the FP64-inverse launch, out[3] PL,
 *              out[4] what the FP64-inverse launch takes: 0 every reactor, 1 plug flow and engines only,
 *              2 those and the reactors the FP32-inverse launch failed on
 *   workgroup: out[1] NB, out[3] PL, the rest 0
 * CKMI_ERR_UNSUPPORTED as the run: nvar > 192, or an open reactor with nvar > 64; CKMI_ERR_ARG: nvar < 2, a path
 * outside 0..3 or out = NULL. */
int ckmi_reactor_variant(int32_t nvar, int32_t has_plog, int32_t has_general, double rtol, int32_t path,
                         int32_t open_reactor, int32_t out[5]);

/* Batched dense LU of Newton iteration matrices too large for one wave (mechanisms with more
 * than 63 species).  Replaces the factorisation inside the reference's
 * KINAll0D_Calculate (batchreactor.py:1158), which has no public entry point of its own.
 *   A     [nsys][n][n] row-major FP64 (device), overwritten by L (unit lower) and U
 *   ipiv  [nsys][n] 0-based pivot rows, LAPACK dgetrf order (row i was swapped with ipiv[i])
 *   info  [nsys] 0, or k + 1 if U(k, k) is exactly zero (dgetrf convention)
 * One workgroup per matrix; the trailing updates run on v_mfma_f64_16x16x4_f64.  n <= 192. */
#define CKMI_LU_NMAX 192
int ckmi_lu_factor_batched(int32_t nsys, int32_t n, double* A, int32_t* ipiv, int32_t* info, void* stream);
/* B[nsys][n] <- A^-1 B from the factors of ckmi_lu_factor_batched (dgetrs, one right-hand side). */
int ckmi_lu_solve_batched(int32_t nsys, int32_t n, const double* LU, const int32_t* ipiv, double* B,
                          void* stream);
const char* ckmi_lu_last_error(void);

/* Viscosity: replaces KINGetViscosity (chemkin_wrapper.py:407-412) and
 * KINGetMixtureViscosity (:442-448), evaluated by the reference's closed library from the
 * transport file preprocessed by KINPreProcess (itran = 1, chemistry.py:636-687).
 *   ckmi_transport_fit      host only: params [KK][6] = geometry, eps/k [K], sigma [A], dipole [D],
 *                           polarizability [A^3], Zrot (TRANLIB columns) -> fits [KK][4], the
 *                           coefficients of ln eta_k [g/(cm s)] as a cubic in ln T, least squares
 *                           on 50 temperatures in [tlow, thigh]
 *   ckmi_transport_create   uploads the fits and the Wilke tables onto the mechanism's device
 *   ckmi_species_viscosity  T [n] -> eta [KK][n]                          (device pointers)
 *   ckmi_mixture_viscosity  T [n], Y [KK][n] mass fractions -> eta [n]    (device pointers, Wilke) */
typedef struct ckmi_transport ckmi_transport;
/* fit interval of KINPreProcess (and of pychemkin_amd/transport.py) */
#define CKMI_VISC_FIT_TLOW 300.0
#define CKMI_VISC_FIT_THIGH 3500.0
int ckmi_transport_fit(int32_t KK, const double* wt, const double* params, double tlow, double thigh, double* fits);
/* Thermal conductivity fits (host only; the engine's wall heat transfer, problem 4): lambda_k
 * [erg/(cm s K)] by the Warnatz form of TRANFIT (eta_k, the self-diffusion rho D_kk / eta_k, Zrot with
 * Parker's correction, Cv from the NASA-7 thermo [KK][17] of ckmi_mech_desc) -> fits [KK][4] of
 * ln lambda_k as a cubic in ln T on the same grid as ckmi_transport_fit. */
int ckmi_conductivity_fit(int32_t KK, const double* wt, const double* params, const double* thermo, double tlow,
                          double thigh, double* fits);
int ckmi_transport_create(const ckmi_mech* mech, const double* fits, ckmi_transport** out);
/* Thermal conductivity: replaces KINGetConductivity (chemkin_wrapper.py:413-418, mixture.py:1885-1909,
 * chemistry.py:1361-1396) and KINGetMixtureConductivity (:449-455, mixture.py:1979-2013).
 *   ckmi_transport_set_conductivity  uploads ckmi_conductivity_fit's [KK][4] fits beside the viscosity tables
 *   ckmi_species_conductivity        T [n] -> lambda [KK][n] erg/(cm s K)                  (device pointers)
 *   ckmi_mixture_conductivity        T [n], Y [KK][n] mass fractions -> lambda [n], mixture-averaged
 *                                    (sum X lambda + 1 / sum X / lambda) / 2                 (device pointers) */
int ckmi_transport_set_conductivity(ckmi_transport* tr, const double* cfits);
int ckmi_species_conductivity(const ckmi_transport* tr, int32_t n, const double* T, double* cond, void* stream);
int ckmi_mixture_conductivity(const ckmi_transport* tr, int32_t n, const double* T, const double* Y, double* cond,
                              void* stream);
int ckmi_transport_destroy(ckmi_transport* tr);
int ckmi_transport_fits(const ckmi_transport* tr, double* fits);
int ckmi_species_viscosity(const ckmi_transport* tr, int32_t n, const double* T, double* visc, void* stream);
int ckmi_mixture_viscosity(const ckmi_transport* tr, int32_t n, const double* T, const double* Y, double* visc,
                           void* stream);
/* Diffusion coefficients: replaces KINGetDiffusionCoeffs (chemkin_wrapper.py:419-425, chemistry.py:1410-1470,
 * mixture.py:1910), KINGetMixtureDiffusionCoeffs (:456-462, mixture.py:2015) and KINGetOrdinaryDiffusionCoeffs
 * (:464-470, mixture.py:2066).  All results in cm^2/s; P in dyn/cm^2.
 *   ckmi_diffusion_fit             host only: params [KK][6] as for ckmi_transport_fit -> dfits [KK][KK][4], the
 *                                  coefficients of ln D_jk at 1 atm as a cubic in ln T (Chapman-Enskog with
 *                                  Omega11* by Neufeld + 0.19 delta*^2 / T*, TRANLIB's combination rules with the
 *                                  polar-nonpolar induction correction), same grid and least squares as
 *                                  ckmi_transport_fit; symmetric in j and k
 *   ckmi_transport_set_diffusion   uploads that table beside the viscosity tables; without it the three
 *                                  functions below return CKMI_ERR_ARG
 *   ckmi_binary_diffusion          T [n], P [n] -> D [n][KK][KK], D_jk = exp(cubic) 1 atm / P   (device pointers)
 *   ckmi_mixture_diffusion         T [n], P [n], Y [KK][n] mass fractions -> D [KK][n], mixture-averaged
 *                                  D_km = sum_{j != k} X_j W_j / (Wbar sum_{j != k} X_j / D_jk) with
 *                                  X = (X+ + 1e-12) / sum (X+ + 1e-12), X+ from max(Y, 0)
 *   ckmi_multicomponent_diffusion  same inputs -> D [n][KK][KK], the ordinary multicomponent coefficients
 *                                  (Dixon-Lewis first order, TRANLIB MCMDIF: D_ij = X_i 16 T / (25 P) Wbar / W_j
 *                                  (p_ij - p_ii), p = L^-1 by partial pivoting, D_ii = 0); info [n] is 0, or
 *                                  k + 1 when the k-th pivot is exactly zero (dgetrf convention).  One wave per
 *                                  state for KK <= 64, ckmi_lu_factor_batched per state up to KK = CKMI_LU_NMAX
 *                                  (that path allocates a workspace of at most 256 MB and synchronises the stream
 *                                  before it returns), CKMI_ERR_UNSUPPORTED above.
 * An empty batch (n = 0) is a no-op. */
int ckmi_diffusion_fit(int32_t KK, const double* wt, const double* params, double tlow, double thigh, double* dfits);
int ckmi_transport_set_diffusion(ckmi_transport* tr, const double* dfits);
int ckmi_binary_diffusion(const ckmi_transport* tr, int32_t n, const double* T, const double* P, double* D,
                          void* stream);
int ckmi_mixture_diffusion(const ckmi_transport* tr, int32_t n, const double* T, const double* P, const double* Y,
                           double* D, void* stream);
int ckmi_multicomponent_diffusion(const ckmi_transport* tr, int32_t n, const double* T, const double* P,
                                  const double* Y, double* D, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
