/* ckoracle.c -- CPU ORACLE (test infrastructure only; see ckoracle.h).
 *
 * Chemistry: standard Chemkin-II gas kinetics (the closed libKINetics.so is not in the
 * reference; its call sites are chemkin_wrapper.py:375-498 and mixture.py:1442,1551).
 * Integrator: CVODE-style variable-order (1..5) variable-step BDF in Nordsieck form with a
 * modified Newton corrector and dense partial-pivot LU, i.e. the DASPK/DASSL-class method
 * family the reference's KINAll0D_Calculate uses.  Ignition
 * definitions follow ChemkinKeywordTips.yaml:184-199 (TIFP, DTIGN, TLIM, KLIM) and the
 * defaults of batchreactor.py:91-92,296.
 */
#include "ckoracle.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define BOLTZMANN 1.3806504e-16
#define AVOGADRO 6.02214179e23
#define RU (BOLTZMANN * AVOGADRO)
#define PATM 1.01325e6
#define NMAX 512

/* ------------------------------------------------------------------ thermo */
void cko_thermo(const cko_mech* m, double T, double* cp_R, double* h_RT, double* s_R) {
  const double lnT = log(T), T2 = T * T, T3 = T2 * T, T4 = T3 * T;
  for (int k = 0; k < m->KK; ++k) {
    const double* th = m->thermo + 17 * k;
    const double* a = (T > th[1]) ? th + 10 : th + 3;
    if (cp_R) cp_R[k] = a[0] + a[1] * T + a[2] * T2 + a[3] * T3 + a[4] * T4;
    if (h_RT) h_RT[k] = a[0] + a[1] * T / 2 + a[2] * T2 / 3 + a[3] * T3 / 4 + a[4] * T4 / 5 + a[5] / T;
    if (s_R) s_R[k] = a[0] * lnT + a[1] * T + a[2] * T2 / 2 + a[3] * T3 / 3 + a[4] * T4 / 4 + a[6];
  }
}

/* C^o for a reaction order o (stoichiometric coefficient, or FORD / RORD) -- one rule on every
 * implementation (oracle/numpy_ref.py _cpow, pychemkin_amd/csrc/ckmi_image.hpp conc_pow):
 *   o in {0, 1, 2, 3}: exact products;
 *   0 < o < 1 (non-integral): C^o for C >= CFLOOR, and the chord CFLOOR^(o-1) C below it (negative
 *     concentrations included), so the rate is Lipschitz at C = 0.  Without this the rate of a species
 *     that runs out is non-Lipschitz there (d C^o/dC unbounded, flat for C <= 0): the BDF corrector
 *     then settles into a period-2 cycle at C ~ 0 with the step size locked, and at some tolerances
 *     the integration hits max steps (case 1 of tests/test_ford.py at rtol 0.97e-8).
 *     The chord changes the rate only below 1e-14 mol/cm3 (this implementation's choice: the
 *     reference holds no FORD golden, parity unpinned).  A Jacobian-only fix does not do it: with
 *     the rate left flat for C <= 0, a floored or chord-slope derivative still stalls (measured);
 *     with the Lipschitz rate, the plain derivative of it is robust;
 *   any other o: pow(C, o) for C > 0 and 0 for C <= 0. */
#define CFLOOR 1e-14
static double conc_pow(double c, double o) {
  if (o == 0.0) return 1.0;
  if (o == 1.0) return c;
  if (o == 2.0) return c * c;
  if (o == 3.0) return c * c * c;
  if (o < 1.0 && c < CFLOOR) return pow(CFLOOR, o - 1.0) * c;
  return c > 0.0 ? pow(c, o) : 0.0;
}
/* d C^o / dC of that rule (the Jacobian): the tangent o C^(o-1) above CFLOOR, the chord's slope
 * CFLOOR^(o-1) below it -- the exact derivative of the Lipschitz rate */
static double dconc_pow(double c, double o) {
  if (o == 0.0) return 0.0;
  if (o == 1.0) return 1.0;
  if (o == 2.0) return 2.0 * c;
  if (o == 3.0) return 3.0 * c * c;
  if (o < 1.0) return c < CFLOOR ? pow(CFLOOR, o - 1.0) : o * pow(c, o - 1.0);
  return c > 0.0 ? o * pow(c, o - 1.0) : 0.0;
}
/* order of reactant slot s / product slot s of reaction i */
static double ford_of(const cko_mech* m, int i, int s) {
  return m->ford ? m->ford[CKO_SLOTS * i + s] : m->rnu[CKO_SLOTS * i + s];
}
static double rord_of(const cko_mech* m, int i, int s) {
  return m->rord ? m->rord[CKO_SLOTS * i + s] : m->pnu[CKO_SLOTS * i + s];
}

/* Per-reaction kinetics at (T, C[]).  Returns kf_eff (incl. falloff), kr_eff, the
 * third-body factor (1 if none), Pi_f, Pi_r, and d ln kf / dT, d ln kr / dT. */
typedef struct {
  double kf, kr, mfac, pf, pr, dlkf, dlkr;
} rxn_eval;

/* PLOG (Chemkin "PLOG /P A b E/"): ln k interpolated linearly in ln P between the two bracketing
 * pressures, clamped to the end points outside the table; d ln k / dT interpolated alike. */
static void plog_rate(const cko_mech* m, int i, double lnP, double lnT, double invT, double* lnk, double* dlk) {
  const int p0 = m->plog_ptr[i], n = m->plog_ptr[i + 1] - p0;
  const double* t = m->plog_par + 4 * p0;
  int j = 0;
  while (j < n - 2 && lnP > t[4 * (j + 1)]) ++j;
  const double lk0 = t[4 * j + 1] + t[4 * j + 2] * lnT - t[4 * j + 3] * invT;
  const double dk0 = (t[4 * j + 2] + t[4 * j + 3] * invT) * invT;
  if (n == 1) {
    *lnk = lk0;
    *dlk = dk0;
    return;
  }
  const double* u = t + 4 * (j + 1);
  const double lk1 = u[1] + u[2] * lnT - u[3] * invT;
  const double dk1 = (u[2] + u[3] * invT) * invT;
  double w = (lnP - t[4 * j]) / (u[0] - t[4 * j]);
  w = w < 0.0 ? 0.0 : (w > 1.0 ? 1.0 : w);
  *lnk = lk0 + w * (lk1 - lk0);
  *dlk = dk0 + w * (dk1 - dk0);
}

/* Chebyshev rate (CKMI_RXN_CHEB, include/ckmi.h): log10 k = sum_t sum_p a[t][p] T_t(Tr) T_p(Pr) with
 * the reduced inverse temperature and log pressure; d ln k / dT through dTr/dT.  Rows of plog_par:
 * (NT, NP), (Tmin, Tmax, Pmin, Pmax [atm]), then a[t][p] t-major.  No clamping outside the range. */
static void cheb_rate(const cko_mech* m, int i, double P, double invT, double* lnk, double* dlk) {
  const double* r = m->plog_par + 4 * m->plog_ptr[i];
  const int nt = (int)r[0], np = (int)r[1];
  const double iTmin = 1.0 / r[4], iTmax = 1.0 / r[5];
  const double lPmin = log10(r[6] * PATM), lPmax = log10(r[7] * PATM);
  const double Tr = (2.0 * invT - iTmin - iTmax) / (iTmax - iTmin);
  const double Pr = (2.0 * log10(P) - lPmin - lPmax) / (lPmax - lPmin);
  const double* a = r + 8;
  double tp[16], tt[16], dt[16], lk = 0.0, dl = 0.0;
  tp[0] = 1.0, tt[0] = 1.0, dt[0] = 0.0;
  tp[1] = Pr, tt[1] = Tr, dt[1] = 1.0;
  for (int p = 2; p < np; ++p) tp[p] = 2.0 * Pr * tp[p - 1] - tp[p - 2];
  for (int t = 2; t < nt; ++t) {
    tt[t] = 2.0 * Tr * tt[t - 1] - tt[t - 2];
    dt[t] = 2.0 * tt[t - 1] + 2.0 * Tr * dt[t - 1] - dt[t - 2];
  }
  for (int t = 0; t < nt; ++t) {
    double row = 0.0;
    for (int p = 0; p < np; ++p) row += a[t * np + p] * tp[p];
    lk += tt[t] * row;
    dl += dt[t] * row;
  }
  const double LN10 = 2.302585092994046;
  *lnk = lk * LN10;
  *dlk = dl * LN10 * (-2.0 * invT * invT / (iTmax - iTmin));
}

static void eval_reaction(const cko_mech* m, int i, double T, double lnT, double invT, double lnPRT, double P,
                          const double* C, double Ctot, const double* g_RT, const double* h_RT, double dlnA,
                          double gfac, rxn_eval* e) {
  const double* a = m->arr + 3 * i;
  double kf, dlkf;
  double mfac = 1.0;
  const int type = m->rtype[i];
  double t13 = 0.0, t23 = 0.0; /* Landau-Teller T^(-1/3), T^(-2/3) */
  if (type == 3 || type == 5) {
    double lnk;
    if (type == 3) plog_rate(m, i, log(P), lnT, invT, &lnk, &dlkf);
    else cheb_rate(m, i, P, invT, &lnk, &dlkf);
    kf = exp(lnk + dlnA);
  } else if (type == 6) {
    const double* lt = m->low + 3 * i;
    t13 = exp(-lnT / 3.0);
    t23 = t13 * t13;
    kf = exp(a[0] + dlnA + a[1] * lnT - a[2] * invT + lt[0] * t13 + lt[1] * t23);
    dlkf = (a[1] + a[2] * invT - (lt[0] * t13 + 2.0 * lt[1] * t23) / 3.0) * invT;
  } else {
    kf = exp(a[0] + dlnA + a[1] * lnT - a[2] * invT);
    dlkf = (a[1] + a[2] * invT) * invT;
  }
  if (type == 1 || type == 2 || type == 4) {
    double M;
    if (m->tbsp[i] >= 0) {
      M = C[m->tbsp[i]];
    } else {
      M = Ctot;
      for (int p = m->eff_ptr[i]; p < m->eff_ptr[i + 1]; ++p) M += (m->eff_val[p] - 1.0) * C[m->eff_sp[p]];
    }
    if (type == 1) {
      mfac = M;
    } else {
      const double* l = m->low + 3 * i;
      /* falloff: main = k_inf, l = LOW; chemically activated (4): main = k0, l = HIGH */
      double k0 = exp(l[0] + l[1] * lnT - l[2] * invT);
      double Pr = type == 4 ? kf * M / k0 : k0 * M / kf;
      double F = 1.0;
      const int ft = m->ftype[i];
      const double* fp = m->fpar + 5 * i;
      if (ft == 2 || ft == 3) {
        double Fcent = (1.0 - fp[0]) * exp(-T / fp[1]) + fp[0] * exp(-T / fp[2]);
        if (ft == 3) Fcent += exp(-fp[3] * invT);
        double lFc = log10(Fcent > 1e-300 ? Fcent : 1e-300);
        double lPr = log10(Pr > 1e-300 ? Pr : 1e-300);
        double c = -0.4 - 0.67 * lFc, nn = 0.75 - 1.27 * lFc;
        double f1 = (lPr + c) / (nn - 0.14 * (lPr + c));
        F = pow(10.0, lFc / (1.0 + f1 * f1));
      } else if (ft == 4) {
        double lPr = log10(Pr > 1e-300 ? Pr : 1e-300);
        double X = 1.0 / (1.0 + lPr * lPr);
        F = fp[3] * pow(fp[0] * exp(-fp[1] * invT) + exp(-T / fp[2]), X) * pow(T, fp[4]);
      }
      kf = type == 4 ? kf * (1.0 / (1.0 + Pr)) * F : kf * (Pr / (1.0 + Pr)) * F;
    }
  }
  double kr = 0.0, dlkr = 0.0;
  if (m->rev[i]) {
    if (m->has_rev[i]) {
      const double* r = m->revp + 3 * i;
      if (type == 6) { /* RLT terms of the explicit reverse rate */
        const double* rl = m->fpar + 5 * i;
        kr = exp(r[0] + r[1] * lnT - r[2] * invT + rl[0] * t13 + rl[1] * t23);
        dlkr = (r[1] + r[2] * invT - (rl[0] * t13 + 2.0 * rl[1] * t23) / 3.0) * invT;
      } else {
        kr = exp(r[0] + r[1] * lnT - r[2] * invT);
        if (type == 2 || type == 4) kr *= kf / exp(a[0] + dlnA + a[1] * lnT - a[2] * invT);
        dlkr = (r[1] + r[2] * invT) * invT;
      }
    } else {
      double dG = 0.0, dH = 0.0, dnu = 0.0;
      for (int s = 0; s < m->nr[i]; ++s) {
        int k = m->rsp[CKO_SLOTS * i + s];
        double nu = m->rnu[CKO_SLOTS * i + s];
        dG -= nu * g_RT[k]; dH -= nu * h_RT[k]; dnu -= nu;
      }
      for (int s = 0; s < m->np[i]; ++s) {
        int k = m->psp[CKO_SLOTS * i + s];
        double nu = m->pnu[CKO_SLOTS * i + s];
        dG += nu * g_RT[k]; dH += nu * h_RT[k]; dnu += nu;
      }
      /* Kc = exp(-dG) (PATM/RT)^dnu ; kr = kf / Kc */
      kr = kf * exp(dG - dnu * lnPRT);
      dlkr = dlkf - (dH - dnu) * invT;
    }
  }
  double pf = 1.0, pr = 1.0;
  for (int s = 0; s < m->nr[i]; ++s) pf *= conc_pow(C[m->rsp[CKO_SLOTS * i + s]], ford_of(m, i, s));
  for (int s = 0; s < m->np[i]; ++s) pr *= conc_pow(C[m->psp[CKO_SLOTS * i + s]], rord_of(m, i, s));
  /* GFAC scales forward and reverse rates alike */
  e->kf = kf * gfac; e->kr = kr * gfac; e->mfac = mfac; e->pf = pf; e->pr = pr; e->dlkf = dlkf; e->dlkr = dlkr;
}

static void conc_from_Y(const cko_mech* m, double rho, const double* Y, int nneg, double* C, double* Ctot) {
  double s = 0.0;
  for (int k = 0; k < m->KK; ++k) {
    double y = Y[k];
    if (nneg && y < 0.0) y = 0.0;
    C[k] = rho * y / m->wt[k];
    s += C[k];
  }
  *Ctot = s;
}

static double mean_wt(const cko_mech* m, const double* Y) {
  double s = 0.0;
  for (int k = 0; k < m->KK; ++k) s += Y[k] / m->wt[k];
  return 1.0 / s;
}

void cko_rates(const cko_mech* m, double T, double P, const double* Y, double* qf, double* qr, double* wdot) {
  const int KK = m->KK;
  double C[NMAX], h_RT[NMAX], s_R[NMAX], g_RT[NMAX], Ctot;
  double rho = P * mean_wt(m, Y) / (RU * T);
  conc_from_Y(m, rho, Y, 0, C, &Ctot);
  cko_thermo(m, T, NULL, h_RT, s_R);
  for (int k = 0; k < KK; ++k) g_RT[k] = h_RT[k] - s_R[k];
  if (wdot) memset(wdot, 0, sizeof(double) * KK);
  const double lnT = log(T), invT = 1.0 / T, lnPRT = log(PATM / (RU * T));
  for (int i = 0; i < m->II; ++i) {
    rxn_eval e;
    eval_reaction(m, i, T, lnT, invT, lnPRT, P, C, Ctot, g_RT, h_RT, 0.0, 1.0, &e);
    double f = e.mfac * e.kf * e.pf, r = e.mfac * e.kr * e.pr;
    if (qf) qf[i] = f;
    if (qr) qr[i] = r;
    if (wdot) {
      double q = f - r;
      for (int s = 0; s < m->nr[i]; ++s) wdot[m->rsp[CKO_SLOTS * i + s]] -= m->rnu[CKO_SLOTS * i + s] * q;
      for (int s = 0; s < m->np[i]; ++s) wdot[m->psp[CKO_SLOTS * i + s]] += m->pnu[CKO_SLOTS * i + s] * q;
    }
  }
}

void cko_rop_batch(const cko_mech* m, int n, const double* T, const double* P, const double* Y, double* wdot,
                   double* cp, double* h, int nthreads) {
  const int KK = m->KK;
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(static)
#endif
  for (int s = 0; s < n; ++s) {
    double Ys[NMAX], cp_R[NMAX], h_RT[NMAX];
    for (int k = 0; k < KK; ++k) Ys[k] = Y[(size_t)k * n + s]; /* SoA input Y[KK][n] */
    double w[NMAX];
    cko_rates(m, T[s], P[s], Ys, NULL, NULL, w);
    for (int k = 0; k < KK; ++k) wdot[(size_t)k * n + s] = w[k];
    cko_thermo(m, T[s], cp_R, h_RT, NULL);
    double c = 0.0, hh = 0.0;
    for (int k = 0; k < KK; ++k) {
      c += Ys[k] * cp_R[k] * RU / m->wt[k];
      hh += Ys[k] * h_RT[k] * RU * T[s] / m->wt[k];
    }
    cp[s] = c;
    h[s] = hh;
  }
}

/* --------------------------------------------------------- reactor model */
typedef struct {
  const cko_mech* m;
  const cko_cfg* cfg;
  int problem;
  double mass_density0; /* rho0 (CONV: density at V0) */
  double V0, P0, T0;
  int nfe, nje;
  double tsel; /* midpoint of the current integration segment (pwl_eval) */
  double G, Pm; /* plug flow (problem 3): mass flux rho0 u0 [g/cm2-s], momentum constant P0 + G u0 */
  double gam0;  /* engine (problem 4): cp / cv of the initial charge (motored pressure) */
} rctx;

/* piecewise-linear profile at t; the linear piece is the one containing tsel, the midpoint of
 * the current integration segment (segments end at every breakpoint), so a step ending on a
 * breakpoint uses the left slope and the first step after the restart the right one */
static void pwl_eval(const double* x, const double* y, int n, double t, double tsel, double* v, double* dvdt) {
  if (tsel <= x[0]) { *v = y[0]; *dvdt = 0.0; return; }
  if (tsel >= x[n - 1]) { *v = y[n - 1]; *dvdt = 0.0; return; }
  int j = 0;
  while (j < n - 2 && tsel >= x[j + 1]) ++j;
  double s = (y[j + 1] - y[j]) / (x[j + 1] - x[j]);
  *v = y[j] + s * (t - x[j]);
  *dvdt = s;
}

static void profile_eval(const cko_cfg* c, double t, double tsel, double base, double* v, double* dvdt) {
  if (c->nprof <= 0 || c->prof_kind != 0) { *v = base; *dvdt = 0.0; return; }
  pwl_eval(c->prof_t, c->prof_v, c->nprof, t, tsel, v, dvdt);
}

/* f = dy/dt for y = (T, Y_1..Y_KK); J (n x n row-major, optional) = approximate analytic Jacobian */
#define ERG_PER_CAL 4.184e7

static double prof2_value(const cko_cfg* c, double t, double tsel, double base, int kind) {
  double v, d;
  if (kind == 2 && c->nprof3 > 0 && c->nprof2 > 0 && c->prof2_kind == 1) { /* AEXT beside QPRO */
    pwl_eval(c->prof3_t, c->prof3_v, c->nprof3, t, tsel, &v, &d);
    return v;
  }
  if (c->nprof2 <= 0 || c->prof2_kind != kind) return base;
  pwl_eval(c->prof2_t, c->prof2_v, c->nprof2, t, tsel, &v, &d);
  return v;
}

/* Plug-flow reactor (problem 3, Chemkin PLUG without surface chemistry, constant flow area): the
 * independent variable is the distance x [cm] and dy/dx = (rho / G) dy/dt of a constant-pressure
 * batch reactor at the local state, G = rho u the constant mass flux.  The pressure follows the
 * inviscid momentum equation A dP/dx + mdot du/dx = 0, i.e. P + G u = P0 + G u0 with u = G / rho =
 * G R T / (P Wbar): the subsonic root of P^2 - Pm P + G^2 R T / Wbar = 0.  With a PPRO profile the
 * pressure is given instead (MOMEN OFF, PFR.py:515-518) and its dP/dx enters the energy equation as
 * u dP/dx; the u dP/dx of the momentum equation and the kinetic energy are dropped there (both
 * O(u^2 / (cp T)), 5e-8 relative at the plugflow golden's 27 cm/s). */
static double pfr_pressure(const rctx* c, double t, double tsel, double T, double Wbar, double* dPdx) {
  if (c->cfg->nprof > 0 && c->cfg->prof_kind == 0) {
    double P;
    pwl_eval(c->cfg->prof_t, c->cfg->prof_v, c->cfg->nprof, t, tsel, &P, dPdx);
    return P;
  }
  *dPdx = 0.0;
  const double q = c->G * c->G * RU * T / Wbar;
  const double disc = c->Pm * c->Pm - 4.0 * q; /* < 0: choked (clamped; the run ends with status 5) */
  return 0.5 * (c->Pm + sqrt(disc > 0.0 ? disc : 0.0));
}

/* Single-zone IC engine (problem 4: Chemkin's ICEN problem, KINAll0D_SetupHCCIInputs, engines/HCCI.py,
 * engine.py:128-223): a closed constant-mass reactor whose volume follows the slider-crank with a
 * piston-pin offset e = -POLEN, the crank angle measured from the offset engine's own top dead centre
 * (theta = CA + asin(e / (L + a))), the clearance volume from the actual stroke
 * (sqrt((L + a)^2 - e^2) - sqrt((L - a)^2 - e^2)) and the compression ratio.  This form reproduces the
 * hcciengine golden's volume column to 1e-14 (tests/test_engine.py); with e = 0 it is the textbook
 * V = Vc [1 + (CR - 1)/2 (R + 1 - cos theta - sqrt(R^2 - sin^2 theta))]. */
#define CKO_PI 3.14159265358979323846
static void engine_volume(const double* e, double t, double* V, double* dVdt) {
  const double B = e[CKO_ENG_BORE], a = 0.5 * e[CKO_ENG_STROKE], L = e[CKO_ENG_LOLR] * a, ee = -e[CKO_ENG_POLEN];
  const double Ab = 0.25 * CKO_PI * B * B;
  const double st = sqrt((L + a) * (L + a) - ee * ee), sb = sqrt((L - a) * (L - a) - ee * ee);
  const double Vc = Ab * (st - sb) / (e[CKO_ENG_CMPR] - 1.0);
  const double omega = e[CKO_ENG_RPM] * (2.0 * CKO_PI / 60.0);            /* rad/s */
  const double th = (e[CKO_ENG_CA0] + 6.0 * e[CKO_ENG_RPM] * t) * (CKO_PI / 180.0) + asin(ee / (L + a));
  const double sn = sin(th), cs = cos(th);
  const double u = a * sn - ee, r = sqrt(L * L - u * u);
  *V = Vc + Ab * (st - (a * cs + r));
  if (dVdt) *dVdt = Ab * (a * sn + u * a * cs / r) * omega;
}
static double engine_displacement(const double* e) {
  const double B = e[CKO_ENG_BORE], a = 0.5 * e[CKO_ENG_STROKE], L = e[CKO_ENG_LOLR] * a, ee = -e[CKO_ENG_POLEN];
  return 0.25 * CKO_PI * B * B * (sqrt((L + a) * (L + a) - ee * ee) - sqrt((L - a) * (L - a) - ee * ee));
}

/* Wall heat loss coefficient h A [erg/K-s] of the ICHX correlation Nu = h B / lambda = a Re^b Pr^c,
 * Re = rho w B / mu, Pr = cp mu / lambda, with the Woschni gas velocity
 * w = (C11 + C12 v_swirl / Sp) Sp + C2 Vd T_i / (P_i V_i) max(P - P_motored, 0), Sp = 2 S N the mean piston
 * speed, v_swirl = swirl ratio x crank angular speed x B / 2, P_motored = P_i (V_i / V)^gamma_i (gamma_i of
 * the initial charge); wall area = (CYBAR + PSBAR) A_bore + pi B (V - Vc) / A_bore (CYBAR taken as the
 * clearance surface, the liner as swept above it).  mu: Wilke mixture of the species fits; lambda:
 * 0.5 (sum X lambda + 1 / sum X / lambda) (cfg->tran), both of the mole fractions of max(Y, 0): negative
 * mass fractions inside the tolerance (runs without NNEG) must not enter the transport sums.  The published form of Chemkin's engine heat
 * transfer (engine.py:766-924 sets its keywords; the correlation runs in the closed library): the
 * hcciengine golden's pressure is met only in part (tests/test_engine.py). */
static double engine_hA(const rctx* c, double T, double P, double rho, double V, const double* Y, double cpmass) {
  const double* e = c->cfg->eng;
  const cko_mech* m = c->m;
  const int KK = m->KK;
  const double* tf = c->cfg->tran;
  /* gas properties at the film temperature (T + Twall) / 2: the hcciengine golden's own heat loss, backed
     out of its P / rho / V columns, is a constant multiple of this form (relative spread 4e-4 over
     -134..-90 CA) and not of the bulk-temperature form (7e-3, drifting with T); scripts/hcci_golden_heat.py */
  const double lnT = log(0.5 * (T + e[CKO_ENG_TWALL]));
  double X[NMAX], mu[NMAX], lam[NMAX], sx = 0.0;
  for (int k = 0; k < KK; ++k) {
    X[k] = fmax(Y[k], 0.0) / m->wt[k];  /* transport of the non-negative part of the composition */
    sx += X[k];
    const double* f = tf + 8 * k;
    mu[k] = exp(f[0] + lnT * (f[1] + lnT * (f[2] + lnT * f[3])));
    lam[k] = exp(f[4] + lnT * (f[5] + lnT * (f[6] + lnT * f[7])));
  }
  double mum = 0.0, l1 = 0.0, l2 = 0.0;
  for (int k = 0; k < KK; ++k) X[k] /= sx;
  for (int k = 0; k < KK; ++k) {
    double d = 0.0;
    for (int j = 0; j < KK; ++j) {
      const double q = 1.0 + sqrt(mu[k] / mu[j]) * pow(m->wt[j] / m->wt[k], 0.25);
      d += X[j] * q * q / sqrt(8.0 * (1.0 + m->wt[k] / m->wt[j]));
    }
    mum += X[k] * mu[k] / d;
    l1 += X[k] * lam[k];
    l2 += X[k] / lam[k];
  }
  const double lamm = 0.5 * (l1 + 1.0 / l2);
  const double B = e[CKO_ENG_BORE], Ab = 0.25 * CKO_PI * B * B;
  const double Sp = 2.0 * e[CKO_ENG_STROKE] * e[CKO_ENG_RPM] / 60.0;
  const double vsw = e[CKO_ENG_SWIRL] * e[CKO_ENG_RPM] * (2.0 * CKO_PI / 60.0) * 0.5 * B;
  const double Vd = engine_displacement(e), Vc = Vd / (e[CKO_ENG_CMPR] - 1.0);
  const double Pmot = c->P0 * pow(c->V0 / V, c->gam0);
  const double w = (e[CKO_ENG_C11] + e[CKO_ENG_C12] * vsw / Sp) * Sp +
                   e[CKO_ENG_C2] * Vd * c->T0 / (c->P0 * c->V0) * fmax(P - Pmot, 0.0);
  const double Re = rho * w * B / mum, Pr = cpmass * mum / lamm;
  const double h = e[CKO_ENG_HTA] * pow(Re, e[CKO_ENG_HTB]) * pow(Pr, e[CKO_ENG_HTC]) * lamm / B;
  const double area = (e[CKO_ENG_CYBAR] + e[CKO_ENG_PSBAR]) * Ab + CKO_PI * B * (V - Vc) / Ab;
  return h * area;
}

static void reactor_rhs(rctx* c, double t, const double* y, double* f, double* J) {
  const cko_mech* m = c->m;
  const int KK = m->KK, n = KK + 1;
  double T = y[0], dTdt_given = 0.0;
  const int tpro = c->cfg->prof_kind == 1 && c->cfg->energy == 2 && c->cfg->nprof > 0;
  if (tpro) pwl_eval(c->cfg->prof_t, c->cfg->prof_v, c->cfg->nprof, t, c->tsel, &T, &dTdt_given);
  const double dlnA_p = c->cfg->pert_rxn >= 0 ? log(c->cfg->pert_fac) : 0.0;
  const double* Y = y + 1;
  double C[NMAX], cp_R[NMAX], h_RT[NMAX], s_R[NMAX], g_RT[NMAX], Ctot;
  double rho, P, V, dVdt = 0.0, dPdt = 0.0;
  const int pfr = (c->problem == 3);
  const int eng = (c->problem == 4);
  const int conp = (c->problem == 1) || pfr;
  double Wbar = mean_wt(m, Y);
  if (eng) {
    engine_volume(c->cfg->eng, t, &V, &dVdt);
    rho = c->mass_density0 * c->V0 / V;
    P = rho * RU * T / Wbar;
  } else if (pfr) {
    double dPdx;
    P = pfr_pressure(c, t, c->tsel, T, Wbar, &dPdx);
    rho = P * Wbar / (RU * T);
    V = c->G / rho; /* the local velocity */
    dPdt = V * dPdx;
  } else if (conp) {
    profile_eval(c->cfg, t, c->tsel, c->P0, &P, &dPdt);
    rho = P * Wbar / (RU * T);
    V = c->mass_density0 * c->V0 / rho;
  } else {
    profile_eval(c->cfg, t, c->tsel, c->V0, &V, &dVdt);
    rho = c->mass_density0 * c->V0 / V;
    P = rho * RU * T / Wbar;
  }
  conc_from_Y(m, rho, Y, 0, C, &Ctot);
  cko_thermo(m, T, cp_R, h_RT, s_R);
  for (int k = 0; k < KK; ++k) g_RT[k] = h_RT[k] - s_R[k];
  double wdot[NMAX];
  memset(wdot, 0, sizeof(double) * KK);
  double dwdT[NMAX];
  if (J) {
    memset(J, 0, sizeof(double) * n * n);
    memset(dwdT, 0, sizeof(double) * KK);
  }
  const double lnT = log(T), invT = 1.0 / T, lnPRT = log(PATM / (RU * T));
  for (int i = 0; i < m->II; ++i) {
    rxn_eval e;
    eval_reaction(m, i, T, lnT, invT, lnPRT, P, C, Ctot, g_RT, h_RT, i == c->cfg->pert_rxn ? dlnA_p : 0.0,
                  c->cfg->gfac, &e);
    const double q = e.mfac * (e.kf * e.pf - e.kr * e.pr);
    const int* rs = m->rsp + CKO_SLOTS * i;
    const int* ps = m->psp + CKO_SLOTS * i;
    const double* rn = m->rnu + CKO_SLOTS * i;
    const double* pn = m->pnu + CKO_SLOTS * i;
    for (int s = 0; s < m->nr[i]; ++s) wdot[rs[s]] -= rn[s] * q;
    for (int s = 0; s < m->np[i]; ++s) wdot[ps[s]] += pn[s] * q;
    if (!J) continue;
    /* dq/dT at fixed C, then at fixed (Y, P) for CONP */
    double dqdT = e.mfac * (e.kf * e.dlkf * e.pf - e.kr * e.dlkr * e.pr);
    if (conp) {
      double ordf = 0.0, ordr = 0.0;
      for (int s = 0; s < m->nr[i]; ++s) ordf += ford_of(m, i, s);
      for (int s = 0; s < m->np[i]; ++s) ordr += rord_of(m, i, s);
      dqdT -= e.mfac * (ordf * e.kf * e.pf - ordr * e.kr * e.pr) * invT;
      if (m->rtype[i] == 1) dqdT -= q * invT;
    }
    for (int s = 0; s < m->nr[i]; ++s) dwdT[rs[s]] -= rn[s] * dqdT;
    for (int s = 0; s < m->np[i]; ++s) dwdT[ps[s]] += pn[s] * dqdT;
    /* dq/dC_j over reactant and product slots */
    for (int side = 0; side < 2; ++side) {
      const int nsl = side == 0 ? m->nr[i] : m->np[i];
      const int* sp = side == 0 ? rs : ps;
      double ord[CKO_SLOTS];
      for (int s = 0; s < nsl; ++s) ord[s] = side == 0 ? ford_of(m, i, s) : rord_of(m, i, s);
      const double kk = side == 0 ? e.mfac * e.kf : -e.mfac * e.kr;
      if (kk == 0.0) continue;
      for (int s = 0; s < nsl; ++s) {
        double d = dconc_pow(C[sp[s]], ord[s]);
        for (int u = 0; u < nsl; ++u)
          if (u != s) d *= conc_pow(C[sp[u]], ord[u]);
        const double dq = kk * d;
        const int j = sp[s];
        const double wj = 1.0 / m->wt[j];
        for (int u = 0; u < m->nr[i]; ++u) J[(1 + rs[u]) * n + 1 + j] -= rn[u] * dq * m->wt[rs[u]] * wj;
        for (int u = 0; u < m->np[i]; ++u) J[(1 + ps[u]) * n + 1 + j] += pn[u] * dq * m->wt[ps[u]] * wj;
      }
    }
  }
  /* species equations */
  const double rinv = 1.0 / rho;
  for (int k = 0; k < KK; ++k) f[1 + k] = wdot[k] * m->wt[k] * rinv;
  /* energy equation */
  if (c->cfg->energy == 1) {
    double cpm = 0.0, sum = 0.0, e_k[NMAX], c_k[NMAX];
    for (int k = 0; k < KK; ++k) {
      const double cpk = cp_R[k] * RU / m->wt[k];              /* erg/g-K */
      const double hk = h_RT[k] * RU * T / m->wt[k];            /* erg/g   */
      c_k[k] = conp ? cpk : cpk - RU / m->wt[k];
      e_k[k] = conp ? hk : hk - RU * T / m->wt[k];
      cpm += Y[k] * c_k[k];
      sum += e_k[k] * f[1 + k];
    }
    double fT = -sum / cpm;
    if (conp) fT += dPdt / (rho * cpm);
    else fT -= P * dVdt / (V * rho * cpm);
    /* heat loss to the surroundings: QLOS + HTC AREAQ (T - TAMB) [cal/s], per heat capacity m cp */
    const double mcp = c->mass_density0 * c->V0 * cpm;
    const double qloss = prof2_value(c->cfg, t, c->tsel, c->cfg->qloss, 1);
    const double area = prof2_value(c->cfg, t, c->tsel, c->cfg->areaq, 2);
    double q1 = c->cfg->htc * area * ERG_PER_CAL;
    if (eng) { /* engine wall heat transfer replaces the QLOS / HTC terms */
      q1 = 0.0;
      if ((int)c->cfg->eng[CKO_ENG_HTMODEL] == 1) {
        double cpmass = 0.0;
        for (int k = 0; k < KK; ++k) cpmass += Y[k] * cp_R[k] * RU / m->wt[k];
        q1 = engine_hA(c, T, P, rho, V, Y, cpmass);
        fT -= q1 * (T - c->cfg->eng[CKO_ENG_TWALL]) / mcp;
      }
    } else {
      fT -= (qloss * ERG_PER_CAL + q1 * (T - c->cfg->tamb)) / mcp;
    }
    f[0] = fT;
    if (J) {
      for (int k = 0; k < KK; ++k) J[(1 + k) * n] = dwdT[k] * m->wt[k] * rinv + (conp ? f[1 + k] * invT : 0.0);
      for (int j = 0; j < KK; ++j) {
        double s = 0.0;
        for (int k = 0; k < KK; ++k) s += e_k[k] * J[(1 + k) * n + 1 + j];
        J[1 + j] = -s / cpm - fT * c_k[j] / cpm;
      }
      double s = 0.0;
      for (int k = 0; k < KK; ++k) s += c_k[k] * f[1 + k] + e_k[k] * J[(1 + k) * n];
      J[0] = -s / cpm - q1 / mcp;
    }
  } else {
    f[0] = dTdt_given; /* 0 without TPRO */
    if (J) {
      for (int k = 0; k < KK; ++k) J[(1 + k) * n] = dwdT[k] * m->wt[k] * rinv + (conp ? f[1 + k] * invT : 0.0);
    }
  }
  if (pfr) { /* d/dx = (rho / G) d/dt; the Jacobian keeps the batch form scaled alike */
    const double sx = rho / c->G;
    if (c->cfg->energy == 1 || !tpro) f[0] *= sx;  /* a TPRO profile is already T(x) */
    for (int k = 0; k < KK; ++k) f[1 + k] *= sx;
    if (J)
      for (int i = 0; i < n * n; ++i) J[i] *= sx;
  }
  c->nfe++;
  if (J) c->nje++;
}

void cko_rhs_jac(const cko_mech* m, const cko_cfg* cfg, double t, const double* y, double mass_density0,
                 double V0, double P0, double* f, double* J) {
  rctx c = {m, cfg, cfg->problem, mass_density0, V0, P0, y[0], 0, 0, t};
  if (cfg->problem == 3) { /* plug flow: V0 = inlet velocity, mass_density0 = inlet density */
    c.G = mass_density0 * V0;
    c.Pm = P0 + c.G * V0;
  }
  reactor_rhs(&c, t, y, f, J);
}

void cko_rhs_jac_engine(const cko_mech* m, const cko_cfg* cfg, double t, const double* y, double T0, double P0,
                        const double* Y0, double* f, double* J) {
  const int KK = m->KK;
  const double Wbar0 = mean_wt(m, Y0);
  double Vstart;
  engine_volume(cfg->eng, 0.0, &Vstart, NULL);
  rctx c = {m, cfg, 4, P0 * Wbar0 / (RU * T0), Vstart, P0, T0, 0, 0, t};
  double cp_R[NMAX], h_RT[NMAX], s_R[NMAX], cpm = 0.0;
  cko_thermo(m, T0, cp_R, h_RT, s_R);
  for (int k = 0; k < KK; ++k) cpm += Y0[k] * cp_R[k] / m->wt[k];
  c.gam0 = cpm / (cpm - 1.0 / Wbar0);
  reactor_rhs(&c, t, y, f, J);
}

/* ---------------------------------------------------------- dense LU */
static int lu_factor(int n, double* A, int* piv) {
  for (int k = 0; k < n; ++k) {
    int p = k;
    double amax = fabs(A[k * n + k]);
    for (int i = k + 1; i < n; ++i)
      if (fabs(A[i * n + k]) > amax) { amax = fabs(A[i * n + k]); p = i; }
    piv[k] = p;
    if (amax == 0.0) return k + 1;
    if (p != k)
      for (int j = 0; j < n; ++j) { double t = A[k * n + j]; A[k * n + j] = A[p * n + j]; A[p * n + j] = t; }
    const double r = 1.0 / A[k * n + k];
    for (int i = k + 1; i < n; ++i) {
      const double l = A[i * n + k] * r;
      A[i * n + k] = l;
      if (l != 0.0)
        for (int j = k + 1; j < n; ++j) A[i * n + j] -= l * A[k * n + j];
    }
  }
  return 0;
}

static void lu_solve(int n, const double* A, const int* piv, double* b) {
  /* whole rows (multipliers included) were swapped during the factorization, so the
   * permutation is applied to b in full before the unit-lower forward sweep */
  for (int k = 0; k < n; ++k) {
    const int p = piv[k];
    if (p != k) { double t = b[k]; b[k] = b[p]; b[p] = t; }
  }
  for (int k = 0; k < n; ++k)
    for (int i = k + 1; i < n; ++i) b[i] -= A[i * n + k] * b[k];
  for (int k = n - 1; k >= 0; --k) {
    double s = b[k];
    for (int j = k + 1; j < n; ++j) s -= A[k * n + j] * b[j];
    b[k] = s / A[k * n + k];
  }
}

/* Batched dense LU, the integrator's own lu_factor above over nsys row-major n x n matrices in place,
 * OpenMP over systems: the CPU baseline of bench.py's batched-LU line (test infrastructure). */
void cko_lu_factor_batch(int n, int nsys, double* A, int* piv, int* info, int nthreads) {
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(static)
#endif
  for (int s = 0; s < nsys; ++s)
    info[s] = lu_factor(n, A + (size_t)s * n * n, piv + (size_t)s * n);
}

/* ------------------------------------------------------ BDF integrator */
#define QMAX 5
#define L_MAX (QMAX + 1)
#define ETAMX1 10000.0
#define ETAMX2 10.0
#define ETAMX3 10.0
#define ETAMXF 0.2
#define ETAMIN 0.1
#define ETACF 0.25
#define ADDON 1e-6
#define BIAS1 6.0
#define BIAS2 6.0
#define BIAS3 10.0
#define ONEPSM 1.000001
#define SMALL_NST 10
#define MXNCF 10
#define MXNEF 7
#define MXNEF1 3
#define SMALL_NEF 2
#define LONG_WAIT 10
#define MAXCOR 3
#define CRDOWN 0.3
#define DGMAX 0.3
#define RDIV 2.0
#define MSBP 20
/* Jacobian refresh after at most 15 steps (CVODE's msbj, default 51): the stiff ignition runs converge with far
 * fewer steps, RHS calls and Newton setups on a fresher J; priced by scripts/solver_knobs_oracle.py
 * (profiles/r06w_solver_knobs_oracle.log: configs[2] -17 %, configs[4] -11 % modelled cycles, tau within 3e-5; 10 saves 2 % more on configs[2] but
 * stalls one of the 35 tolerance-perturbed FORD runs of tests/test_ford.py) */
#define MSBJ 15
#define THRESH 1.5
#define CORTES 0.1
#define UROUND 2.220446049250313e-16
#define NNEG_TOL 0.01


typedef struct {
  int n;
  double zn[QMAX + 1][NMAX];
  double ewt[NMAX], acor[NMAX], tempv[NMAX], ftemp[NMAX], y[NMAX];
  double* J; /* saved Jacobian n*n */
  double* M; /* LU of I - gamma J */
  int piv[NMAX];
  double tau[QMAX + 2], tq[6], l[QMAX + 1];
  double h, hprime, hscale, eta, etamax, hmin, hmax_inv, tn, rl1, gamma, gammap, gamrat, crate, acnrm, hu;
  double saved_tq5;
  int q, qprime, qwait, L, nst, nstlp, nstlj, jcur, nscon, ncf_tot, nef_tot, nlu;
  double rtol, atol;
  int nneg;
  rctx* ctx;
  /* element projection of the accepted corrector: npe elements (0 = off), pc[m][k] = a_mk / W_k for
   * state component k = 1 + species, eb0[m] = the reactor's initial element content [mol/g] */
  int npe;
  double pc[CKO_PROJ_MMAX][NMAX];
  double eb0[CKO_PROJ_MMAX];
} bdf;

/* x^(1/p) for the step-size / order heuristics, in single precision as on the device
 * (ckmi_reactor.hpp eta_root): it only selects the next step size. */
static double eta_root(double x, int p) { return (double)exp2f(log2f((float)x) / (float)p); }

static double wrms(const bdf* b, const double* v) {
  double s = 0.0;
  for (int i = 0; i < b->n; ++i) { double x = v[i] * b->ewt[i]; s += x * x; }
  return sqrt(s / b->n);
}

static void set_ewt(bdf* b, const double* y) {
  for (int i = 0; i < b->n; ++i) b->ewt[i] = 1.0 / (b->rtol * fabs(y[i]) + b->atol);
}

static void rescale(bdf* b) {
  double factor = b->eta;
  for (int j = 1; j <= b->q; ++j) {
    for (int i = 0; i < b->n; ++i) b->zn[j][i] *= factor;
    factor *= b->eta;
  }
  b->h = b->hscale * b->eta;
  b->hscale = b->h;
  b->nscon = 0;
}

static void predict(bdf* b) {
  b->tn += b->h;
  for (int k = 1; k <= b->q; ++k)
    for (int j = b->q; j >= k; --j)
      for (int i = 0; i < b->n; ++i) b->zn[j - 1][i] += b->zn[j][i];
}

static void restore(bdf* b, double saved_t) {
  b->tn = saved_t;
  for (int k = 1; k <= b->q; ++k)
    for (int j = b->q; j >= k; --j)
      for (int i = 0; i < b->n; ++i) b->zn[j - 1][i] -= b->zn[j][i];
}

static void set_bdf(bdf* b) {
  const int q = b->q;
  double* l = b->l;
  double xi_inv = 1.0, xistar_inv = 1.0, alpha0 = -1.0, alpha0_hat = -1.0, hsum = b->h;
  l[0] = l[1] = 1.0;
  for (int i = 2; i <= QMAX; ++i) l[i] = 0.0;
  if (q > 1) {
    for (int j = 2; j < q; ++j) {
      hsum += b->tau[j - 1];
      xi_inv = b->h / hsum;
      alpha0 -= 1.0 / j;
      for (int i = j; i >= 1; --i) l[i] += l[i - 1] * xi_inv;
    }
    alpha0 -= 1.0 / q;
    xistar_inv = -l[1] - alpha0;
    hsum += b->tau[q - 1];
    xi_inv = b->h / hsum;
    alpha0_hat = -l[1] - xi_inv;
    for (int i = q; i >= 1; --i) l[i] += l[i - 1] * xistar_inv;
  }
  const double A1 = 1.0 - alpha0_hat + alpha0;
  const double A2 = 1.0 + q * A1;
  b->tq[2] = fabs(A1 / (alpha0 * A2));
  b->tq[5] = fabs(A2 * xistar_inv / (l[q] * xi_inv));
  if (b->qwait == 1) {
    if (q > 1) {
      const double Cc = xistar_inv / l[q];
      const double A3 = alpha0 + 1.0 / q;
      const double A4 = alpha0_hat + xi_inv;
      const double Cpinv = (1.0 - A4 + A3) / A3;
      b->tq[1] = fabs(Cc * Cpinv);
    } else {
      b->tq[1] = 1.0;
    }
    hsum += b->tau[q];
    xi_inv = b->h / hsum;
    const double A5 = alpha0 - 1.0 / (q + 1);
    const double A6 = alpha0_hat - xi_inv;
    const double Cppinv = (1.0 - A6 + A5) / A2;
    b->tq[3] = fabs(Cppinv / (xi_inv * (q + 2) * A5));
  }
  b->tq[4] = CORTES / b->tq[2];
  b->rl1 = 1.0 / l[1];
  b->gamma = b->h * b->rl1;
  if (b->nst == 0) b->gammap = b->gamma;
  b->gamrat = (b->nst > 0) ? b->gamma / b->gammap : 1.0;
}

static void adjust_order(bdf* b, int deltaq) {
  const int q = b->q;
  double* l = b->l;
  for (int i = 0; i <= QMAX; ++i) l[i] = 0.0;
  l[2] = 1.0;
  if (deltaq == 1) {
    double alpha1 = 1.0, prod = 1.0, xiold = 1.0, alpha0 = -1.0, hsum = b->hscale;
    for (int j = 1; j < q; ++j) {
      hsum += b->tau[j + 1];
      const double xi = hsum / b->hscale;
      prod *= xi;
      alpha0 -= 1.0 / (j + 1);
      alpha1 += 1.0 / xi;
      for (int i = j + 2; i >= 2; --i) l[i] = l[i] * xiold + l[i - 1];
      xiold = xi;
    }
    const double A1 = (-alpha0 - alpha1) / prod;
    const int L = q + 1;
    for (int i = 0; i < b->n; ++i) b->zn[L][i] = A1 * b->zn[QMAX][i];
    for (int j = 2; j <= q; ++j)
      for (int i = 0; i < b->n; ++i) b->zn[j][i] += l[j] * b->zn[L][i];
  } else {
    double hsum = 0.0;
    for (int j = 1; j <= q - 2; ++j) {
      hsum += b->tau[j];
      const double xi = hsum / b->hscale;
      for (int i = j + 2; i >= 2; --i) l[i] = l[i] * xi + l[i - 1];
    }
    for (int j = 2; j < q; ++j)
      for (int i = 0; i < b->n; ++i) b->zn[j][i] -= l[j] * b->zn[q][i];
  }
}

/* Element projection of an accepted step (CVODE's projection of the corrector, CVodeSetProjFn, restated for
 * the linear element constraints).  A closed reactor conserves the element content e_m = sum_k a_mk Y_k / W_k
 * exactly; the modified Newton iteration conserves it only to the accuracy of the linear solves (J is parked
 * in FP32 and M^-1 is inexact: c M^-1 != c), so without this the element totals drift by up to a few 1e-7
 * over a run.  Conservation is held to PROJ_TOL rtol: after the error test passes, when the residual of
 * y = zn[0] + acor, max_m |C y - eb0|_m / max_m eb0_m, exceeds PROJ_TOL rtol, y is moved to the nearest state with
 * C y = eb0 in the weighted norm sum_k dy_k^2 / w_k, w_k = Y_k W_k (moles: dY_k = Y_k sum_m a_mk lambda_m, the
 * element-potential form of equilibrium solvers -- every species changes by a relative amount of the size of
 * the drift, ~1e-10, so none changes sign; error weights (rtol |y| + atol)^2 put corrections of atol size on
 * trace species and drove them negative under NNEG), by
 *     (C W C^T + eps diag(C W C^T)) lambda = C y - eb0,   acor_k -= w_k sum_m C_mk lambda_m,
 * before the history update, so the whole Nordsieck array moves with it.  eps = PROJ_RIDGE keeps element
 * combinations carried only by trace species from amplifying the residual; an element with no weight at all
 * (absent from the mixture) is left out; species at or below 0 get no weight.  Both device kernels do the same
 * (ckmi_reactor.hpp elem_project_wave, ckmi_big.hip elem_project_big: one fused 8-value reduction of the
 * residual per accepted step, the Gram matrix only past the threshold).  Below the threshold the step is left as it is (most runs are
 * never projected: their drift stays far below rtol), which keeps the integrator's results those of the
 * unconstrained BDF (e.g. the sensitivity golden's finite differences). */
#define PROJ_RIDGE 1e-8
#define PROJ_TRACE 1e-6
#ifndef PROJ_TOL
#define PROJ_TOL 0.1
#endif
/* the residual is checked on every accepted step.  (-DPROJ_EVERY=4, checking every 4th step only, was measured
 * and rejected: the 4-step drift then comes back in one correction, which the error estimate of the following
 * steps sees as a periodic perturbation -- with a tight PROJ_TOL the configs[4] sample's steps went from
 * 1,228 to 5,903 on average and 115,061 at worst -- and up to 3 unprojected steps end a run: drift max 4.6e-8
 * against 7.9e-10) */
#ifndef PROJ_EVERY
#define PROJ_EVERY 1
#endif
static int elem_project(bdf* b) {
  const int n = b->n, M = b->npe;
  if (M <= 0) return 0;
  double r[CKO_PROJ_MMAX], G[CKO_PROJ_MMAX][CKO_PROJ_MMAX], w[NMAX];
  for (int m = 0; m < M; ++m) {
    r[m] = 0.0;
    for (int l = 0; l < M; ++l) G[m][l] = 0.0;
  }
  for (int k = 1; k < n; ++k) {
    const double y = b->zn[0][k] + b->acor[k];
    w[k] = y > 0.0 ? y * b->ctx->m->wt[k - 1] : 0.0;
    for (int m = 0; m < M; ++m) {
      const double cm = b->pc[m][k];
      r[m] += cm * y;
      const double cw = cm * w[k];
      for (int l = 0; l <= m; ++l) G[m][l] += cw * b->pc[l][k];
    }
  }
  double rmax = 0.0, bmax = 0.0;
  for (int m = 0; m < M; ++m) {
    rmax = fmax(rmax, fabs(r[m] - b->eb0[m]));
    bmax = fmax(bmax, b->eb0[m]);
  }
  if (!(rmax > PROJ_TOL * b->rtol * bmax)) return 0;
  /* trace elements (initial content at most PROJ_TRACE of the largest) are left out: their Gram entries carry
   * only trace species, and a multiplier from them would rescale those species by orders of magnitude */
  for (int m = 0; m < M; ++m)
    if (!(b->eb0[m] > PROJ_TRACE * bmax)) G[m][m] = 0.0;
  /* LDL^T of the ridged Gram matrix (lower triangle), elements without weight dropped */
  double L[CKO_PROJ_MMAX][CKO_PROJ_MMAX], dg[CKO_PROJ_MMAX], z[CKO_PROJ_MMAX], lam[CKO_PROJ_MMAX];
  int live[CKO_PROJ_MMAX];
  for (int j = 0; j < M; ++j) {
    live[j] = G[j][j] > 0.0;
    double dj = G[j][j] * (1.0 + PROJ_RIDGE);
    for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k] * dg[k];
    dg[j] = live[j] ? dj : 1.0;
    for (int i = j + 1; i < M; ++i) {
      double v = G[i][j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * dg[k];
      L[i][j] = live[j] ? v / dg[j] : 0.0;
    }
  }
  for (int j = 0; j < M; ++j) {
    double v = r[j] - b->eb0[j];
    for (int k = 0; k < j; ++k) v -= L[j][k] * z[k];
    z[j] = live[j] ? v : 0.0;
  }
  for (int j = M - 1; j >= 0; --j) {
    double v = z[j] / dg[j];
    for (int i = j + 1; i < M; ++i) v -= L[i][j] * lam[i];
    lam[j] = live[j] ? v : 0.0;
  }
  for (int k = 1; k < n; ++k) {
    double s = 0.0;
    for (int m = 0; m < M; ++m) s += b->pc[m][k] * lam[m];
    b->acor[k] -= w[k] * s;
  }
  return 1;
}

enum { NF_FIRST = 0, NF_CONV_FAIL = 1, NF_ERR_FAIL = 2 };
enum { CF_NONE = 0, CF_BAD_J = 1, CF_OTHER = 2 };

/* modified Newton corrector: 0 converged, 1 convergence failure */
static int nls(bdf* b, int nflag) {
  const int n = b->n;
  int convfail = (nflag == NF_FIRST || nflag == NF_ERR_FAIL) ? CF_NONE : CF_OTHER;
  int call_setup = (nflag != NF_FIRST) || b->nst == 0 || b->nst >= b->nstlp + MSBP || fabs(b->gamrat - 1.0) > DGMAX;
  for (;;) {
    for (int i = 0; i < n; ++i) b->y[i] = b->zn[0][i];
    reactor_rhs(b->ctx, b->tn, b->y, b->ftemp, NULL);
    if (call_setup) {
      const double dgamma = fabs(b->gamma / b->gammap - 1.0);
      const int jbad = b->nst == 0 || b->nst >= b->nstlj + MSBJ || (convfail == CF_BAD_J && dgamma < DGMAX) ||
                       convfail == CF_OTHER;
      if (jbad) {
        double* fdum = b->tempv;
        reactor_rhs(b->ctx, b->tn, b->y, fdum, b->J);
        b->nstlj = b->nst;
        b->jcur = 1;
      } else {
        b->jcur = 0;
      }
      /* the device parks J in FP32 between setups (ckmi.hip reactor_kernel): M is built from
         the same rounded J, so both take the same Newton iterations */
      for (int i = 0; i < n * n; ++i) b->M[i] = -b->gamma * (double)(float)b->J[i];
      for (int i = 0; i < n; ++i) b->M[i * n + i] += 1.0;
      const int sing = lu_factor(n, b->M, b->piv);
      b->nlu++;
      b->crate = 1.0;
      b->gammap = b->gamma;
      b->gamrat = 1.0;
      b->nstlp = b->nst;
      if (sing) return 1;
    }
    for (int i = 0; i < n; ++i) b->acor[i] = 0.0;
    double delp = 0.0;
    int mm = 0;
    int failed = 0;
    for (;;) {
      for (int i = 0; i < n; ++i) b->tempv[i] = b->gamma * b->ftemp[i] - (b->rl1 * b->zn[1][i] + b->acor[i]);
      lu_solve(n, b->M, b->piv, b->tempv);
      if (b->gamrat != 1.0) {
        const double s = 2.0 / (1.0 + b->gamrat);
        for (int i = 0; i < n; ++i) b->tempv[i] *= s;
      }
      const double del = wrms(b, b->tempv);
      for (int i = 0; i < n; ++i) {
        b->acor[i] += b->tempv[i];
        b->y[i] = b->zn[0][i] + b->acor[i];
      }
      if (mm > 0) b->crate = fmax(CRDOWN * b->crate, del / delp);
      const double dcon = del * fmin(1.0, b->crate) / b->tq[4];
      if (dcon <= 1.0) {
        if (b->nneg) {
          /* DASSL-style non-negativity: a large negative excursion is a failure, a small one is projected */
          double s = 0.0;
          int neg = 0;
          for (int i = 1; i < n; ++i)
            if (b->y[i] < 0.0) { const double x = b->y[i] * b->ewt[i]; s += x * x; neg = 1; }
          if (neg) {
            if (sqrt(s / n) > NNEG_TOL) { failed = 2; break; }
            for (int i = 1; i < n; ++i)
              if (b->y[i] < 0.0) { b->y[i] = 0.0; b->acor[i] = -b->zn[0][i]; }
            b->acnrm = wrms(b, b->acor);
            b->jcur = 0;
            return 0;
          }
        }
        b->acnrm = (mm == 0) ? del : wrms(b, b->acor);
        b->jcur = 0;
        return 0;
      }
      mm++;
      if (mm == MAXCOR || (mm >= 2 && del > RDIV * delp)) { failed = 1; break; }
      delp = del;
      reactor_rhs(b->ctx, b->tn, b->y, b->ftemp, NULL);
    }
    if (failed == 1 && !b->jcur) {
      convfail = CF_BAD_J;
      call_setup = 1;
      continue;
    }
    return 1;
  }
}

static double dky0(const bdf* b, double t, int comp) {
  const double s = (t - b->tn) / b->h;
  double v = b->zn[b->q][comp];
  for (int j = b->q - 1; j >= 0; --j) v = b->zn[j][comp] + s * v;
  return v;
}

static void dky_vec(const bdf* b, double t, double* out) {
  const double s = (t - b->tn) / b->h;
  for (int i = 0; i < b->n; ++i) {
    double v = b->zn[b->q][i];
    for (int j = b->q - 1; j >= 0; --j) v = b->zn[j][i] + s * v;
    out[i] = v;
  }
}

/* initial step size, CVODE cvHin-style */
static double initial_step(bdf* b, double tout) {
  const int n = b->n;
  const double t0 = b->tn;
  const double tdist = fabs(tout - t0);
  const double tround = UROUND * fmax(fabs(t0), fabs(tout));
  const double hlb = 100.0 * tround;
  double hub = 0.1 * tdist;
  double hub_inv = 0.0;
  for (int i = 0; i < n; ++i) {
    const double num = fabs(b->zn[1][i]);
    const double den = 0.1 * fabs(b->zn[0][i]) + b->atol;
    const double r = num / (den > 0 ? den : 1e-300);
    if (r > hub_inv) hub_inv = r;
  }
  if (hub * hub_inv > 1.0) hub = 1.0 / hub_inv;
  double hg = sqrt(hlb * hub);
  if (hub < hlb) return hg;
  double hnew = hg;
  double y1[NMAX], f1[NMAX];
  for (int count = 1; count <= 4; ++count) {
    /* ydd norm */
    for (int i = 0; i < n; ++i) y1[i] = b->zn[0][i] + hg * b->zn[1][i];
    reactor_rhs(b->ctx, t0 + hg, y1, f1, NULL);
    for (int i = 0; i < n; ++i) f1[i] = (f1[i] - b->zn[1][i]) / hg;
    const double yddnrm = wrms(b, f1);
    hnew = (yddnrm * hub * hub > 2.0) ? sqrt(2.0 / yddnrm) : sqrt(hg * hub);
    if (count == 4) break;
    const double hrat = hnew / hg;
    if (hrat > 0.5 && hrat < 2.0) break;
    if (count >= 2 && hrat > 2.0) { hnew = hg; break; }
    hg = hnew;
  }
  double h0 = 0.5 * hnew;
  if (h0 < hlb) h0 = hlb;
  if (h0 > hub) h0 = hub;
  return h0;
}

/* (re)start the Nordsieck history at (t, y) */
static void bdf_start(bdf* b, double t, const double* y, double tout, double h0, double hmax) {
  const int n = b->n;
  b->tn = t;
  for (int i = 0; i < n; ++i) b->zn[0][i] = y[i];
  set_ewt(b, y);
  reactor_rhs(b->ctx, t, y, b->zn[1], NULL);
  double h = h0 > 0.0 ? h0 : initial_step(b, tout);
  if (h > hmax) h = hmax;
  if (h > tout - t) h = tout - t;
  for (int i = 0; i < n; ++i) b->zn[1][i] *= h;
  b->h = b->hscale = b->hprime = h;
  b->q = b->qprime = 1;
  b->L = 2;
  b->qwait = b->L;
  b->etamax = ETAMX1;
  b->nst = 0;
  b->nstlp = 0;
  b->nstlj = 0;
  b->jcur = 0;
  b->nscon = 0;
  b->crate = 1.0;
  b->gammap = b->gamma = b->h;
  b->gamrat = 1.0;
  b->saved_tq5 = 0.0;
  for (int i = 0; i <= QMAX + 1; ++i) b->tau[i] = 0.0;
  for (int i = 0; i < 6; ++i) b->tq[i] = 0.0;
  b->hu = 0.0;
}

/* one BDF step: 0 ok, 2 error test failures, 3 convergence failures */
static int bdf_step(bdf* b, int* nst_global) {
  const double saved_t = b->tn;
  int ncf = 0, nef = 0, nflag = NF_FIRST;
  double dsm;
  if (b->nst > 0 && b->hprime != b->h) {
    if (b->qprime != b->q) {
      adjust_order(b, b->qprime - b->q);
      b->q = b->qprime;
      b->L = b->q + 1;
      b->qwait = b->L;
    }
    rescale(b);
  }
  for (;;) {
    predict(b);
    set_bdf(b);
    const int r = nls(b, nflag);
    if (r != 0) {
      ncf++;
      b->ncf_tot++;
      b->etamax = 1.0;
      restore(b, saved_t);
      if (fabs(b->h) <= b->hmin * ONEPSM || ncf == MXNCF) return 3;
      b->eta = fmax(ETACF, b->hmin / fabs(b->h));
      nflag = NF_CONV_FAIL;
      rescale(b);
      continue;
    }
    dsm = b->acnrm * b->tq[2];
    if (dsm <= 1.0) break;
    nef++;
    b->nef_tot++;
    nflag = NF_ERR_FAIL;
    restore(b, saved_t);
    if (fabs(b->h) <= b->hmin * ONEPSM || nef == MXNEF) return 2;
    b->etamax = 1.0;
    if (nef <= MXNEF1) {
      b->eta = 1.0 / (eta_root(BIAS2 * dsm, b->L) + ADDON);
      b->eta = fmax(ETAMIN, fmax(b->eta, b->hmin / fabs(b->h)));
      if (nef >= SMALL_NEF) b->eta = fmin(b->eta, ETAMXF);
      rescale(b);
      continue;
    }
    if (b->q > 1) {
      b->eta = fmax(ETAMIN, b->hmin / fabs(b->h));
      adjust_order(b, -1);
      b->L = b->q;
      b->q--;
      b->qwait = b->L;
      rescale(b);
      continue;
    }
    b->eta = fmax(ETAMIN, b->hmin / fabs(b->h));
    b->h *= b->eta;
    b->hscale = b->h;
    b->qwait = LONG_WAIT;
    b->nscon = 0;
    reactor_rhs(b->ctx, b->tn, b->zn[0], b->tempv, NULL);
    for (int i = 0; i < b->n; ++i) b->zn[1][i] = b->h * b->tempv[i];
  }
  /* complete step */
  b->nst++;
  (*nst_global)++;
  b->nscon++;
  b->hu = b->h;
  for (int i = b->q; i >= 2; --i) b->tau[i] = b->tau[i - 1];
  if (b->q == 1 && b->nst > 1) b->tau[2] = b->tau[1];
  b->tau[1] = b->h;
  /* the order-selection norms of a step that selects (qwait reaches 0 below), from the corrector before
   * the element projection: the device kernels take them in the step's one fused reduction beside the
   * element residual (ckmi_big.hip: one workgroup barrier per accepted step) */
  double ddn = 0.0, dup = 0.0;
  if (b->etamax != 1.0 && b->qwait == 1) {
    if (b->q > 1) {
      for (int i = 0; i < b->n; ++i) b->tempv[i] = b->zn[b->q][i] + b->l[b->q] * b->acor[i];
      ddn = wrms(b, b->tempv) * b->tq[1];
    }
    if (b->q != QMAX && b->saved_tq5 != 0.0) {
      const double hr = b->h / b->tau[2];
      double hrL = hr;
      for (int j = 1; j < b->L; ++j) hrL *= hr;
      const double cquot = (b->tq[5] / b->saved_tq5) * hrL;
      for (int i = 0; i < b->n; ++i) b->tempv[i] = b->acor[i] - cquot * b->zn[QMAX][i];
      dup = wrms(b, b->tempv) * b->tq[3];
    }
  }
  if (b->nst % PROJ_EVERY == 0) elem_project(b);
  for (int j = 0; j <= b->q; ++j)
    for (int i = 0; i < b->n; ++i) b->zn[j][i] += b->l[j] * b->acor[i];
  b->qwait--;
  if (b->qwait == 1 && b->q != QMAX) {
    for (int i = 0; i < b->n; ++i) b->zn[QMAX][i] = b->acor[i];
    b->saved_tq5 = b->tq[5];
  }
  /* prepare next step */
  if (b->etamax == 1.0) {
    if (b->qwait < 2) b->qwait = 2;
    b->qprime = b->q;
    b->hprime = b->h;
    b->eta = 1.0;
  } else {
    const double etaq = 1.0 / (eta_root(BIAS2 * dsm, b->L) + ADDON);
    if (b->qwait != 0) {
      b->eta = etaq;
      b->qprime = b->q;
    } else {
      b->qwait = 2;
      double etaqm1 = 0.0, etaqp1 = 0.0;
      if (b->q > 1) etaqm1 = 1.0 / (eta_root(BIAS1 * ddn, b->q) + ADDON);
      if (b->q != QMAX && b->saved_tq5 != 0.0) etaqp1 = 1.0 / (eta_root(BIAS3 * dup, b->L + 1) + ADDON);
      const double etam = fmax(etaqm1, fmax(etaq, etaqp1));
      if (etam < THRESH) {
        b->eta = 1.0;
        b->qprime = b->q;
      } else if (etam == etaq) {
        b->eta = etaq;
        b->qprime = b->q;
      } else if (etam == etaqm1) {
        b->eta = etaqm1;
        b->qprime = b->q - 1;
      } else {
        b->eta = etaqp1;
        b->qprime = b->q + 1;
        for (int i = 0; i < b->n; ++i) b->zn[QMAX][i] = b->acor[i];
      }
    }
    /* set eta */
    if (b->eta < THRESH) {
      b->eta = 1.0;
      b->hprime = b->h;
    } else {
      b->eta = fmin(b->eta, b->etamax);
      b->eta /= fmax(1.0, fabs(b->h) * b->hmax_inv * b->eta);
      b->hprime = b->h * b->eta;
    }
  }
  b->etamax = (b->nst <= SMALL_NST) ? ETAMX2 : ETAMX3;
  return 0;
}

/* ------------------------------------------------------ ignition monitor */
typedef struct {
  int mode, comp;
  double thresh;
  double best, tbest, tprev, vprev, tnext, vnext, tlast, vlast;
  int have_prev, have_next, found, started;
  double tau;
} ignmon;

static void ign_init(ignmon* g, const cko_cfg* cfg, double T0) {
  memset(g, 0, sizeof(*g));
  g->mode = cfg->ign_mode;
  g->tau = -1.0;
  g->best = -1e300;
  if (g->mode == 2) g->thresh = T0 + cfg->ign_val;
  if (g->mode == 3) g->thresh = cfg->ign_val;
  g->comp = (g->mode == 4) ? 1 + cfg->ign_species : 0;
}

/* called after every accepted step; v = monitored value at tn (dT/dt for TIFP, Y_k for KLIM) */
static void ign_peak_update(ignmon* g, double t, double v) {
  if (g->started && g->found == 0 && v > g->best) {
    g->tprev = g->tlast; g->vprev = g->vlast; g->have_prev = 1;
    g->best = v; g->tbest = t; g->have_next = 0;
  } else if (g->started && !g->have_next && g->tbest != 0.0 && t > g->tbest) {
    g->tnext = t; g->vnext = v; g->have_next = 1;
  } else if (!g->started) {
    g->best = v; g->tbest = t; g->have_prev = 0;
  }
  g->started = 1;
  g->tlast = t; g->vlast = v;
}

static double ign_peak_time(const ignmon* g) {
  if (g->tbest <= 0.0) return -1.0;
  if (!(g->have_prev && g->have_next)) return g->tbest;
  /* vertex of the parabola through the three samples around the maximum */
  const double x0 = g->tprev, x1 = g->tbest, x2 = g->tnext;
  const double y0 = g->vprev, y1 = g->best, y2 = g->vnext;
  const double d01 = (y1 - y0) / (x1 - x0), d12 = (y2 - y1) / (x2 - x1);
  const double a = (d12 - d01) / (x2 - x0);
  if (!(a < 0.0)) return x1;
  const double bcoef = d01 - a * (x0 + x1);
  const double tv = -bcoef / (2.0 * a);
  if (tv < x0 || tv > x2) return x1;
  return tv;
}

/* ---------------------------------------------------------- driver */
int cko_reactor(const cko_mech* m, const cko_cfg* cfg, double T0, double P0, double V0, const double* Y0,
                double* Yend, cko_result* res, int nsave, const double* t_save, double* y_save, double* p_save,
                double* v_save) {
  const int KK = m->KK, n = KK + 1;
  if (cfg->prof_kind == 1 && cfg->energy == 2 && cfg->nprof > 0) T0 = cfg->prof_v[0]; /* TPRO start */
  bdf* b = (bdf*)calloc(1, sizeof(bdf));
  b->J = (double*)calloc((size_t)n * n, sizeof(double));
  b->M = (double*)calloc((size_t)n * n, sizeof(double));
  b->n = n;
  b->rtol = cfg->rtol;
  b->atol = cfg->atol;
  b->nneg = cfg->nneg;
  b->npe = (!cfg->no_elem_proj && m->ncf && m->MM > 0 && m->MM <= CKO_PROJ_MMAX) ? m->MM : 0;
  for (int e = 0; e < b->npe; ++e) {
    b->pc[e][0] = 0.0;
    b->eb0[e] = 0.0;
    for (int k = 0; k < KK; ++k) {
      b->pc[e][1 + k] = m->ncf[(size_t)e * KK + k] / m->wt[k];
      b->eb0[e] += b->pc[e][1 + k] * Y0[k];
    }
  }
  const double Wbar0 = mean_wt(m, Y0);
  const double rho0 = P0 * Wbar0 / (RU * T0);
  double Vstart = V0;
  if (cfg->problem == 2 && cfg->nprof > 0 && cfg->prof_kind == 0) Vstart = cfg->prof_v[0];
  if (cfg->problem == 4) engine_volume(cfg->eng, 0.0, &Vstart, NULL);
  rctx ctx = {m, cfg, cfg->problem, rho0, Vstart, P0, T0, 0, 0};
  if (cfg->problem == 4) {
    double cp_R[NMAX], h_RT[NMAX], s_R[NMAX], cpm = 0.0;
    cko_thermo(m, T0, cp_R, h_RT, s_R);
    for (int k = 0; k < KK; ++k) cpm += Y0[k] * cp_R[k] / m->wt[k];
    ctx.gam0 = cpm / (cpm - 1.0 / Wbar0);
  }
  if ((cfg->problem == 1 || cfg->problem == 3) && cfg->nprof > 0 && cfg->prof_kind == 0) ctx.P0 = cfg->prof_v[0];
  if (cfg->problem == 3) { /* plug flow: V0 is the inlet velocity u0 [cm/s] */
    ctx.G = rho0 * V0; /* mdot / A: the inlet density (inlet pressure) x u0, with or without PPRO */
    ctx.Pm = ctx.P0 + ctx.G * V0;
  }
  b->ctx = &ctx;
  const double tend = cfg->t_end;
  const double hmax = cfg->hmax > 0.0 ? cfg->hmax : tend / 100.0;
  b->hmax_inv = 1.0 / hmax;
  b->hmin = 0.0;
  double y[NMAX];
  y[0] = T0;
  for (int k = 0; k < KK; ++k) y[1 + k] = Y0[k];
  /* profile breakpoints are integration stop points (derivative discontinuities) */
  double tcrit[194];
  int ncrit = 0;
  for (int i = 0; i < cfg->nprof && ncrit < 64; ++i)
    if (cfg->prof_t[i] > 0.0 && cfg->prof_t[i] < tend) tcrit[ncrit++] = cfg->prof_t[i];
  for (int i = 0; i < cfg->nprof2 && ncrit < 128; ++i)
    if (cfg->prof2_t[i] > 0.0 && cfg->prof2_t[i] < tend) tcrit[ncrit++] = cfg->prof2_t[i];
  for (int i = 0; i < cfg->nprof3 && ncrit < 192; ++i)
    if (cfg->prof3_t[i] > 0.0 && cfg->prof3_t[i] < tend) tcrit[ncrit++] = cfg->prof3_t[i];
  /* sorted union of both profiles' breakpoints */
  for (int i = 1; i < ncrit; ++i)
    for (int j = i; j > 0 && tcrit[j - 1] > tcrit[j]; --j) {
      const double tmp = tcrit[j]; tcrit[j] = tcrit[j - 1]; tcrit[j - 1] = tmp;
    }
  {
    int u = 0;
    for (int i = 0; i < ncrit; ++i)
      if (u == 0 || tcrit[i] != tcrit[u - 1]) tcrit[u++] = tcrit[i];
    ncrit = u;
  }
  tcrit[ncrit++] = tend;
  int icrit = 0;
  ctx.tsel = 0.5 * tcrit[0];
  bdf_start(b, 0.0, y, tcrit[0], cfg->h0, hmax);
  ignmon g;
  ign_init(&g, cfg, T0);
  int isave = 0;
  /* save points at t = 0 */
  while (isave < nsave && t_save[isave] <= 0.0) {
    for (int i = 0; i < n; ++i) y_save[(size_t)isave * n + i] = y[i];
    if (p_save) p_save[isave] = P0;
    if (v_save) v_save[isave] = Vstart;
    isave++;
  }
  if (g.mode == 1 || g.mode == 4) {
    double f0[NMAX];
    reactor_rhs(&ctx, 0.0, y, f0, NULL);
    ign_peak_update(&g, 0.0, g.mode == 1 ? f0[0] : y[g.comp]);
  }
  int status = 0, nst = 0, stopped = 0;
  const int max_steps = cfg->max_steps > 0 ? cfg->max_steps : 200000;
  const double guard_y = cfg->atol * 1e3 > 1e-3 ? cfg->atol * 1e3 : 1e-3;
  double guard_tlo = 1e300, guard_thi = 0.0;
  for (int k = 0; k < KK; ++k) {
    if (m->thermo[17 * k] < guard_tlo) guard_tlo = m->thermo[17 * k];
    if (m->thermo[17 * k + 2] > guard_thi) guard_thi = m->thermo[17 * k + 2];
  }
  guard_tlo *= 0.5;
  guard_thi *= 2.0; /* margin: legitimately hot runs extrapolate the fits (runaways reach 8-10k K) */
  double tstop_final = tend;
  while (b->tn < tend * (1.0 - 1e-15)) {
    /* clamp the next step to the next critical time */
    const double tc = tcrit[icrit];
    if (b->tn + b->hprime > tc) {
      const double hp = tc - b->tn;
      b->eta = hp / b->h;
      if (b->nst > 0) {
        b->hprime = hp;
      } else {
        rescale(b);
        b->hprime = b->h;
      }
    }
    set_ewt(b, b->zn[0]);
    const double told = b->tn;
    int r = bdf_step(b, &nst);
    if (r != 0) { status = r; break; }
    /* runaway guard (include/ckmi.h CKMI_RUN_RUNAWAY; both device kernels test the same) */
    {
      int bad = cfg->energy == 1 && !(b->zn[0][0] >= guard_tlo && b->zn[0][0] <= guard_thi);
      for (int k = 0; k < KK && !bad; ++k) bad = -b->zn[0][1 + k] > guard_y;
      if (bad) { status = 4; break; }
    }
    /* plug flow past the choke point of the momentum equation (include/ckmi.h CKMI_RUN_CHOKED) */
    if (cfg->problem == 3 && !(cfg->nprof > 0 && cfg->prof_kind == 0)) {
      const double Wb = mean_wt(m, b->zn[0] + 1);
      if (ctx.Pm * ctx.Pm - 4.0 * ctx.G * ctx.G * RU * b->zn[0][0] / Wb < 0.0) { status = 5; break; }
    }
    const double tn = b->tn;
    /* solution saving by interpolation */
    while (isave < nsave && t_save[isave] <= tn) {
      double ys[NMAX];
      dky_vec(b, t_save[isave], ys);
      for (int i = 0; i < n; ++i) y_save[(size_t)isave * n + i] = ys[i];
      double Wb = mean_wt(m, ys + 1), rho, P, V, d;
      if (cfg->problem == 4) {
        engine_volume(cfg->eng, t_save[isave], &V, NULL);
        P = (rho0 * Vstart / V) * RU * ys[0] / Wb;
      } else if (cfg->problem == 3) {
        P = pfr_pressure(&ctx, t_save[isave], t_save[isave], ys[0], Wb, &d);
        V = ctx.G / (P * Wb / (RU * ys[0])); /* velocity */
      } else if (cfg->problem == 1) {
        profile_eval(cfg, t_save[isave], t_save[isave], ctx.P0, &P, &d);
        rho = P * Wb / (RU * ys[0]);
        V = rho0 * Vstart / rho;
      } else {
        profile_eval(cfg, t_save[isave], t_save[isave], Vstart, &V, &d);
        rho = rho0 * Vstart / V;
        P = rho * RU * ys[0] / Wb;
      }
      if (p_save) p_save[isave] = P;
      if (v_save) v_save[isave] = V;
      isave++;
    }
    /* ignition detection */
    if (g.mode == 1) {
      ign_peak_update(&g, tn, b->zn[1][0] / b->h);
    } else if (g.mode == 4) {
      ign_peak_update(&g, tn, b->zn[0][g.comp]);
    } else if ((g.mode == 2 || g.mode == 3) && !g.found && b->zn[0][0] >= g.thresh) {
      double lo = told, hi = tn;
      for (int it = 0; it < 60; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (dky0(b, mid, 0) >= g.thresh) hi = mid; else lo = mid;
      }
      g.found = 1;
      g.tau = hi;
    }
    if (cfg->ign_stop) {
      if ((g.mode == 2 || g.mode == 3) && g.found) { stopped = 1; tstop_final = tn; break; }
      if (g.mode == 1 && g.have_next && g.vlast < 0.1 * g.best && b->zn[0][0] > T0 + 200.0) {
        stopped = 1; tstop_final = tn; break;
      }
    }
    if (nst >= max_steps) { status = 1; break; }
    if (tn >= tc * (1.0 - 1e-15) && icrit < ncrit - 1) {
      /* restart at the breakpoint */
      double yc[NMAX];
      for (int i = 0; i < n; ++i) yc[i] = b->zn[0][i];
      icrit++;
      const int nlu = b->nlu, ncf = b->ncf_tot, nef = b->nef_tot;
      ctx.tsel = 0.5 * (tn + tcrit[icrit]);
      bdf_start(b, tn, yc, tcrit[icrit], 0.0, hmax);
      b->nlu = nlu; b->ncf_tot = ncf; b->nef_tot = nef;
    }
  }
  /* final state */
  double yf[NMAX];
  double tf = tend;
  if (stopped || status) {
    tf = b->tn;
    for (int i = 0; i < n; ++i) yf[i] = b->zn[0][i];
  } else {
    dky_vec(b, tend, yf);
  }
  (void)tstop_final;
  if (g.mode == 1 || g.mode == 4) g.tau = ign_peak_time(&g);
  if (res) {
    res->tau = g.tau;
    res->t_end = tf;
    res->T = yf[0];
    double Wb = mean_wt(m, yf + 1), d;
    if (cfg->problem == 4) {
      engine_volume(cfg->eng, tf, &res->V, NULL);
      res->P = (rho0 * Vstart / res->V) * RU * yf[0] / Wb;
    } else if (cfg->problem == 3) {
      res->P = pfr_pressure(&ctx, tf, tf, yf[0], Wb, &d);
      res->V = ctx.G / (res->P * Wb / (RU * yf[0]));
    } else if (cfg->problem == 1) {
      profile_eval(cfg, tf, tf, ctx.P0, &res->P, &d);
      res->V = rho0 * Vstart / (res->P * Wb / (RU * yf[0]));
    } else {
      profile_eval(cfg, tf, tf, Vstart, &res->V, &d);
      res->P = (rho0 * Vstart / res->V) * RU * yf[0] / Wb;
    }
    res->status = status;
    res->nst = nst;
    res->nfe = ctx.nfe;
    res->nje = ctx.nje;
    res->nlu = b->nlu;
    res->ncf = b->ncf_tot;
    res->nef = b->nef_tot;
  }
  if (Yend)
    for (int k = 0; k < KK; ++k) Yend[k] = yf[1 + k];
  free(b->J);
  free(b->M);
  free(b);
  return status;
}

int cko_reactor_batch(const cko_mech* m, const cko_cfg* cfg, int n, const int* problem, const double* T0,
                      const double* P0, const double* V0, const double* Y0, double* Yend, cko_result* res,
                      int nthreads) {
  const int KK = m->KK;
  int nfail = 0;
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : nfail)
#endif
  for (int i = 0; i < n; ++i) {
    cko_cfg c = *cfg;
    if (problem) c.problem = problem[i];
    int r = cko_reactor(m, &c, T0[i], P0[i], V0 ? V0[i] : 1.0, Y0 + (size_t)i * KK, Yend + (size_t)i * KK,
                        res + i, 0, NULL, NULL, NULL, NULL);
    if (r) nfail++;
  }
  return nfail;
}

int cko_reactor_batch_pert(const cko_mech* m, const cko_cfg* cfg, int n, const int* problem, const double* T0,
                           const double* P0, const double* V0, const double* Y0, const int* pert_rxn,
                           const double* pert_fac, double* Yend, cko_result* res, int nthreads) {
  const int KK = m->KK;
  int nfail = 0;
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : nfail)
#endif
  for (int i = 0; i < n; ++i) {
    cko_cfg c = *cfg;
    if (problem) c.problem = problem[i];
    if (pert_rxn) {
      c.pert_rxn = pert_rxn[i];
      c.pert_fac = pert_fac[i];
    }
    int r = cko_reactor(m, &c, T0[i], P0[i], V0 ? V0[i] : 1.0, Y0 + (size_t)i * KK, Yend + (size_t)i * KK,
                        res + i, 0, NULL, NULL, NULL, NULL);
    if (r) nfail++;
  }
  return nfail;
}
