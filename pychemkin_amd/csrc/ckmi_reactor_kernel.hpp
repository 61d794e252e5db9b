// ckmi_reactor_kernel.hpp -- the wave-per-reactor integrator kernel (KK + 1 <= 64) and its launcher.
// Included by ckmi.hip (closed reactors: CONP, CONV, plug flow, engine) and by ckmi_psr.hip (the open
// well-stirred reactor).  The open-reactor instantiations live in a translation unit of their own so that
// the closed-reactor kernels compile exactly as they do without them: instantiated in one module, the
// optimiser's cross-function decisions (inlining of shared helpers) shifted the closed-reactor kernels'
// spill counts by a few registers (PSR section).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "../../include/ckmi.h"
#include "ckmi_reactor.hpp"
#include "ckmi_run.hpp"
#include "ckmi_internal.hpp"

namespace {
using namespace ckmi;

// Diagnostic build only (-DCKMI_PHASE_TIMERS, scripts/phase_profile.py): per-reactor shader
// cycles spent in each phase, written to a debug buffer no other code reads.
// Slots 8..31 accumulate the cycles spent in each integrator state (RHS, LU, solve excluded).
enum { PH_RHS = 0, PH_JAC = 1, PH_LU = 2, PH_SOLVE = 3, PH_TOTAL = 4, PH_STATE = 8, PH_N = 48 };
#ifdef CKMI_PHASE_TIMERS
__device__ unsigned long long* g_phase_buf = nullptr;
#define PH_T0() const unsigned long long _ph0 = __builtin_amdgcn_s_memtime()
#define PH_ADD(slot) ph[slot] += __builtin_amdgcn_s_memtime() - _ph0
#else
#define PH_T0() (void)0
#define PH_ADD(slot) (void)0
#endif

// ---------------------------------------------------------------- reactor kernel
template <bool PF>
__device__ __forceinline__ void state_PV(const MechView& M, const RunCtx& R, double t, double yl, int lane, double& P,
                                         double& V) {
  const int KK = M.KK;
  const bool isp = lane >= 1 && lane <= KK;
  const double T = bcast(yl, 0);
  const double Wb = 1.0 / wave_sum(isp ? yl * M.rwt()[lane - 1] : 0.0);
  double d;
  if (PF && R.pfr == 2) {
    engine_volume(R.cfg->eng, t, V, d);
    P = (R.rho0 * R.V0 / V) * RU * T / Wb;
  } else if (PF && R.pfr == 1) {
    P = pfr_pressure(R.cfg, R.npv, R.G, R.Pm, t, t, T, Wb, d);
    V = R.G / (P * Wb / (RU * T));  // velocity
  } else if (R.conp) {
    profile_eval(R.cfg, R.npv, t, t, R.P0, P, d);
    const double rho = P * Wb / (RU * T);
    V = R.rho0 * R.V0 / rho;
  } else {
    profile_eval(R.cfg, R.npv, t, t, R.V0, V, d);
    const double rho = R.rho0 * R.V0 / V;
    P = rho * RU * T / Wb;
  }
}

// Persistent reactor kernel: one workgroup of RWAVES waves per CU slot.  The workgroup stages
// the mechanism image into LDS once; each wave then pulls reactor indices from an HBM work
// counter until the batch is exhausted (dynamic balancing: step counts differ by 10x across a
// T0 / phi / P sweep).  No workgroup barrier after staging, so waves run independently.
//
// The integrator (CVODE-style variable-order BDF with modified Newton, control flow identical
// to oracle/ckoracle.c) is written as a wave-uniform state machine whose only RHS evaluation,
// factorisation and solve each appear ONCE in the loop: the explicit inverse of M = I - gamma J
// then stays in VGPRs for the life of the wave.
// Waves per workgroup by Newton-matrix form: 12 (3 per SIMD) with the FP32-stored inverse, whose
// 54 VGPRs leave room for a third wave per SIMD within 168 VGPRs (+16 % reactors/s on configs[2]
// over 8 waves with the FP64 inverse, MI355X, although the 168-VGPR allocation spills ~28 values
// per step to scratch); 8 (2 per SIMD) with the FP64 inverse (256 VGPRs).
__host__ __device__ constexpr int rwaves(bool f64) { return f64 ? 8 : 12; }
// PL: the mechanism has PLOG / chemically activated / general reactions; F64: FP64-stored inverse.
// Plug flow (problem 3) is compiled into the FP64-inverse variants only (PF = F64): its branches
// cost the FP32-inverse variant, the configs[2] kernel, 12 B of scratch per lane and 0.5 % of its
// rate.  sel: 0 integrate every reactor, 1 skip the plug-flow reactors, 2 only those (the host
// pairs a sel 1 launch of an FP32-inverse variant with a sel 2 launch of an FP64 one), 3 those and the reactors
// the sel 1 launch before it gave up on with repeated error-test or convergence failures (N = 64 variants only:
// near equilibrium, at steps of 1e-2 s and more, the FP32-stored inverse of the tracer mechanisms' Newton matrix
// no longer contracts the iteration; the FP64 one integrates the same reactors, tests/test_gpu_size_variants.py).
enum { SEL_ALL = 0, SEL_NO_PFR = 1, SEL_PFR = 2, SEL_PFR_RETRY = 3 };
// sel of the FP64-inverse launch of a WavePlan (ckmi_dispatch.hpp)
constexpr int f64_sel(int takes) {
  return takes == F64_TAKES_ALL ? SEL_ALL : (takes == F64_TAKES_PFR ? SEL_PFR : SEL_PFR_RETRY);
}
// PSR: the open well-stirred reactor (problem 5, ckmi_psr_run) instead of the closed ones: every reactor of
// the launch is a PSR, io is a PsrIO, the wave's slice ends with one more [VL] vector (the inlet mass
// fractions), and the run ends at the first steady state.  A compile-time flag of three FP64-inverse
// instantiations; the closed-reactor instantiations compile to the code they had without it.
//   steady-state rule   after an accepted step a fresh f at the new state must satisfy
//                       tau |f_k| <= ss_rtol |Y_k| + ss_atol for every species and tau |f_T| <= ss_rtol T
//                       (tau the current residence time); the BDF history's zn[1] / h screens the steps on
//                       which the extra f is paid for
//   polish              a state close to the rule but above it takes Newton steps on f = 0 with the Newton
//                       matrix in registers: M^-1 gamma f = (I / gamma - J)^-1 f, an implicit Euler step
//                       of size gamma from the state; the integration goes on from the BDF history if they
//                       stop contracting
// Ctl fields the open reactor has no other use for hold its scalars: nadap (polish iterations), delp
// (residual of the previous iterate), avar_last (the returned residual).
constexpr double PSR_SCREEN = 100.0, PSR_POLISH_MAX = 1e6, PSR_POLISH_RATE = 0.7;
constexpr int PSR_POLISH_ITERS = 12;
template <int N, bool PL = false, bool F64 = false, bool PSR = false>
__global__ __launch_bounds__(rwaves(F64)* WAVE) void reactor_kernel(MechImage img, const DevCfg* __restrict__ dcfg,
                                                               int nreact, int sel, int* __restrict__ queue,
                                                               double* __restrict__ jws,
                                                               std::conditional_t<PSR, PsrIO, ReactorIO> io) {
  static_assert(!PSR || F64, "the open reactor is compiled into FP64-inverse variants only");
  constexpr bool PF = F64;
  const ckmi_reactor_cfg* __restrict__ cfg = &dcfg->c;
  const int oJ = img.bytes;
  const int olock = oJ + jlock_offset(N);  // where reactor_rhs<..., LOCK> looks for it
  if (threadIdx.x == 0) *lds_at<int>(olock) = 0;
  stage_image(0, img);
  const MechView V = make_view(0, img);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int ows = oJ + jscratch_bytes<N>() + wid * (slice_bytes(img.G) + (PSR ? 8 * VL : 0));
  WaveLds L;
  L.base = ows;
  double* const Yin = PSR ? lds_at<double>(ows + slice_bytes(img.G)) : nullptr;  // inlet mass fractions [VL]
  const int oS = ows + slice_vec_bytes(img.G);
  BdfS& S = *lds_at<BdfS>(oS);
  Ctl& c = *lds_at<Ctl>(oS + align16((int)sizeof(BdfS)));
  Ign& g = *lds_at<Ign>(oS + align16((int)sizeof(BdfS)) + align16((int)sizeof(Ctl)));
  // the wave's parked Jacobian, rounded to FP32: M = I - gamma J is rebuilt from it at every
  // setup (5.6 per J); the modified Newton iteration only needs an approximate M, and half
  // the bytes keep the slots of an XCD's 256 waves (3.5 MB) within its 4 MB L2
  constexpr int RWAVES = rwaves(F64);
  float* Jg = reinterpret_cast<float*>(jws) + ((size_t)blockIdx.x * RWAVES + wid) * N * WAVE;
  const int KK = V.KK;
  const int n = KK + 1;
  const bool isp = lane >= 1 && lane <= KK;
  const bool act = lane < n;
  // per-reactor constants of the RHS: in LDS, not registers (the Newton matrix owns those)
  RunCtx& R = *lds_at<RunCtx>(oS + align16((int)sizeof(BdfS)) + align16((int)sizeof(Ctl)) + align16((int)sizeof(Ign)));
  R.cfg = cfg;
  std::conditional_t<F64, NewtonMatrixGJ64<N>, NewtonMatrixF32S<N>> M;
  Bdf b;
  b.zn.base = oS + align16((int)sizeof(BdfS)) + align16((int)sizeof(Ctl)) + align16((int)sizeof(Ign)) +
              align16((int)sizeof(RunCtx)) + lane * 8;
  double fe = 0.0, y_e = 0.0, t_e = 0.0;
  bool with_j = false;
#ifdef CKMI_PHASE_TIMERS
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_r0 = 0;
  unsigned long long* phs = lds_at<unsigned long long>(oS + align16((int)sizeof(BdfS)) + align16((int)sizeof(Ctl)) +
                                                     align16((int)sizeof(Ign)) + align16((int)sizeof(RunCtx)) +
                                                     ZN_BYTES);
#endif
  int st = ST_NEXT;

  // request f at (t, y): sets the evaluation point and the state that consumes it
#define REQUEST_F(T_, Y_, NEXT_) \
  do {                           \
    t_e = (T_);                  \
    y_e = (Y_);                  \
    with_j = false;              \
    st = (NEXT_);                \
    want = true;                 \
  } while (0)
  // bdf_start: history at (t, y), then the initial step size (oracle bdf_start)
#define START_BEGIN(T_, Y_, TOUT_, H0_)                                 \
  do {                                                                 \
    S.tn = (T_);                                                       \
    b.zn[0] = act ? (Y_) : 0.0;                                        \
    _Pragma("unroll") for (int j_ = 1; j_ <= QMAX; ++j_) b.zn[j_] = 0.0; \
    b.ewt = act ? 1.0 / (S.rtol * fabs(b.zn[0]) + S.atol) : 0.0;       \
    c.tc = c.st_tout = (TOUT_); /* the step loop's stop point */      \
    R.tsel = 0.5 * (S.tn + c.st_tout);                                 \
    c.st_h0 = (H0_);                                                   \
    REQUEST_F(S.tn, b.zn[0], ST_START_F);                              \
  } while (0)

  // open reactor: the largest scaled residual of the steady-state rule for f at the state y (lane-wise)
  auto psr_resid = [&](double f, double y) -> double {
    if constexpr (PSR) {
      const double T = bcast(y, 0);
      const double sYW = wave_sum(isp ? y * V.rwt()[lane - 1] : 0.0);
      const double tau = R.pfr == 4 ? R.P0 / (RU * T * sYW * R.G) : 1.0 / R.G;  // rho V / mdot
      const double den = lane == 0 ? io.ss_rtol * T : io.ss_rtol * fabs(y) + io.ss_atol;
      const double v = act ? tau * fabs(f) / den : 0.0;
      // a NaN anywhere must fail the rule (a max reduction would drop it)
      return __ballot(act && !(v == v)) != 0 ? __builtin_nan("") : wave_max(v);
    } else {
      return 0.0;
    }
  };

  for (;;) {
    bool want = false;
    while (!want && st != ST_EXIT) {
#ifdef CKMI_PHASE_TIMERS
      const int st_in = st;
      const unsigned long long t_st = __builtin_amdgcn_s_memtime();
#endif
      if constexpr (PSR) {
        if (st == ST_FINISH && c.stopped == 0) {
          // a run that ends without a steady state (t_max, solver failure): the residual of the state it
          // returns (after a failed step the history is back at the last accepted state)
          c.stopped = 2;
          REQUEST_F(S.tn, b.zn[0], ST_PSR_END_F);
          continue;
        }
        if (st > ST_EXIT) {
          S.nfe++;
          const double res = psr_resid(fe, y_e);
          if (st == ST_PSR_END_F) {
            c.avar_last = res;
            if (c.status == 0 && !(res <= 1.0)) c.status = CKMI_RUN_NOT_STEADY;
            st = ST_FINISH;
            continue;
          }
          const bool polishing = st == ST_PSR_POLISH_F;
          if (res <= 1.0) {
            if (polishing) b.zn[0] = b.y;  // the run ends here: the history is not used again
            c.avar_last = res;
            c.stopped = 1;
            st = ST_FINISH;
            continue;
          }
          if (polishing ? (c.nadap < PSR_POLISH_ITERS && res < PSR_POLISH_RATE * c.delp) : res <= PSR_POLISH_MAX) {
            c.nadap = polishing ? c.nadap + 1 : 1;
            c.delp = res;
            const double d = M.solve(act ? S.gammap * fe : 0.0, n);
            S.nni++;
            b.y = act ? y_e + d : 0.0;
            REQUEST_F(S.tn, b.y, ST_PSR_POLISH_F);
            continue;
          }
          st = ST_STEP_BEGIN;  // not steady yet (the polished iterates are dropped): integrate on
          continue;
        }
      }
      switch (st) {
        case ST_NEXT: {
          int r = 0;
          if (lane == 0) r = atomicAdd(queue, 1);
          r = uni(bcast(r, 0));
          if (r >= nreact) {
            st = ST_EXIT;
            break;
          }
          int prob;
          if constexpr (PSR) prob = 5;
          else prob = io.problem[r];
          // plug flow (3) and engines (4) run in the FP64-inverse launch
          if (PF ? (sel == SEL_PFR && prob < 3) : prob >= 3) break;  // the other launch's reactor
          if constexpr (PF && !PSR && N == 64) {
            if (sel == SEL_PFR_RETRY && prob < 3) {  // its status is final unless the FP32 inverse was the cause
              const int s32 = io.stats[(size_t)r * CKMI_NSTAT + CKMI_STAT_STATUS];
              if (s32 != CKMI_RUN_ERRTEST && s32 != CKMI_RUN_CONVFAIL) break;
            }
          }
          c.r = r;
          // TPRO runs start at the profile's initial temperature
          const double T0 = (cfg->prof_kind == 1 && cfg->energy == 2 && cfg->nprof > 0) ? cfg->prof_v[0] : io.T0[r];
          const double P0 = io.P0[r];
          double yl = 0.0;
          if (lane == 0) yl = T0;
          if (isp) yl = io.Y0[(size_t)r * KK + lane - 1];
          const double Wbar0 = 1.0 / wave_sum(isp ? yl * V.rwt()[lane - 1] : 0.0);
          if (dcfg->npe) {  // initial element contents: the element projection's target
            const uint64_t cnt = isp ? elem_table(V)[lane - 1] : 0ull;
            const double rw = isp ? V.rwt()[lane - 1] : 0.0;
            double v[PROJ_MMAX];
#pragma unroll
            for (int e = 0; e < PROJ_MMAX; ++e) v[e] = elem_coef(cnt, rw, e) * yl;
            wave_sum_multi<PROJ_MMAX>(v, lane);
#pragma unroll
            for (int e = 0; e < PROJ_MMAX; ++e) c.eb0[e] = v[e];
          }
          R.pfr = PF ? (prob == 3 ? 1 : (prob == 4 ? 2 : 0)) : 0;
          R.conp = (prob == 1 || prob == 3);
          R.energy = cfg->energy;
          R.npv = cfg->prof_kind == 0 ? cfg->nprof : 0;
          R.ntp = (cfg->prof_kind == 1 && cfg->energy == 2) ? cfg->nprof : 0;
          R.rho0 = P0 * Wbar0 / (RU * T0);
          R.V0 = (!R.conp && R.npv > 0) ? cfg->prof_v[0] : io.V0[r];
          R.P0 = (R.conp && R.npv > 0) ? cfg->prof_v[0] : P0;
          if constexpr (PF) {
            if (R.pfr == 2) {  // engine: V0 from the crank position at t = 0; gamma (G), T (Pm) of the charge
              double dv;
              engine_volume(cfg->eng, 0.0, R.V0, dv);
              const double cpR = isp ? nasa7_img(V, lane - 1, T0, log(T0), 1.0 / T0).cpR : 0.0;
              const double cpm = wave_sum(isp ? yl * cpR * V.rwt()[lane - 1] : 0.0);
              R.G = cpm / (cpm - 1.0 / Wbar0);
              R.Pm = T0;
            }
          }
          R.mass = R.rho0 * R.V0;
          if (PF && R.pfr == 1) {  // plug flow: V0 is the inlet velocity u0 [cm/s]
            R.G = R.rho0 * R.V0;  // mdot / A: the inlet density (inlet pressure) x u0, with or without PPRO
            R.Pm = R.P0 + R.G * R.V0;
          }
          if constexpr (PSR) {  // io.V0 is tau_or_vol: R.V0 holds it
            const bool vgiven = io.mode == 2;
            R.conp = 1;
            R.pfr = vgiven ? 4 : 3;
            const double Tin = io.Tin[r], mdot = io.mdot[r];
            const double yi = isp ? io.Yin[(size_t)r * KK + lane - 1] : 0.0;
            if (isp) Yin[lane - 1] = yi;
            const double hin = isp ? nasa7_img(V, lane - 1, Tin, log(Tin), 1.0 / Tin).hRT * RU * Tin * V.rwt()[lane - 1] : 0.0;
            R.Pm = wave_sum(yi * hin);
            R.G = vgiven ? mdot / R.V0 : 1.0 / R.V0;
            R.mass = vgiven ? R.rho0 * R.V0 : R.V0 * mdot;
            wave_lds_sync();
          }
          R.gfac = cfg->gfac;
          R.qloss = cfg->qloss;
          R.htc = cfg->htc;
          R.areaq = cfg->areaq;
          R.tamb = cfg->tamb;
          R.nq = cfg->prof2_kind == 1 ? cfg->nprof2 : 0;
          R.na = cfg->prof2_kind == 2 ? cfg->nprof2 : cfg->nprof3;
          R.a_t = cfg->prof2_kind == 2 ? cfg->prof2_t : cfg->prof3_t;
          R.a_v = cfg->prof2_kind == 2 ? cfg->prof2_v : cfg->prof3_v;
          {
            const int ar = io.afac_rxn ? io.afac_rxn[r] : -1;
            R.pslot = (ar >= 0 && ar < img.II) ? img.slot_of[ar] : -1;
            R.plnf = R.pslot >= 0 ? log(io.afac[r]) : 0.0;
          }
          c.nadap = 0;
          c.avar_last = bcast(yl, cfg->avar > 0 ? cfg->avar : 0);
          c.T0 = T0;
          c.yguard = dcfg->guard_y;
          c.tguard_lo = dcfg->guard_tlo;
          c.tguard_hi = dcfg->guard_thi;
          S.rtol = cfg->rtol;
          S.atol = cfg->atol;
          S.nneg = cfg->nneg;
          S.ncf_tot = S.nef_tot = S.nlu = S.nfe = S.nje = S.nni = 0;
          c.tend = cfg->t_end;
          if constexpr (PSR) {  // t_max: 1000 residence times (of the estimate, when the volume is given)
            if (!(c.tend > 0.0)) c.tend = 1000.0 * (R.pfr == 4 ? R.rho0 / R.G : 1.0 / R.G);
          }
          c.hmax = cfg->hmax > 0.0 ? cfg->hmax : c.tend / 100.0;
          S.hmax_inv = 1.0 / c.hmax;
          S.hmin = 0.0;
          c.ncrit = n_crit(dcfg);
          c.icrit = 0;
          c.first = 1;
          c.max_steps = cfg->max_steps > 0 ? cfg->max_steps : 200000;
          c.flags = (dcfg->ncrit > 0 ? SF_CRIT : 0) | (cfg->ign_stop ? SF_IGN_STOP : 0) | (io.nsave > 0 ? SF_SAVE : 0) |
                    (io.n_adap ? SF_ADAP : 0) | (cfg->asteps > 0 ? SF_ASTEPS : 0) | (cfg->avar >= 0 ? SF_AVAR : 0) |
                    (dcfg->npe << SF_NPE_SHIFT);
#ifdef CKMI_PHASE_TIMERS
#pragma unroll
          for (int k = 0; k < 8; ++k) ph[k] = 0;
          if (lane < 40) phs[lane] = 0;
          t_r0 = __builtin_amdgcn_s_memtime();
#endif
          START_BEGIN(0.0, yl, crit_time(dcfg, c.tend, 0), cfg->h0);
          break;
        }
        case ST_START_F: {
          b.zn[1] = act ? fe : 0.0;
          S.nfe++;
          if (c.st_h0 > 0.0) {
            c.st_h = c.st_h0;
            st = ST_START_FINISH;
            break;
          }
          // initial step estimate (oracle bdf_initial_step)
          const double t0 = S.tn, tout = c.st_tout;
          const double tdist = fabs(tout - t0);
          const double tround = UROUND * fmax(fabs(t0), fabs(tout));
          const double hlb = 100.0 * tround;
          double hub = 0.1 * tdist;
          const double num = act ? fabs(b.zn[1]) : 0.0;
          const double den = 0.1 * fabs(b.zn[0]) + S.atol;
          const double hub_inv = wave_max(act ? num / (den > 0 ? den : 1e-300) : 0.0);
          if (hub * hub_inv > 1.0) hub = 1.0 / hub_inv;
          const double hg = sqrt(hlb * hub);
          if (hub < hlb) {
            c.st_h = hg;
            st = ST_START_FINISH;
            break;
          }
          c.is_t0 = t0;
          c.is_hg = hg;
          c.is_hub = hub;
          c.is_hlb = hlb;
          c.is_count = 1;
          REQUEST_F(t0 + hg, b.zn[0] + hg * b.zn[1], ST_INITSTEP_F);
          break;
        }
        case ST_INITSTEP_F: {
          S.nfe++;
          const double hg = c.is_hg, hub = c.is_hub;
          const double f1 = act ? (fe - b.zn[1]) / hg : 0.0;
          const double yddnrm = wrms_lane(f1, b.ewt, n);
          double hnew = (yddnrm * hub * hub > 2.0) ? sqrt(2.0 / yddnrm) : sqrt(hg * hub);
          bool done = c.is_count == 4;
          if (!done) {
            const double hrat = hnew / hg;
            if (hrat > 0.5 && hrat < 2.0) {
              done = true;
            } else if (c.is_count >= 2 && hrat > 2.0) {
              hnew = hg;
              done = true;
            }
          }
          if (!done) {
            c.is_hg = hnew;
            c.is_count++;
            REQUEST_F(c.is_t0 + hnew, b.zn[0] + hnew * b.zn[1], ST_INITSTEP_F);
            break;
          }
          double h0 = 0.5 * hnew;
          if (h0 < c.is_hlb) h0 = c.is_hlb;
          if (h0 > hub) h0 = hub;
          c.st_h = h0;
          st = ST_START_FINISH;
          break;
        }
        case ST_START_FINISH: {
          double h = c.st_h;
          if (h > c.hmax) h = c.hmax;
          if (h > c.st_tout - S.tn) h = c.st_tout - S.tn;
          b.zn[1] *= h;
          S.h = S.hscale = S.hprime = h;
          S.q = S.qprime = 1;
          S.L = 2;
          S.qwait = S.L;
          S.etamax = ETAMX1;
          S.nst = 0;
          S.nstlp = 0;
          S.nstlj = 0;
          S.jcur = 0;
          S.crate = 1.0;
          S.gammap = S.gamma = S.h;
          S.gamrat = 1.0;
          S.saved_tq5 = 0.0;
#pragma unroll
          for (int i = 0; i <= QMAX + 1; ++i) S.tau[i] = 0.0;
#pragma unroll
          for (int i = 0; i < 6; ++i) S.tq[i] = 0.0;
          S.hu = 0.0;
          st = ST_STEP_BEGIN;
          if (c.first) {
            c.first = 0;
            g.mode = cfg->ign_mode;
            g.comp = (g.mode == 4) ? 1 + cfg->ign_species : 0;
            g.found = g.started = g.have_prev = g.have_next = 0;
            g.thresh = 0.0;
            g.best = -1e300;
            g.tbest = g.tprev = g.vprev = g.tnext = g.vnext = g.tlast = g.vlast = 0.0;
            g.tau = -1.0;
            if (g.mode == 2) g.thresh = c.T0 + cfg->ign_val;
            if (g.mode == 3) g.thresh = cfg->ign_val;
            c.isave = 0;
            while (c.isave < io.nsave && io.t_save[c.isave] <= 0.0) {
              if (act) io.y_save[((size_t)c.r * io.nsave + c.isave) * n + lane] = b.zn[0];
              c.isave++;
            }
            c.status = 0;
            c.nst = 0;
            c.stopped = 0;
            if (g.mode == 1 || g.mode == 4) REQUEST_F(0.0, b.zn[0], ST_IGN0_F);
          }
          break;
        }
        case ST_IGN0_F: {
          S.nfe++;
          ign_peak_update(g, 0.0, g.mode == 1 ? bcast(fe, 0) : bcast(b.zn[0], g.comp));
          st = ST_STEP_BEGIN;
          break;
        }
        case ST_STEP_BEGIN: {
          // one batch of independent reads (c.tc is crit_time(dcfg, c.tend, c.icrit): set where icrit is, in
          // START_BEGIN, not asked of dcfg per step)
          const double tn = S.tn, tend = c.tend, tc = c.tc, h = S.h, rtol = S.rtol, atol = S.atol, z0 = b.zn[0];
          double hprime = S.hprime;
          const int nst = S.nst, q = S.q, qprime = S.qprime;
          if (!(tn < tend * (1.0 - 1e-15))) {
            st = ST_FINISH;
            break;
          }
          if (tn + hprime > tc) {
            const double hp = tc - tn;
            S.eta = hp / h;
            if (nst > 0) {
              hprime = hp;
              S.hprime = hp;
            } else {
              bdf_rescale(b, S);
              S.hprime = S.h;
            }
          }
          b.ewt = act ? 1.0 / (rtol * fabs(z0) + atol) : 0.0;
          c.told = tn;
          c.saved_t = tn;
          c.ncf = c.nef = 0;
          c.nflag = NF_FIRST;
          if (nst > 0 && hprime != h) {  // (at nst == 0 the clip above leaves hprime == h)
            if (qprime != q) {
              bdf_adjust_order(b, S, qprime - q);
              S.q = qprime;
              S.L = qprime + 1;
              S.qwait = qprime + 1;
            }
            bdf_rescale(b, S);
          }
          st = ST_STEP_ATTEMPT;
          break;
        }
        case ST_STEP_ATTEMPT: {
          bdf_predict(b, S);
          bdf_set(b, S);
          {  // every input read at once; the tests combine without short-circuit branches
            const int nflag = c.nflag, nst = S.nst, nstlp = S.nstlp;
            const double gamrat = S.gamrat;
            c.convfail = (nflag == NF_FIRST || nflag == NF_ERR_FAIL) ? CF_NONE : CF_OTHER;
            c.call_setup = (nflag != NF_FIRST) | (nst == 0) | (nst >= nstlp + MSBP) | (fabs(gamrat - 1.0) > DGMAX);
          }
          st = ST_NLS_ATTEMPT;
          break;
        }
        case ST_NLS_ATTEMPT: {
          b.y = b.zn[0];
          // a stale Jacobian (oracle nls_setup's jbad: none of its inputs depends on f) is decided here, so
          // that f and J of the point come from ONE evaluation, its reactions visited once
          if (c.call_setup) {
            const int nst = S.nst, nstlj = S.nstlj, convfail = c.convfail;
            const double dgamma = fabs(S.gamma / S.gammap - 1.0);
            const int jbad = (nst == 0) | (nst >= nstlj + MSBJ) | ((convfail == CF_BAD_J) & (dgamma < DGMAX)) |
                             (convfail == CF_OTHER);
            if (jbad) {
              // the with_j call takes the lock of the workgroup's J scratch itself, behind its prologue
              // (reactor_rhs<..., LOCK>), and returns holding it; ST_NLS_J -- the state this request sets, which
              // nothing between here and there changes: the call has no early exit, and the loop around the
              // switch dispatches on st alone -- copies J out and releases it, unconditionally
              REQUEST_F(S.tn, b.y, ST_NLS_J);
              with_j = true;
              break;
            }
          }
          REQUEST_F(S.tn, b.y, ST_NLS_F);
          break;
        }
        case ST_NLS_F: {
          b.ftemp = fe;
          S.nfe++;
          if (!c.call_setup) {
            b.acor = 0.0;
            c.delp = 0.0;
            c.mm = 0;
            st = ST_NEWTON_ITER;
            break;
          }
          S.jcur = 0;  // a set-up with the parked Jacobian (ST_NLS_ATTEMPT found it still good)
          st = ST_SETUP;
          break;
        }
        case ST_NLS_J: {
          b.ftemp = fe;  // f of the same evaluation
          {
            const double* Jsh = lds_at<const double>(oJ);
#pragma unroll 2
            for (int j = 0; j < N; ++j) Jg[j * WAVE + lane] = (float)Jsh[j * LDJ + lane];
          }
          wave_lds_sync();
          if (lane == 0) atomicExch(lds_at<int>(olock), 0);
          S.nfe += 2;  // as the oracle counts a Jacobian event: the step's f and the Jacobian's own evaluation
          S.nje++;
          S.nstlj = S.nst;
          S.jcur = 1;
          st = ST_SETUP;
          break;
        }
        case ST_SETUP: {
#ifdef CKMI_PHASE_TIMERS
          const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
          // each lane reads back only the J entries it wrote itself (same-address order); the
          // dwdT row of the slice (free here) is the pivot-row scratch
          const bool ok = M.build_factor(Jg, WAVE, S.gamma, n, L.base + 32 * VL);
#ifdef CKMI_PHASE_TIMERS
          ph[PH_LU] += __builtin_amdgcn_s_memtime() - t0;
#endif
          S.nlu++;
          S.crate = 1.0;
          S.gammap = S.gamma;
          S.gamrat = 1.0;
          S.nstlp = S.nst;
          if (!ok) {
            st = ST_STEP_CONVFAIL;
            break;
          }
          b.acor = 0.0;
          c.delp = 0.0;
          c.mm = 0;
          st = ST_NEWTON_ITER;
          break;
        }
        case ST_NEWTON_ITER: {
          const double rhs = act ? S.gamma * b.ftemp - (S.rl1 * b.zn[1] + b.acor) : 0.0;
#ifdef CKMI_PHASE_TIMERS
          const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
          double x = M.solve(rhs, n);
#ifdef CKMI_PHASE_TIMERS
          ph[PH_SOLVE] += __builtin_amdgcn_s_memtime() - t0;
#endif
          // one batch of independent reads behind the solve (nothing of it lives across the solve)
          const double gamrat = S.gamrat, crate0 = S.crate, tq4 = S.tq[4], delp = c.delp, z0 = b.zn[0];
          const int nneg = S.nneg, mm = c.mm;
          S.nni++;
          if (gamrat != 1.0) x *= 2.0 / (1.0 + gamrat);
          if (!act) x = 0.0;
          // the iteration's norms in one fused reduction (oracle nls: the same quantities): the correction
          // (del), the accumulated correction (acnrm), NNEG's negative part and acnrm after NNEG's clipping
          b.acor += x;
          b.y = z0 + b.acor;
          const bool neg = nneg && act && lane >= 1 && b.y < 0.0;
          double nv[4];
          {
            const double xe = x * b.ewt, ae = b.acor * b.ewt, ne = neg ? b.y * b.ewt : 0.0;
            const double fe2 = neg ? z0 * b.ewt : ae;
            nv[0] = xe * xe;
            nv[1] = ae * ae;
            nv[2] = ne * ne;
            nv[3] = fe2 * fe2;
          }
          wave_sum_multi<4>(nv, lane);
          const double del = sqrt(nv[0] / n);
          double crate = crate0;
          if (mm > 0) {
            crate = fmax(CRDOWN * crate0, del / delp);
            S.crate = crate;
          }
          const double dcon = del * fmin(1.0, crate) / tq4;
          if (dcon <= 1.0) {
            bool negfail = false, negfix = false;
            if (nneg && nv[2] > 0.0) {
              if (sqrt(nv[2] / n) > NNEG_TOL) {
                negfail = true;
              } else {
                negfix = true;
                if (neg) {
                  b.y = 0.0;
                  b.acor = -z0;
                }
              }
            }
            if (negfail) {
              c.failed = 2;
              st = ST_NLS_FAIL;
              break;
            }
            S.acnrm = (mm == 0 && !negfix) ? del : sqrt((negfix ? nv[3] : nv[1]) / n);
            S.jcur = 0;
            st = ST_ERRTEST;
            break;
          }
          c.mm = mm + 1;
          if (mm + 1 == MAXCOR || (mm + 1 >= 2 && del > RDIV * delp)) {
            c.failed = 1;
            st = ST_NLS_FAIL;
            break;
          }
          c.delp = del;
          REQUEST_F(S.tn, b.y, ST_NEWTON_F);
          break;
        }
        case ST_NEWTON_F: {
          b.ftemp = fe;
          S.nfe++;
          st = ST_NEWTON_ITER;
          break;
        }
        case ST_NLS_FAIL: {
          if (c.failed == 1 && !S.jcur) {
            c.convfail = CF_BAD_J;
            c.call_setup = 1;
            st = ST_NLS_ATTEMPT;
          } else {
            st = ST_STEP_CONVFAIL;
          }
          break;
        }
        case ST_STEP_CONVFAIL: {
          c.ncf++;
          S.ncf_tot++;
          S.etamax = 1.0;
          bdf_restore(b, S, c.saved_t);
          if (fabs(S.h) <= S.hmin * ONEPSM || c.ncf == MXNCF) {
            c.rc = CKMI_RUN_CONVFAIL;
            st = ST_STEP_END;
            break;
          }
          S.eta = fmax(ETACF, S.hmin / fabs(S.h));
          c.nflag = NF_CONV_FAIL;
          bdf_rescale(b, S);
          st = ST_STEP_ATTEMPT;
          break;
        }
        case ST_ERRTEST: {
          c.dsm = S.acnrm * S.tq[2];
          if (c.dsm <= 1.0) {
            st = ST_STEP_COMPLETE;
            break;
          }
          c.nef++;
          S.nef_tot++;
          c.nflag = NF_ERR_FAIL;
          bdf_restore(b, S, c.saved_t);
          if (fabs(S.h) <= S.hmin * ONEPSM || c.nef == MXNEF) {
            c.rc = CKMI_RUN_ERRTEST;
            st = ST_STEP_END;
            break;
          }
          S.etamax = 1.0;
          st = ST_STEP_ATTEMPT;
          if (c.nef <= MXNEF1) {
            S.eta = 1.0 / (eta_root(BIAS2 * c.dsm, S.L) + ADDON);
            S.eta = fmax(ETAMIN, fmax(S.eta, S.hmin / fabs(S.h)));
            if (c.nef >= SMALL_NEF) S.eta = fmin(S.eta, ETAMXF);
            bdf_rescale(b, S);
            break;
          }
          if (S.q > 1) {
            S.eta = fmax(ETAMIN, S.hmin / fabs(S.h));
            bdf_adjust_order(b, S, -1);
            S.L = S.q;
            S.q--;
            S.qwait = S.L;
            bdf_rescale(b, S);
            break;
          }
          S.eta = fmax(ETAMIN, S.hmin / fabs(S.h));
          S.h *= S.eta;
          S.hscale = S.h;
          S.qwait = LONG_WAIT;
          REQUEST_F(S.tn, b.zn[0], ST_ERR_F);
          break;
        }
        case ST_ERR_F: {
          S.nfe++;
          b.zn[1] = act ? S.h * fe : 0.0;
          st = ST_STEP_ATTEMPT;
          break;
        }
        case ST_STEP_COMPLETE: {
          // one batch of independent reads; the decisions run on locals, the changed fields are stored once
          const double dsm = c.dsm, h = S.h, etamax = S.etamax, hmax_inv = S.hmax_inv, tq5 = S.tq[5];
          double saved_tq5 = S.saved_tq5;
          const int q = S.q, Lq = S.L, nst = S.nst + 1, fl = c.flags;
          int qwait = S.qwait;
          S.nst = nst;
          c.nst++;
          S.hu = h;
          const double tau2 = bdf_tau_shift(S, q, nst, h);
          // the q - 1 and q + 1 error norms of a step that selects the next order (qwait reaches 0 below), from
          // the corrector before the element projection (oracle bdf_step), in one fused 2-value reduction
          double ddn = 0.0, dup = 0.0;
          if (etamax != 1.0 && qwait == 1) {
            const bool qm = q > 1, qp = q != QMAX && saved_tq5 != 0.0;
            const double tq1 = S.tq[1], tq3 = S.tq[3];
            double cquot = 0.0;
            if (qp) {
              const double hr = h / tau2;
              double hrL = hr;
              for (int j = 1; j < Lq; ++j) hrL *= hr;
              cquot = (tq5 / saved_tq5) * hrL;
            }
            double ov[2];
            {
              // zn[q] and l[q]: every entry read, the order selects (scalars, not arrays: a select chain over
              // a local array folds into a dynamically indexed stack slot)
              double znq = 0.0, lq = 0.0, znQ = 0.0;
#pragma unroll
              for (int j = 0; j <= QMAX; ++j) {
                const double zj = b.zn[j], lj = S.l[j];
                znq = (j == q) ? zj : znq;
                lq = (j == q) ? lj : lq;
                if (j == QMAX) znQ = zj;
              }
              const double a = (act && qm) ? (znq + lq * b.acor) * b.ewt : 0.0;
              const double t = (act && qp) ? (b.acor - cquot * znQ) * b.ewt : 0.0;
              ov[0] = a * a;
              ov[1] = t * t;
            }
            wave_sum_multi<2>(ov, lane);
            ddn = sqrt(ov[0] / n) * tq1;
            dup = sqrt(ov[1] / n) * tq3;
          }
          // element conservation held to PROJ_TOL rtol (oracle elem_project), before the history update
          if (const int npe = fl >> SF_NPE_SHIFT) elem_project_wave(V, npe, c.eb0, S.rtol, b.zn[0], b.acor, lane, L.ek());
          qwait--;
          const bool park = qwait == 1 && q != QMAX;
          bdf_correct_history(b, S, q, park);
          if (park) saved_tq5 = tq5;
          double eta, hprime;
          int qprime = q;
          if (etamax == 1.0) {
            if (qwait < 2) qwait = 2;
            hprime = h;
            eta = 1.0;
          } else {
            const double etaq = 1.0 / (eta_root(BIAS2 * dsm, Lq) + ADDON);
            if (qwait != 0) {
              eta = etaq;
            } else {
              qwait = 2;
              double etaqm1 = 0.0, etaqp1 = 0.0;
              if (q > 1) etaqm1 = 1.0 / (eta_root(BIAS1 * ddn, q) + ADDON);
              if (q != QMAX && saved_tq5 != 0.0) etaqp1 = 1.0 / (eta_root(BIAS3 * dup, Lq + 1) + ADDON);
              const double etam = fmax(etaqm1, fmax(etaq, etaqp1));
              if (etam < THRESH) {
                eta = 1.0;
              } else if (etam == etaq) {
                eta = etaq;
              } else if (etam == etaqm1) {
                eta = etaqm1;
                qprime = q - 1;
              } else {
                eta = etaqp1;
                qprime = q + 1;
                b.zn[QMAX] = b.acor;
              }
            }
            if (eta < THRESH) {
              eta = 1.0;
              hprime = h;
            } else {
              eta = fmin(eta, etamax);
              eta /= fmax(1.0, fabs(h) * hmax_inv * eta);
              hprime = h * eta;
            }
          }
          S.qwait = qwait;
          S.saved_tq5 = saved_tq5;
          S.qprime = qprime;
          S.hprime = hprime;
          S.eta = eta;
          S.etamax = (nst <= SMALL_NST) ? ETAMX2 : ETAMX3;
          {  // runaway guard on the accepted state: a mass fraction far below 0, or T off the thermo range
             // (energy runs); it ends the reactor through ST_STEP_END's failure exit
            // (one ballot, not a max reduction: only "any lane beyond the guard" matters)
            const double z0 = b.zn[0];
            const bool bad = isp ? -z0 > c.yguard
                                 : (lane == 0 && R.energy == 1 && !(z0 >= c.tguard_lo && z0 <= c.tguard_hi));
            c.rc = __ballot(bad) != 0 ? CKMI_RUN_RUNAWAY : 0;
          }
          if constexpr (PF) {  // plug flow past the choke point of the momentum equation (pfr_pressure)
            if (R.pfr == 1 && R.npv == 0 && c.rc == 0) {
              const double z0 = b.zn[0];
              const double sYW = wave_sum(isp ? z0 * V.rwt()[lane - 1] : 0.0);
              if (R.Pm * R.Pm - 4.0 * R.G * R.G * RU * bcast(z0, 0) * sYW < 0.0) c.rc = CKMI_RUN_CHOKED;
            }
          }
          st = ST_STEP_END;
          break;
        }
        case ST_STEP_END: {
          // one batch of independent reads for the common path
          const int rc = c.rc, fl = c.flags, gmode = g.mode, nst = c.nst, max_steps = c.max_steps;
          const double tn = S.tn;
          if (rc != 0) {
            c.status = rc;
            st = ST_FINISH;
            break;
          }
          if (fl & SF_SAVE) {
            while (c.isave < io.nsave && io.t_save[c.isave] <= tn) {
              const double ys = dky0_lane(b, S, io.t_save[c.isave]);
              if (act) io.y_save[((size_t)c.r * io.nsave + c.isave) * n + lane] = ys;
              c.isave++;
            }
          }
          if (gmode == 1) {
            ign_peak_update(g, tn, bcast(b.zn[1], 0) / S.h);
          } else if (gmode == 4) {
            ign_peak_update(g, tn, bcast(b.zn[0], g.comp));
          } else if ((gmode == 2 || gmode == 3) && !g.found && bcast(b.zn[0], 0) >= g.thresh) {
            double lo = c.told, hi = tn;
            for (int it = 0; it < 60; ++it) {
              const double mid = 0.5 * (lo + hi);
              if (bcast(dky0_lane(b, S, mid), 0) >= g.thresh) hi = mid;
              else lo = mid;
            }
            g.found = 1;
            g.tau = hi;
          }
          st = ST_STEP_BEGIN;
          if (fl & SF_IGN_STOP) {
            if ((gmode == 2 || gmode == 3) && g.found) {
              c.stopped = 1;
              st = ST_FINISH;
              break;
            }
            if (gmode == 1 && g.have_next && g.vlast < 0.1 * g.best && bcast(b.zn[0], 0) > c.T0 + 200.0) {
              c.stopped = 1;
              st = ST_FINISH;
              break;
            }
          }
          bool adap = false;
          if ((fl & SF_ADAP) && c.nadap < io.max_adap) {
            // ADAP: extra solution points every ASTEPS steps, or when AVAR moved by AVALUE
            if ((fl & SF_ASTEPS) && nst % cfg->asteps == 0) adap = true;
            if ((fl & SF_AVAR) && cfg->avalue > 0.0) {
              const double v = bcast(b.zn[0], cfg->avar);
              if (fabs(v - c.avar_last) >= cfg->avalue) adap = true;
            }
          }
          if (adap) {
            const size_t a = (size_t)c.r * io.max_adap + c.nadap;
            if (lane == 0) io.t_adap[a] = tn;
            if (act) io.y_adap[a * n + lane] = b.zn[0];
            c.nadap++;
            if (fl & SF_AVAR) c.avar_last = bcast(b.zn[0], cfg->avar);
          }
          if (nst >= max_steps) {
            c.status = CKMI_RUN_MAXSTEPS;
            st = ST_FINISH;
            break;
          }
          if ((fl & SF_CRIT) && tn >= c.tc * (1.0 - 1e-15) && c.icrit < c.ncrit - 1) {
            c.icrit++;
            START_BEGIN(tn, b.zn[0], crit_time(dcfg, c.tend, c.icrit), 0.0);
          }
          if constexpr (PSR) {
            // steady-state rule: screened with the history's derivative before the fresh f is paid for
            if (st == ST_STEP_BEGIN && psr_resid(b.zn[1] / S.h, b.zn[0]) <= PSR_SCREEN)
              REQUEST_F(tn, b.zn[0], ST_PSR_SS_F);
          }
          break;
        }
        case ST_FINISH: {
          double yf;
          double tf = c.tend;
          if (c.stopped || c.status) {
            tf = S.tn;
            yf = b.zn[0];
          } else {
            yf = dky0_lane(b, S, c.tend);
          }
          if (g.mode == 1 || g.mode == 4) g.tau = ign_peak_time(g);
          double Pf, Vf;
          state_PV<PF>(V, R, tf, yf, lane, Pf, Vf);
          const int r = c.r;
          // a run that ended early (IGN_STOP, solver failure) has no solution after tf: its
          // remaining DTSV rows are NaN, never stale memory (the host trims them)
          while (c.isave < io.nsave) {
            if (act) io.y_save[((size_t)r * io.nsave + c.isave) * n + lane] = __builtin_nan("");
            c.isave++;
          }
          if (io.t_stop && lane == 0) io.t_stop[r] = tf;
          if constexpr (PSR) {  // density, residence time and volume of the returned state
            const double sYW = wave_sum(isp ? yf * V.rwt()[lane - 1] : 0.0);
            const double rho = R.P0 / (RU * bcast(yf, 0) * sYW);
            if (lane == 0) {
              io.rho[r] = rho;
              io.tau_res[r] = R.pfr == 4 ? rho / R.G : 1.0 / R.G;
              io.vol[r] = R.pfr == 4 ? R.V0 : R.mass / rho;
              io.resid[r] = c.avar_last;
            }
          }
          if (lane == 0) {
            if constexpr (!PSR) io.tau[r] = g.tau;
            io.T[r] = yf;
            if constexpr (!PSR) {
              io.P[r] = Pf;
              io.V[r] = Vf;
            }
            int* sto = io.stats + (size_t)r * CKMI_NSTAT;
            sto[CKMI_STAT_NST] = c.nst;
            sto[CKMI_STAT_NFE] = S.nfe;
            sto[CKMI_STAT_NJE] = S.nje;
            sto[CKMI_STAT_NLU] = S.nlu;
            sto[CKMI_STAT_NCF] = S.ncf_tot;
            sto[CKMI_STAT_NEF] = S.nef_tot;
            sto[CKMI_STAT_STATUS] = c.status;
            sto[CKMI_STAT_NNI] = S.nni;
          }
          if (isp) io.Y[(size_t)r * KK + lane - 1] = yf;
          if (io.n_adap && lane == 0) io.n_adap[r] = c.nadap;
#ifdef CKMI_PHASE_TIMERS
          ph[PH_TOTAL] = __builtin_amdgcn_s_memtime() - t_r0;
          wave_lds_sync();
          if (g_phase_buf && lane < PH_N) {
            unsigned long long v = lane >= PH_STATE ? phs[lane - PH_STATE] : 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) v = (lane == k) ? ph[k] : v;
            g_phase_buf[(size_t)r * PH_N + lane] = v;
          }
#endif
          st = ST_NEXT;
          break;
        }
        default:
          st = ST_EXIT;
          break;
      }
#ifdef CKMI_PHASE_TIMERS
      if (st_in != ST_NEXT && st_in != ST_FINISH && lane == 0) phs[st_in] += __builtin_amdgcn_s_memtime() - t_st;
#endif
    }
    if (st == ST_EXIT) break;
    // the single RHS (+ Jacobian) evaluation site of the integrator
#ifdef CKMI_PHASE_TIMERS
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
#ifdef CKMI_PHASE_TIMERS
    unsigned long long sub[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    fe = reactor_rhs<PL, PF, PSR, true>(V, R, t_e, y_e, L, oJ, N, with_j, Yin, sub);
    ph[with_j ? PH_JAC : PH_RHS] += __builtin_amdgcn_s_memtime() - t0;
    if (!with_j) {
      ph[5] += sub[0];
      ph[6] += sub[1];
      ph[7] += sub[2];
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) phs[24 + k] += sub[3 + k];
      }
    }
#else
    // (LOCK: a with_j call takes the lock at olock = oJ + jlock_offset(N) and returns holding it)
    fe = reactor_rhs<PL, PF, PSR, true>(V, R, t_e, y_e, L, oJ, N, with_j, Yin);
#endif
  }
#undef REQUEST_F
#undef START_BEGIN
}

template <int N, bool F64>
size_t reactor_lds_bytes(const ckmi_mech* m) {
  return (size_t)m->img.bytes + jscratch_bytes<N>() + (size_t)rwaves(F64) * slice_bytes(m->G);
}
// Grid = (CUs x resident workgroups per CU), capped by the batch; J workspace = one
// column-major N x 64 matrix per wave slot, allocated stream-ordered (~55 MB for GRI-3.0).
template <int N, bool PL = false, bool F64 = false, bool PSR = false>
int launch_reactors(const ckmi_mech* m, int n, const DevCfg& dc, const std::conditional_t<PSR, PsrIO, ReactorIO>& io,
                    hipStream_t stream, int sel = SEL_ALL) {
  if (!F64 && sel != SEL_NO_PFR) return set_error(CKMI_ERR_ARG, "internal: FP32-inverse reactor launch must skip plug flow");
  constexpr int RWAVES = rwaves(F64);
  // open reactors: one more [VL] vector per wave (the inlet mass fractions)
  const size_t lds = reactor_lds_bytes<N, F64>(m) + (PSR ? (size_t)RWAVES * 8 * VL : 0);
  if (int rc = raise_lds_limit(m->device, (const void*)reactor_kernel<N, PL, F64, PSR>, lds)) return rc;
  int ncu = 0, per_cu = 0;
  CKMI_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, m->device));
  CKMI_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reactor_kernel<N, PL, F64, PSR>, RWAVES * WAVE, lds));
  if (per_cu < 1) return set_error(CKMI_ERR_SIZE, "reactor kernel does not fit on a CU (LDS " + std::to_string(lds) + " B)");
  const int want = (n + RWAVES - 1) / RWAVES;
  const int grid = std::max(1, std::min(ncu * per_cu, want));
  // the wave's parked Jacobian is FP32 (N x 64 floats per wave slot)
  const size_t jbytes = StreamWorkspace::aligned((size_t)grid * RWAVES * N * WAVE * sizeof(float));
  const size_t cbytes = StreamWorkspace::aligned(sizeof(DevCfg));
  StreamWorkspace ws(stream);
  if (int rc = ws.alloc(jbytes + cbytes + 256)) return rc;
  double* jws = ws.take<double>(jbytes);
  DevCfg* dcfg = ws.take<DevCfg>(cbytes);
  int* queue = ws.take<int>(256);
  if (int rc = stage_cfg(dc, dcfg, stream)) return rc;
  CKMI_HIP_CHECK(hipMemsetAsync(queue, 0, sizeof(int), stream));
  hipLaunchKernelGGL((reactor_kernel<N, PL, F64, PSR>), dim3(grid), dim3(RWAVES * WAVE), lds, stream, m->img, dcfg, n, sel,
                     queue, jws, io);
  CKMI_HIP_CHECK(hipGetLastError());
  return CKMI_OK;
}

// ---------------------------------------------------------------- RHS / Jacobian probe (diagnostic)
// ckmi_reactor_rhs_jac: one wave per state evaluates the integrator's own reactor_rhs<PL, PF, PSR> once, with
// the per-reactor context built from the state's initial condition exactly as ST_NEXT of reactor_kernel builds
// it (engine_heat_kernel of ckmi.hip is the model), and copies f and, on a with_j call, the FP64 Jacobian out
// of the shared scratch Jsh[col * LDJ + row] into J[row][col].  The probe holds its own inlined copy of
// reactor_rhs: it checks the source the integrators are compiled from, not their machine code.
// sel as reactor_kernel: the PF = false instantiation takes problems 1 and 2, the PF = true one the others
// (SEL_PFR) or every state (SEL_ALL); ncol is the N of the reactor_kernel variant the run would use.
template <bool PL, bool PF, bool PSR>
__global__ __launch_bounds__(WAVE) void rhs_probe_kernel(MechImage img, const DevCfg* __restrict__ dcfg, int n, int sel,
                                                         int ncol, ProbeIO io) {
  const ckmi_reactor_cfg* __restrict__ cfg = &dcfg->c;
  stage_image(0, img);
  const MechView V = make_view(0, img);
  const int lane = threadIdx.x;
  const int oJ = img.bytes;
  WaveLds L;
  L.base = oJ + align16(8 * ncol * LDJ);
  RunCtx& R = *lds_at<RunCtx>(L.base + slice_vec_bytes(img.G));
  double* const Yin = PSR ? lds_at<double>(L.base + slice_vec_bytes(img.G) + align16((int)sizeof(RunCtx))) : nullptr;
  const int KK = V.KK;
  const int nv = KK + 1;
  const bool isp = lane >= 1 && lane <= KK;
  const int s = isp ? lane - 1 : 0;
  const double rw = isp ? V.rwt()[s] : 0.0;
  const bool with_j = io.J != nullptr;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    int prob;
    if constexpr (PSR) prob = 5;
    else prob = io.problem[i];
    if (PF ? (sel == SEL_PFR && prob < 3) : prob >= 3) continue;  // the other launch's state
    const double T0 = (cfg->prof_kind == 1 && cfg->energy == 2 && cfg->nprof > 0) ? cfg->prof_v[0] : io.T0[i];
    const double P0 = io.P0[i];
    const double y0 = lane == 0 ? T0 : (isp ? io.Y0[(size_t)i * KK + s] : 0.0);
    const double Wbar0 = 1.0 / wave_sum(isp ? y0 * rw : 0.0);
    double gam0 = 0.0, hin = 0.0;
    if constexpr (PF && !PSR) {
      if (prob == 4) {  // engine: gamma of the initial charge
        const double cpR = isp ? nasa7_img(V, s, T0, log(T0), 1.0 / T0).cpR : 0.0;
        const double cpm = wave_sum(isp ? y0 * cpR * rw : 0.0);
        gam0 = cpm / (cpm - 1.0 / Wbar0);
      }
    }
    if constexpr (PSR) {  // inlet mass fractions into the slice, inlet enthalpy
      const double Tin = io.Tin[i];
      const double yi = isp ? io.Yin[(size_t)i * KK + s] : 0.0;
      if (isp) Yin[s] = yi;
      const double hk = isp ? nasa7_img(V, s, Tin, log(Tin), 1.0 / Tin).hRT * RU * Tin * rw : 0.0;
      hin = wave_sum(yi * hk);
    }
    const double t = io.t[i];
    if (lane == 0) {
      R.cfg = cfg;
      R.pfr = PF ? (prob == 3 ? 1 : (prob == 4 ? 2 : 0)) : 0;
      R.conp = (prob == 1 || prob == 3);
      R.energy = cfg->energy;
      R.npv = cfg->prof_kind == 0 ? cfg->nprof : 0;
      R.ntp = (cfg->prof_kind == 1 && cfg->energy == 2) ? cfg->nprof : 0;
      R.rho0 = P0 * Wbar0 / (RU * T0);
      R.V0 = (!R.conp && R.npv > 0) ? cfg->prof_v[0] : io.V0[i];
      R.P0 = (R.conp && R.npv > 0) ? cfg->prof_v[0] : P0;
      R.G = R.Pm = 0.0;
      if constexpr (PF) {
        if (R.pfr == 2) {
          double dv;
          engine_volume(cfg->eng, 0.0, R.V0, dv);
          R.G = gam0;
          R.Pm = T0;
        }
      }
      R.mass = R.rho0 * R.V0;
      if (PF && R.pfr == 1) {
        R.G = R.rho0 * R.V0;
        R.Pm = R.P0 + R.G * R.V0;
      }
      if constexpr (PSR) {
        const bool vgiven = io.mode == 2;
        const double mdot = io.mdot[i];
        R.conp = 1;
        R.pfr = vgiven ? 4 : 3;
        R.Pm = hin;
        R.G = vgiven ? mdot / R.V0 : 1.0 / R.V0;
        R.mass = vgiven ? R.rho0 * R.V0 : R.V0 * mdot;
      }
      R.gfac = cfg->gfac;
      R.qloss = cfg->qloss;
      R.htc = cfg->htc;
      R.areaq = cfg->areaq;
      R.tamb = cfg->tamb;
      R.nq = cfg->prof2_kind == 1 ? cfg->nprof2 : 0;
      R.na = cfg->prof2_kind == 2 ? cfg->nprof2 : cfg->nprof3;
      R.a_t = cfg->prof2_kind == 2 ? cfg->prof2_t : cfg->prof3_t;
      R.a_v = cfg->prof2_kind == 2 ? cfg->prof2_v : cfg->prof3_v;
      const int ar = io.afac_rxn ? io.afac_rxn[i] : -1;
      R.pslot = (ar >= 0 && ar < img.II) ? img.slot_of[ar] : -1;
      R.plnf = R.pslot >= 0 ? log(io.afac[i]) : 0.0;
      R.tsel = t;  // the profile piece that contains the evaluation point
    }
    wave_lds_sync();
    const double yl = lane <= KK ? io.y[(size_t)i * nv + lane] : 0.0;
#ifdef CKMI_PHASE_TIMERS
    unsigned long long sub[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const double fl = reactor_rhs<PL, PF, PSR>(V, R, t, yl, L, oJ, ncol, with_j, Yin, sub);
#else
    const double fl = reactor_rhs<PL, PF, PSR>(V, R, t, yl, L, oJ, ncol, with_j, Yin);
#endif
    if (lane <= KK) io.f[(size_t)i * nv + lane] = fl;
    if (with_j) {
      wave_lds_sync();
      const double* Jsh = lds_at<const double>(oJ);
      double* Jo = io.J + (size_t)i * nv * nv;
      if (lane <= KK)  // lane = column: coalesced rows out, conflict-free column reads (LDJ is odd)
        for (int r = 0; r < nv; ++r) Jo[(size_t)r * nv + lane] = Jsh[lane * LDJ + r];
    }
    wave_lds_sync();  // R, the slice and the J scratch are rewritten for the next state
  }
}

template <bool PL, bool PF, bool PSR>
int launch_rhs_probe(const ckmi_mech* m, int n, const DevCfg& dc, const ProbeIO& io, int sel, int ncol,
                     hipStream_t stream) {
  const size_t lds = (size_t)m->img.bytes + align16(8 * ncol * LDJ) + slice_vec_bytes(m->G) +
                     align16((int)sizeof(RunCtx)) + (PSR ? 8 * VL : 0);
  int lds_max = 0;
  CKMI_HIP_CHECK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, m->device));
  if (lds > (size_t)lds_max)
    return set_error(CKMI_ERR_SIZE, "mechanism image + probe work space exceed the LDS of a CU");
  if (int rc = raise_lds_limit(m->device, (const void*)rhs_probe_kernel<PL, PF, PSR>, lds)) return rc;
  const size_t cbytes = StreamWorkspace::aligned(sizeof(DevCfg));
  StreamWorkspace ws(stream);
  if (int rc = ws.alloc(cbytes)) return rc;
  DevCfg* dcfg = ws.take<DevCfg>(cbytes);
  if (int rc = stage_cfg(dc, dcfg, stream)) return rc;
  hipLaunchKernelGGL((rhs_probe_kernel<PL, PF, PSR>), dim3(std::min(n, PROBE_GRID_MAX)), dim3(WAVE), lds, stream,
                     m->img, dcfg, n, sel, ncol, io);
  CKMI_HIP_CHECK(hipGetLastError());
  return CKMI_OK;
}

// ---------------------------------------------------------------- Newton-matrix probe (diagnostic)
// ckmi_newton_probe on the wave kernel's matrix forms: one wave per system, in workgroups of the integrator's
// wave count for the form, makes the calls ST_SETUP and ST_NEWTON_ITER of reactor_kernel make -- build_factor(Jg,
// WAVE, gamma, n, orow) on a parked FP32 slot in the kernel's Jg[j * WAVE + lane] layout (rows and columns >= n
// zero) and solve(b, n) -- on one matrix object that lives across the wave's systems, as the persistent loop's
// does.  The waves' scratch rows are neighbours in LDS.  The probe holds its own inlined copy of the member
// functions: it checks the source the integrators are compiled from, not their machine code.
template <int N, bool F64>
__global__ __launch_bounds__(rwaves(F64) * WAVE) void newton_probe_kernel(NewtonProbeIO io, float* __restrict__ jws) {
  constexpr int RWAVES = rwaves(F64);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int n = io.n;
  const int orow = wid * align16(8 * N);
  float* Jg = jws + ((size_t)blockIdx.x * RWAVES + wid) * N * WAVE;
  std::conditional_t<F64, NewtonMatrixGJ64<N>, NewtonMatrixF32S<N>> M;
  for (int s = blockIdx.x * RWAVES + wid; s < io.nsys; s += gridDim.x * RWAVES) {
    bool ok = true;
#pragma unroll 1
    for (int pass = io.Jprev ? 0 : 1; pass < 2; ++pass) {  // pass 0: the set-up before the one that is judged
      const float* Js = (pass ? io.J : io.Jprev) + (size_t)s * n * n;
      const double gamma = (pass ? io.gamma : io.gprev)[s];
      for (int j = 0; j < N; ++j)  // lane = row, read back by the same lane
        Jg[j * WAVE + lane] = (lane < n && j < n) ? Js[(size_t)lane * n + j] : 0.0f;
      ok = M.build_factor(Jg, WAVE, gamma, n, orow);
    }
#pragma unroll 1
    for (int r = 0; r < io.nrhs; ++r) {
      const size_t o = ((size_t)s * io.nrhs + r) * n;
      const double x = M.solve(lane < n ? io.B[o + lane] : io.b_pad, n);
      if (lane < n) io.X[o + lane] = x;
    }
    if (lane < n) io.perm[(size_t)s * n + lane] = M.permv;
    if (lane == 0) io.ok[s] = ok ? 1 : 0;
  }
}

template <int N, bool F64>
int launch_newton_probe(const NewtonProbeIO& io, hipStream_t stream) {
  constexpr int RWAVES = rwaves(F64);
  const int grid = std::min((io.nsys + RWAVES - 1) / RWAVES, PROBE_GRID_MAX);
  const size_t jbytes = StreamWorkspace::aligned((size_t)grid * RWAVES * N * WAVE * sizeof(float));
  StreamWorkspace ws(stream);
  if (int rc = ws.alloc(jbytes)) return rc;
  float* jws = ws.take<float>(jbytes);
  hipLaunchKernelGGL((newton_probe_kernel<N, F64>), dim3(grid), dim3(RWAVES * WAVE), RWAVES * align16(8 * N), stream, io,
                     jws);
  CKMI_HIP_CHECK(hipGetLastError());
  return CKMI_OK;
}

}  // namespace
