// ckmi_psr.hip -- batched steady-state perfectly stirred reactors (ckmi_psr_run, include/ckmi.h): the
// open-reactor instantiations of the wave-per-reactor kernel (ckmi_reactor_kernel.hpp) and their C entry point.
#include "ckmi_reactor_kernel.hpp"

using namespace ckmi;

#define HIP_CHECK(x) CKMI_RK_HIP_CHECK(x)
static int fail(int code, const std::string& msg) { return ckmi::set_error(code, msg); }

// ckmi_reactor_rhs_jac on open reactors: the PSR = true instantiation ckmi_psr_run would pick
int ckmi::launch_psr_probe(const ckmi_mech* m, int n, const DevCfg& dc, const ProbeIO& io, hipStream_t stream) {
  const int nvar = m->KK + 1;
  if (m->has_plog) return launch_rhs_probe<true, true, true>(m, n, dc, io, SEL_ALL, 64, stream);
  return launch_rhs_probe<false, true, true>(m, n, dc, io, SEL_ALL, nvar <= 54 ? 54 : 64, stream);
}

extern "C" {

int ckmi_psr_run(const ckmi_mech* m, const ckmi_reactor_cfg* cfg, const ckmi_psr_cfg* psr, int32_t n, const double* P,
                 const double* Tin, const double* Yin, const double* mdot, const double* tau_or_vol,
                 const double* Tguess, const double* Yguess, double* Tss, double* Yss, double* rho, double* tau_res,
                 double* vol, double* resid, int32_t* stats, void* stream) {
  if (!m || !cfg || !psr || n < 0) return fail(CKMI_ERR_ARG, "bad argument");
  if (psr->mode != 1 && psr->mode != 2) return fail(CKMI_ERR_ARG, "psr mode must be 1 (residence time) or 2 (volume)");
  if (!(psr->ss_rtol > 0.0) || !(psr->ss_atol >= 0.0)) return fail(CKMI_ERR_ARG, "ss_rtol must be > 0 and ss_atol >= 0");
  if (!(cfg->t_end >= 0.0) || !(cfg->rtol > 0.0) || !(cfg->atol > 0.0))
    return fail(CKMI_ERR_ARG, "t_end must be >= 0 (0: 1000 residence times), rtol and atol > 0");
  if (cfg->energy != 1 && cfg->energy != 2) return fail(CKMI_ERR_ARG, "energy must be 1 or 2");
  if (cfg->ign_mode != 0 || cfg->ign_stop) return fail(CKMI_ERR_ARG, "ignition detection does not apply to a PSR");
  if (cfg->nprof != 0 || cfg->nprof2 != 0 || cfg->nprof3 != 0) return fail(CKMI_ERR_ARG, "profiles do not apply to a PSR");
  if (cfg->asteps != 0 || cfg->avar >= 0) return fail(CKMI_ERR_ARG, "adaptive saving does not apply to a PSR");
  if (!(cfg->gfac >= 0.0)) return fail(CKMI_ERR_ARG, "GFAC must be >= 0");
  if (!(cfg->htc >= 0.0) || !(cfg->areaq >= 0.0) || !(cfg->tamb > 0.0 || cfg->htc * cfg->areaq == 0.0))
    return fail(CKMI_ERR_ARG, "HTC, AREAQ must be >= 0 and TAMB > 0");
  if (m->KK + 1 > WAVE)
    return fail(CKMI_ERR_UNSUPPORTED, "PSRs need KK + 1 <= 64 (the wave-per-reactor kernel); this mechanism has " +
                                          std::to_string(m->KK) + " species");
  if (n > 0 && (!P || !Tin || !Yin || !mdot || !tau_or_vol || !Tguess || !Yguess || !Tss || !Yss || !rho || !tau_res ||
                !vol || !resid || !stats))
    return fail(CKMI_ERR_ARG, "every input and output array is required");
  if (n == 0) return CKMI_OK;
  DevCfg dc;
  dc.c = *cfg;
  if (dc.c.gfac == 0.0) dc.c.gfac = 1.0;
  dc.ncrit = 0;
  dc.guard_y = std::max(1e-3, 1e3 * cfg->atol);
  dc.guard_tlo = m->tguard_lo;
  dc.guard_thi = m->tguard_hi;
  dc.npe = 0;  // an open reactor relaxes to the inlet's element content, not the estimate's
  PsrIO io{};
  io.T0 = Tguess;
  io.P0 = P;
  io.V0 = tau_or_vol;
  io.Y0 = Yguess;
  io.T = Tss;
  io.Y = Yss;
  io.stats = stats;
  io.Tin = Tin;
  io.Yin = Yin;
  io.mdot = mdot;
  io.tau_or_vol = tau_or_vol;
  io.rho = rho;
  io.tau_res = tau_res;
  io.vol = vol;
  io.resid = resid;
  io.mode = psr->mode;
  io.ss_rtol = psr->ss_rtol;
  io.ss_atol = psr->ss_atol;
  const hipStream_t st = (hipStream_t)stream;
  const int nvar = m->KK + 1;
  int rc;
  // the FP64-inverse variants, whatever the tolerances: N = 54, N = 64 and the PLOG variant
  if (m->has_plog) rc = launch_reactors<64, true, true, true>(m, n, dc, io, st);
  else if (nvar <= 54) rc = launch_reactors<54, false, true, true>(m, n, dc, io, st);
  else rc = launch_reactors<64, false, true, true>(m, n, dc, io, st);
  if (rc) return rc;
  HIP_CHECK(hipGetLastError());
  return CKMI_OK;
}

}  // extern "C"
