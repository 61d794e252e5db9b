// ckmi_psr.hip -- batched steady-state perfectly stirred reactors (ckmi_psr_run, include/ckmi.h): the
// open-reactor instantiations of the wave-per-reactor kernel (ckmi_reactor_kernel.hpp) and their C entry point.
#include "ckmi_reactor_kernel.hpp"

using namespace ckmi;

// ckmi_reactor_rhs_jac on open reactors: the PSR = true instantiation ckmi_psr_run picks
int ckmi::launch_psr_probe(const ckmi_mech* m, int n, const DevCfg& dc, const ProbeIO& io, hipStream_t stream) {
  const WavePlan p = wave_plan(m->KK + 1, m->has_plog, m->has_general, dc.c.rtol, 0, true);
  return p.pl ? launch_rhs_probe<true, true, true>(m, n, dc, io, SEL_ALL, p.n64, stream)
              : launch_rhs_probe<false, true, true>(m, n, dc, io, SEL_ALL, p.n64, stream);
}

extern "C" {

int ckmi_psr_run(const ckmi_mech* m, const ckmi_reactor_cfg* cfg, const ckmi_psr_cfg* psr, int32_t n, const double* P,
                 const double* Tin, const double* Yin, const double* mdot, const double* tau_or_vol,
                 const double* Tguess, const double* Yguess, double* Tss, double* Yss, double* rho, double* tau_res,
                 double* vol, double* resid, int32_t* stats, void* stream) {
  if (!m || !cfg || !psr || n < 0) return set_error(CKMI_ERR_ARG, "bad argument");
  if (psr->mode != 1 && psr->mode != 2) return set_error(CKMI_ERR_ARG, "psr mode must be 1 (residence time) or 2 (volume)");
  if (!(psr->ss_rtol > 0.0) || !(psr->ss_atol >= 0.0)) return set_error(CKMI_ERR_ARG, "ss_rtol must be > 0 and ss_atol >= 0");
  if (!(cfg->t_end >= 0.0) || !(cfg->rtol > 0.0) || !(cfg->atol > 0.0))
    return set_error(CKMI_ERR_ARG, "t_end must be >= 0 (0: 1000 residence times), rtol and atol > 0");
  if (cfg->ign_mode != 0 || cfg->ign_stop) return set_error(CKMI_ERR_ARG, "ignition detection does not apply to a PSR");
  if (cfg->nprof != 0 || cfg->nprof2 != 0 || cfg->nprof3 != 0) return set_error(CKMI_ERR_ARG, "profiles do not apply to a PSR");
  if (cfg->asteps != 0 || cfg->avar >= 0) return set_error(CKMI_ERR_ARG, "adaptive saving does not apply to a PSR");
  if (int rc = check_reactor_cfg(cfg, nullptr, false)) return rc;
  if (m->KK + 1 > WAVE_NMAX)
    return set_error(CKMI_ERR_UNSUPPORTED, "PSRs need KK + 1 <= 64 (the wave-per-reactor kernel); this mechanism has " +
                                          std::to_string(m->KK) + " species");
  if (n > 0 && (!P || !Tin || !Yin || !mdot || !tau_or_vol || !Tguess || !Yguess || !Tss || !Yss || !rho || !tau_res ||
                !vol || !resid || !stats))
    return set_error(CKMI_ERR_ARG, "every input and output array is required");
  if (n == 0) return CKMI_OK;
  const DevCfg dc = make_dev_cfg(m, cfg, false);  // (no element projection: see make_dev_cfg)
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
  // the FP64-inverse variants, whatever the tolerances and the path
  const WavePlan p = wave_plan(m->KK + 1, m->has_plog, m->has_general, cfg->rtol, 0, true);
  const int rc = visit_wave_variant<true>(p.n64, p.pl, [&](auto N, auto PL) {
    return launch_reactors<decltype(N)::value, decltype(PL)::value, true, true>(m, n, dc, io, st);
  });
  if (rc) return rc;
  CKMI_HIP_CHECK(hipGetLastError());
  return CKMI_OK;
}

}  // extern "C"
