// ckmi_dispatch.hpp -- which compiled variant of the two integrator kernels a mechanism and a configuration
// get.  Host-only and free of HIP: the two pure functions below are the only place the rules are written, and
// the two visitors the only place a plan becomes template arguments.  ckmi_reactor_run_ex, ckmi_psr_run, the
// probes of ckmi_reactor_rhs_jac, ckmi_big_max_image_bytes and the query ckmi_reactor_variant all go through
// them (tests/test_size_variants_host.py holds the query against the tests' own restatement).
#pragma once
#include <string>
#include <type_traits>

#include "../../include/ckmi.h"

namespace ckmi {

// record the message for ckmi_last_error() and return code (ckmi.hip)
int set_error(int code, const std::string& msg);

constexpr int WAVE_NMAX = 64;  // KK + 1 of the wave-per-reactor kernel (ckmi_reactor_kernel.hpp)
constexpr int BIG_NMAX = 192;  // KK + 1 of the workgroup-per-reactor kernel (ckmi_big.hip)

// closed reactors leave the wave kernel above its size or when the workgroup path is forced (path 1); open
// reactors and engines exist in the wave kernel only
constexpr bool use_workgroup_kernel(int nvar, int path) { return nvar > WAVE_NMAX || path == 1; }

// what the FP64-inverse launch of the wave kernel takes
enum { F64_TAKES_ALL = 0, F64_TAKES_PFR = 1, F64_TAKES_PFR_RETRY = 2 };

// reactor_kernel<N, PL, F64, PSR>: an FP32-inverse launch (problems 1 and 2; none when n32 = 0) and an
// FP64-inverse launch behind it
struct WavePlan {
  bool pl;
  int n32;        // N of the FP32-inverse launch, 0 = none
  int n64;        // N of the FP64-inverse launch
  int f64_takes;  // F64_TAKES_*
};

// PLOG mechanisms use one (64-wide) variant, so that the PLOG branch costs compile time once.  The Newton
// inverse is stored in FP64 alone when the tolerances ask for more than its FP32 rounding resolves
// (rtol < 1e-9; measured: the FP32-stored inverse integrates the rtol = 1e-8 sweeps of configs[2] and [3]
// without a failure, and fails one of 55 reactors at rtol = 1e-10, atol = 1e-20), and for mechanisms with
// FORD / RORD / fractional orders, whose d C^o / dC = o C^(o-1) grows without bound as C -> 0 (the
// FP32-stored inverse of such a Newton matrix stalled one reactor of five).  path: ckmi_set_reactor_path
// (2 forces the FP64 inverse, 3 the FP32-stored one).  Otherwise the FP32-inverse launch skips the plug-flow
// and engine reactors and the FP64-inverse launch follows it for them; on the automatic path the 64-wide
// variants also let it take again what the FP32-inverse launch failed on (error test, convergence), while a
// forced path keeps the FP32 inverse's own status.  Open reactors use the FP64-inverse variant, whatever the
// tolerances and the path.
constexpr WavePlan wave_plan(int nvar, bool has_plog, bool has_general, double rtol, int path, bool open_reactor) {
  const int n64 = (has_plog || nvar > 54) ? 64 : 54;
  const bool f64_alone = open_reactor || path == 2 || (path != 3 && (rtol < 1e-9 || has_general));
  if (f64_alone) return {has_plog, 0, n64, F64_TAKES_ALL};
  const int n32 = (!has_plog && nvar <= 32) ? 32 : n64;
  return {has_plog, n32, n64, (path == 0 && n64 == 64) ? F64_TAKES_PFR_RETRY : F64_TAKES_PFR};
}

// big_reactor_kernel<NB, PL>: NB register blocks per dimension (NC = 16 NB >= nvar); nb = 0 above BIG_NMAX.
// PLOG, chemically activated and general (FORD / RORD / fractional) reactions: the extended variant,
// compiled for three matrix sizes (a mechanism runs in the smallest that holds it)
struct BigPlan {
  int nb;
  bool pl;
};
constexpr BigPlan big_plan(int nvar, bool has_plog) {
  if (nvar > BIG_NMAX) return {0, has_plog};
  if (has_plog) return {nvar <= 128 ? 8 : (nvar <= 176 ? 11 : 12), true};
  const int nb = (nvar + 15) / 16;
  return {nb < 4 ? 4 : (nb > 12 ? 12 : nb), false};
}

template <int V>
using int_c = std::integral_constant<int, V>;

// f(int_c<N>, std::bool_constant<PL>) for the (N, PL) of one launch of a WavePlan; F64 names the launch, since
// the 32-wide variant exists with the FP32-stored inverse only.  ISA probe build (-DCKMI_PROBE_C3,
// scripts/isa_probe.sh): only the configs[2] kernel is instantiated, so that its register / scratch figures
// come out of a one-variant compile; never linked into libckmi.so
template <bool F64, class F>
int visit_wave_variant(int N, bool PL, F&& f) {
#ifdef CKMI_PROBE_C3
  if constexpr (F64) return CKMI_OK;
  else return f(int_c<54>{}, std::false_type{});
#else
  if (PL && N == 64) return f(int_c<64>{}, std::true_type{});
  if (!PL && N == 54) return f(int_c<54>{}, std::false_type{});
  if (!PL && N == 64) return f(int_c<64>{}, std::false_type{});
  if constexpr (!F64)
    if (!PL && N == 32) return f(int_c<32>{}, std::false_type{});
  return set_error(CKMI_ERR_ARG, "internal: no such wave reactor kernel variant");
#endif
}

// f(int_c<NB>, std::bool_constant<PL>) for a BigPlan (nb != 0).  -DCKMI_BIG_ONLY_NB=<NB>: diagnostics, compile
// one matrix size only (register-usage checks), no extended variants
template <class F>
int visit_big_variant(BigPlan p, F&& f) {
#ifdef CKMI_BIG_ONLY_NB
  if (p.pl) return set_error(CKMI_ERR_UNSUPPORTED, "diagnostic build: no extended variants");
  return f(int_c<CKMI_BIG_ONLY_NB>{}, std::false_type{});
#else
  if (p.pl) {
    switch (p.nb) {
      case 8: return f(int_c<8>{}, std::true_type{});
      case 11: return f(int_c<11>{}, std::true_type{});
      case 12: return f(int_c<12>{}, std::true_type{});
      default: break;
    }
  } else {
    switch (p.nb) {
      case 4: return f(int_c<4>{}, std::false_type{});
      case 5: return f(int_c<5>{}, std::false_type{});
      case 6: return f(int_c<6>{}, std::false_type{});
      case 7: return f(int_c<7>{}, std::false_type{});
      case 8: return f(int_c<8>{}, std::false_type{});
      case 9: return f(int_c<9>{}, std::false_type{});
      case 10: return f(int_c<10>{}, std::false_type{});
      case 11: return f(int_c<11>{}, std::false_type{});
      case 12: return f(int_c<12>{}, std::false_type{});
      default: break;
    }
  }
  return set_error(CKMI_ERR_ARG, "internal: no such workgroup reactor kernel variant");
#endif
}

}  // namespace ckmi
